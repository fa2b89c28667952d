"""Graphs for the tests of the inertial local-BA window: the small keyframe store of ba_window_cases.py (the "world"), a generator of flat
graphs around one current keyframe and its chain of predecessors, a builder for hand-made graphs of a few keyframes, the flat graph of a
synthetic inertial window, and the comparison (integers and floats widened to double: equality)."""
import numpy as np

import inertial_window_ref as ref
from ba_window_cases import BOUNDS, EMPTY_SLOT, KEYPOINT_DTYPE, N_LEVELS, SIGMA, WORLD, WORLD_SLOTS, edge   # noqa: F401 -- the same world

BAD, OTHER_MAP, IMU, PREINT = 1, 2, 4, 8                                              # kf_flags


def states_of(rng, n):
    """n keyframe states as the map holds them (floats, widened)"""
    return rng.normal(0, 3, (n, 33)).astype(np.float32).astype(np.float64)


def make_graph(seed, n_kf, n_points, chain=None, in_map=None, large=None, rec_init=None, with_lidar=None, views=WORLD, bad=0.12, other=0.08,
               imu=0.85, preint=0.85, minus=0.1, max_obs=6, held=0.9, point_bad=0.05, point_other=0.05, old=None):
    """One gather.  n_kf keyframe rows over the occupied slots (several rows may name one slot), ids in an order of their own; `chain` of
    them (default: 1 .. min(n_kf, 30) drawn) are linked by prev_kf from a current keyframe backwards, in rows of no order; the flags are
    drawn per keyframe; n_points points with 1 .. max_obs observers, an observation's index -1 with probability `minus`, bad and other-map
    points.  The chain keyframes hold a share `held` of the points they observe, shuffled, with NULL slots, points held twice and points
    they do not observe.  old: the share of observers drawn from outside the chain (default: as it falls)."""
    rng = np.random.default_rng(seed)
    occupied = np.array([s for s, v in enumerate(views) if v is not None])
    kf_slot = rng.choice(occupied, n_kf).astype(np.int32)
    kf_id = (rng.permutation(4 * n_kf)[:n_kf].astype(np.int64) + 1) * 1000003 + (1 << 33)      # beyond 32 bits, order unlike the rows'
    flags = ((rng.random(n_kf) < bad) * BAD + (rng.random(n_kf) < other) * OTHER_MAP + (rng.random(n_kf) < imu) * IMU +
             (rng.random(n_kf) < preint) * PREINT).astype(np.uint8)
    chain = int(rng.integers(1, min(n_kf, 30) + 1)) if chain is None else min(chain, n_kf)
    rows = rng.permutation(n_kf)[:chain]
    prev_kf = np.full(n_kf, -1, np.int32)
    prev_kf[rows[:-1]] = rows[1:]
    cur = int(rows[0])
    large = bool(rng.integers(0, 2)) if large is None else large
    in_map = int(rng.integers(1, 32)) if in_map is None else in_map
    Nd = min(in_map - 2, 25 if large else 10)
    holders = rows[:max(Nd, 1)]
    outside = np.setdiff1d(np.arange(n_kf), rows[:max(Nd, 1) + 1])
    point_flags = ((rng.random(n_points) < point_bad) * 1 + (rng.random(n_points) < point_other) * 2).astype(np.uint8)
    n_obs = rng.integers(1, min(max_obs, n_kf) + 1, n_points)
    if old is None or not len(outside):
        per = [np.sort(rng.choice(n_kf, int(m), replace=False)) for m in n_obs]
    else:                                                                              # one holder, the rest mostly from outside the window
        per = [np.unique(np.r_[rng.choice(holders), rng.choice(outside if rng.random() < old else n_kf, int(m) - 1)]) for m in n_obs]
    n_obs = np.array([len(x) for x in per])
    obs_offsets = np.r_[0, np.cumsum(n_obs)].astype(np.int32)
    obs_kf = np.concatenate(per).astype(np.int32)
    n_keys = np.array([len(views[s]["keys"]) for s in kf_slot])
    obs_index = np.where(rng.random(len(obs_kf)) < minus, -1, rng.integers(0, 1 << 30, len(obs_kf)) % n_keys[obs_kf]).astype(np.int32)
    point_of_obs = np.repeat(np.arange(n_points), n_obs)
    slot_offsets, slot_point = [0], []
    hold = set(holders.tolist())
    for k in range(n_kf):
        row = np.zeros(0, np.int64)
        if k in hold:
            mine = point_of_obs[obs_kf == k]
            mine = mine[rng.random(len(mine)) < held]
            extra = rng.integers(0, n_points, max(1, len(mine) // 8))                 # points held twice, points not observed, NULL slots
            row = rng.permutation(np.r_[mine, extra, rng.choice(mine, len(mine) // 8) if len(mine) else mine, -np.ones(1 + len(mine) // 6, np.int64)])
        slot_point.append(row)
        slot_offsets.append(slot_offsets[-1] + len(row))
    return dict(kf_slot=kf_slot, kf_id=kf_id, kf_flags=flags, prev_kf=prev_kf, states=states_of(rng, n_kf), slot_offsets=np.array(slot_offsets, np.int32),
                slot_point=np.concatenate(slot_point).astype(np.int32), current=cur, keyframes_in_map=in_map, large=int(large),
                rec_init=int(rng.integers(0, 2)) if rec_init is None else int(rec_init),
                with_lidar=int(rng.integers(0, 2)) if with_lidar is None else int(with_lidar), point_flags=point_flags,
                positions=rng.normal(0, 10, (n_points, 3)).astype(np.float32).astype(np.float64), obs_offsets=obs_offsets, obs_kf=obs_kf,
                obs_index=obs_index)


def family(lds_keyframes, lds_points):
    """About 40 graphs of 5-40 keyframes and 20-400 points, then the ones aimed at single branches, one graph just beyond each LDS limit of
    tc2li_inertial_window_limits, one beyond both, and one with more than 200 candidate observers (the cap of :605)."""
    rng = np.random.default_rng(78)
    out = []
    for i in range(30):
        out.append(make_graph(600 + i, int(rng.integers(5, 41)), int(rng.integers(20, 401))))
    out += [make_graph(700, 5, 40, chain=1, in_map=1),                                # a window of one keyframe without predecessor: EMPTY
            make_graph(701, 8, 60, chain=1, in_map=30, large=True),                   # the same with a large Nd
            make_graph(702, 12, 120, chain=2, in_map=2),                              # Nd = 0: the current keyframe alone, its predecessor fixed
            make_graph(703, 12, 150, chain=4, in_map=30, large=True, bad=0),          # the chain ends early: the oldest keyframe is popped
            make_graph(704, 30, 300, chain=30, in_map=40, large=True, with_lidar=1),  # 25 optimisable keyframes, LiDAR
            make_graph(705, 30, 300, chain=30, in_map=40, large=False, with_lidar=1), # 10
            make_graph(706, 20, 200, chain=7, in_map=9, with_lidar=1, bad=0.3),       # Nd = 7 cuts the chain: 7 keyframes, LiDAR by position
            make_graph(707, 20, 200, chain=6, in_map=30, large=True, with_lidar=1),   # six in the chain, the sixth popped: five, no LiDAR
            make_graph(708, 40, 400, chain=12, in_map=30, large=True, bad=0.5, old=0.9),   # many bad observers outside the window
            make_graph(709, 16, 257, chain=5, in_map=30, minus=0.7, imu=0.3, preint=0.3)]
    out.append(make_graph(800, lds_keyframes + 1, 400, chain=9, in_map=30, large=True, max_obs=6, old=0.8))
    out.append(make_graph(801, 12, lds_points + 1, chain=6, in_map=30, max_obs=3))
    out.append(make_graph(802, lds_keyframes + 1, lds_points + 1, chain=26, in_map=30, large=True, max_obs=2, old=0.7))
    out.append(make_graph(803, 700, 900, chain=8, in_map=30, large=True, max_obs=4, old=1.0, bad=0.1))   # more than 200 candidates
    return out


def hand(kfs, points, current, in_map=30, large=False, rec_init=False, with_lidar=False):
    """A hand-made graph over WORLD.  kfs: dicts with slot, id and optionally flags (default IMU | PREINT), prev (a row) and holds (its slots:
    points or -1); points: dicts with obs = {keyframe row: keypoint index or -1} and optionally flags.  State of row k: 33 times k + 0.5;
    position of point p: (p, 0.5, 2)."""
    so = np.cumsum([0] + [len(k.get("holds", [])) for k in kfs])
    oo = np.cumsum([0] + [len(p["obs"]) for p in points])
    return dict(kf_slot=np.array([k["slot"] for k in kfs], np.int32), kf_id=np.array([k["id"] for k in kfs], np.int64),
                kf_flags=np.array([k.get("flags", IMU | PREINT) for k in kfs], np.uint8), prev_kf=np.array([k.get("prev", -1) for k in kfs], np.int32),
                states=np.array([[i + 0.5] * 33 for i in range(len(kfs))], np.float64).reshape(-1, 33), slot_offsets=so.astype(np.int32),
                slot_point=np.array([s for k in kfs for s in k.get("holds", [])], np.int32), current=current, keyframes_in_map=in_map,
                large=int(large), rec_init=int(rec_init), with_lidar=int(with_lidar), point_flags=np.array([p.get("flags", 0) for p in points], np.uint8),
                positions=np.array([[i, 0.5, 2] for i in range(len(points))], np.float64).reshape(-1, 3), obs_offsets=oo.astype(np.int32),
                obs_kf=np.array([k for p in points for k in sorted(p["obs"])], np.int32),
                obs_index=np.array([p["obs"][k] for p in points for k in sorted(p["obs"])], np.int32))


def from_inertial_window(w, first_id=100):
    """The flat graph and the store contents behind a synthetic inertial window (synthetic.inertial_window): keyframe row k = keyframe k in
    slot k with one keypoint per edge of the keyframe; keyframe 0 is the predecessor of keyframe 1, and so on; the current keyframe is the
    last; the optimisable keyframes hold the points they observe; keyframes_in_map = n_opt + 2, so that the window is exactly the synthetic
    one.  -> (views, problem, inv_level_sigma2)."""
    e = w["edges"]
    K, P = len(w["kf33"]), len(w["points"])
    pt, po = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    sigma = (1.0 / 1.2 ** (2 * np.arange(N_LEVELS))).astype(np.float32)               # the window's own table as floats
    level = np.argmin(np.abs(e[:, 5][:, None] - sigma.astype(np.float64)[None, :]), 1)
    idx = np.zeros(len(e), np.int64)
    views = []
    for k in range(K):
        m = np.flatnonzero(po == k)
        idx[m] = np.arange(len(m))
        keys = np.zeros(len(m), KEYPOINT_DTYPE)
        keys["x"], keys["y"], keys["octave"], keys["size"] = e[m, 2], e[m, 3], level[m], 31
        ur = e[m, 4].astype(np.float32)
        views.append(dict(keys=keys, u_right=ur, depth=np.where(ur >= 0, 10.0, -1.0).astype(np.float32), descriptors=np.zeros((len(m), 32), np.uint8),
                          fv_node=np.zeros(0, np.int32), fv_offset=np.zeros(1, np.int32), fv_index=np.zeros(0, np.int32)))
    free = np.flatnonzero(np.asarray(w["fixed"]) == 0)
    assert free.tolist() == list(range(1, K))
    order = np.lexsort((po, pt))                                                      # point-major, rows ascending
    n_obs = np.bincount(pt, minlength=P)
    slot_offsets, slot_point = [0], []
    for k in range(K):
        row = pt[po == k] if k in free else np.zeros(0, np.int64)                     # slot i = keypoint i
        slot_point.append(row)
        slot_offsets.append(slot_offsets[-1] + len(row))
    flags = np.where(np.asarray(w["has_imu"]) != 0, IMU | PREINT, 0).astype(np.uint8)
    pr = dict(kf_slot=np.arange(K, dtype=np.int32), kf_id=np.arange(K, dtype=np.int64) + first_id, kf_flags=flags,
              prev_kf=np.arange(K, dtype=np.int32) - 1, states=np.asarray(w["kf33"], np.float64), slot_offsets=np.array(slot_offsets, np.int32),
              slot_point=np.concatenate(slot_point).astype(np.int32), current=K - 1, keyframes_in_map=len(free) + 2, large=int(len(free) > 10),
              rec_init=0, with_lidar=0, point_flags=np.zeros(P, np.uint8), positions=np.asarray(w["points"], np.float64),
              obs_offsets=np.r_[0, np.cumsum(n_obs)].astype(np.int32), obs_kf=po[order].astype(np.int32), obs_index=idx[order].astype(np.int32))
    return views, pr, sigma


def assert_equal(got, want, what=""):
    for k in ref.OUTPUTS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if k == "edges":
            assert len(g) == len(w), (what, k, len(g), len(w))
            for f in ref.EDGE_DTYPE.names:
                assert np.array_equal(g[f], w[f]), (what, k, f, g[f], w[f])
        else:
            assert g.shape == w.shape and np.array_equal(g, w), (what, k, g, w)
    if "link_null" in got:
        assert got["link_null"], (what, "a link came back with a preintegrated pointer or padding set")

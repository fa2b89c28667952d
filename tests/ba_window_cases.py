"""Graphs for the tests of the local-BA window: a small keyframe store (the "world"), a generator of flat graphs around one current
keyframe, a builder for hand-made graphs of a few keyframes, the flat graph of a synthetic BA window, and the comparison (integers and
floats widened to double: equality)."""
import numpy as np

import ba_window_ref as ref

N_LEVELS = 8
SIGMA = (np.float32(1.0) / (np.float32(1.2) ** np.arange(N_LEVELS, dtype=np.float32)) ** 2).astype(np.float32)   # mvInvLevelSigma2
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
WORLD_SLOTS, EMPTY_SLOT = 16, 13


def make_view(rng, n, mono=0.3):
    """What a store slot holds of a keyframe: n keypoints, a share `mono` of them without a right coordinate."""
    keys = np.zeros(n, KEYPOINT_DTYPE)
    keys["x"], keys["y"] = rng.uniform(1, 1240, n).astype(np.float32), rng.uniform(1, 375, n).astype(np.float32)
    keys["octave"] = rng.integers(0, N_LEVELS, n)
    keys["size"], keys["angle"], keys["response"] = 31 * 1.2 ** keys["octave"], rng.uniform(0, 360, n), rng.uniform(1, 100, n)
    ur = np.where(rng.random(n) < mono, -1.0, keys["x"] - rng.uniform(0, 60, n)).astype(np.float32)
    ur[(ur < 0) & (ur != -1)] = 0.0
    return dict(keys=keys, u_right=ur, depth=np.where(ur >= 0, 10.0, -1.0).astype(np.float32), descriptors=rng.integers(0, 256, (n, 32)).astype(np.uint8),
                fv_node=np.zeros(0, np.int32), fv_offset=np.zeros(1, np.int32), fv_index=np.zeros(0, np.int32))


def world(seed=1):
    """WORLD_SLOTS slots: 8 to 64 keypoints each (one of each bound), slot EMPTY_SLOT empty."""
    rng = np.random.default_rng(seed)
    n = rng.integers(8, 65, WORLD_SLOTS)
    n[0], n[1] = 64, 8
    return [None if s == EMPTY_SLOT else make_view(rng, int(n[s])) for s in range(WORLD_SLOTS)]


WORLD = world()


def make_graph(seed, n_kf, n_points, n_cov=None, views=WORLD, bad=0.1, other=0.08, cloud=0.4, minus=0.1, init="any", max_obs=6, held=0.9):
    """One gather.  n_kf keyframe rows over the occupied slots (several rows may name one slot), ids in an order of their own; a current
    keyframe and n_cov others as its covisibility list in random order; bad / other-map / cloud flags drawn per keyframe; n_points points with
    1 .. max_obs observers, an observation's index -1 with probability `minus`, bad and other-map points.  The current keyframe and the listed
    neighbours hold a share `held` of the points they observe, shuffled, with NULL slots, points held twice and points they do not observe.
    init: "local" the initial keyframe is the current one or a neighbour, "other" another row, "none" no row, "any" one of the three."""
    rng = np.random.default_rng(seed)
    occupied = np.array([s for s, v in enumerate(views) if v is not None])
    kf_slot = rng.choice(occupied, n_kf).astype(np.int32)
    kf_id = (rng.permutation(4 * n_kf)[:n_kf].astype(np.int64) + 1) * 1000003 + (1 << 33)      # beyond 32 bits, order unlike the rows'
    flags = ((rng.random(n_kf) < bad) * 1 + (rng.random(n_kf) < other) * 2 + (rng.random(n_kf) < cloud) * 4).astype(np.uint8)
    cur = int(rng.integers(0, n_kf))
    others = np.array([k for k in range(n_kf) if k != cur], np.int64)
    n_cov = int(rng.integers(0, len(others) + 1)) if n_cov is None else min(n_cov, len(others))
    cov = rng.permutation(others)[:n_cov].astype(np.int32)
    kind = init if init != "any" else ("local", "other", "none")[int(rng.integers(0, 3))]
    rest = np.setdiff1d(others, cov)
    init_id = int(kf_id[rng.choice(np.r_[cur, cov])]) if kind == "local" else int(kf_id[rng.choice(rest)]) if kind == "other" and len(rest) else 7
    point_flags = ((rng.random(n_points) < 0.05) * 1 + (rng.random(n_points) < 0.05) * 2).astype(np.uint8)
    n_obs = rng.integers(1, min(max_obs, n_kf) + 1, n_points)
    obs_offsets = np.r_[0, np.cumsum(n_obs)].astype(np.int32)
    obs_kf = np.concatenate([np.sort(rng.choice(n_kf, int(m), replace=False)) for m in n_obs]).astype(np.int32)
    n_keys = np.array([len(views[s]["keys"]) for s in kf_slot])
    obs_index = np.where(rng.random(len(obs_kf)) < minus, -1, rng.integers(0, 1 << 30, len(obs_kf)) % n_keys[obs_kf]).astype(np.int32)
    point_of_obs = np.repeat(np.arange(n_points), n_obs)
    slot_offsets, slot_point = [0], []
    holders = set([cur] + cov.tolist())
    for k in range(n_kf):
        row = np.zeros(0, np.int64)
        if k in holders:
            mine = point_of_obs[obs_kf == k]
            mine = mine[rng.random(len(mine)) < held]
            extra = rng.integers(0, n_points, max(1, len(mine) // 8))                 # points held twice, points not observed, NULL slots
            row = rng.permutation(np.r_[mine, extra, rng.choice(mine, len(mine) // 8) if len(mine) else mine, -np.ones(1 + len(mine) // 6, np.int64)])
        slot_point.append(row)
        slot_offsets.append(slot_offsets[-1] + len(row))
    poses7 = np.c_[rng.normal(0, 1, (n_kf, 4)), rng.normal(0, 5, (n_kf, 3))].astype(np.float32).astype(np.float64)
    return dict(kf_slot=kf_slot, kf_id=kf_id, kf_flags=flags, poses7=poses7, slot_offsets=np.array(slot_offsets, np.int32),
                slot_point=np.concatenate(slot_point).astype(np.int32), cov_kf=cov, current=cur, init_kf_id=init_id, point_flags=point_flags,
                positions=rng.normal(0, 10, (n_points, 3)).astype(np.float32).astype(np.float64), obs_offsets=obs_offsets, obs_kf=obs_kf,
                obs_index=obs_index)


def family(lds_keyframes, lds_points):
    """About 40 graphs of 3-12 keyframes and 20-300 points, one graph just beyond each LDS limit of tc2li_ba_window_limits (as few points /
    keyframes as that allows; the first also has more than 256 neighbours and poses, so that every chunked loop of the kernel goes round
    more than once), and one beyond both: the kernel has a form for each of the four combinations."""
    rng = np.random.default_rng(77)
    out = []
    for i in range(30):
        out.append(make_graph(200 + i, int(rng.integers(3, 13)), int(rng.integers(20, 301))))
    # aimed at single branches: nobody fixed (ABORTED unless the initial keyframe is local), clouds few and many, indices mostly -1
    out += [make_graph(300, 6, 40, n_cov=5, bad=0, other=0, init="none"), make_graph(301, 6, 40, n_cov=5, bad=0, other=0, init="local"),
            make_graph(302, 12, 120, n_cov=11, cloud=1.0, bad=0, init="other"), make_graph(303, 12, 120, n_cov=9, cloud=0.15, init="other"),
            make_graph(304, 8, 60, n_cov=3, minus=0.7), make_graph(305, 5, 20, n_cov=0), make_graph(306, 3, 300, n_cov=2, held=1.0, bad=0),
            make_graph(307, 12, 300, bad=0.4, other=0.3), make_graph(308, 10, 257, n_cov=4, held=1.0, max_obs=2)]
    out.append(make_graph(400, lds_keyframes + 1, 400, n_cov=300, max_obs=6))
    out.append(make_graph(401, 6, lds_points + 1, n_cov=3, max_obs=3))
    out.append(make_graph(402, lds_keyframes + 1, lds_points + 1, n_cov=600, max_obs=2))
    return out


def hand(kfs, points, current, cov, init=-1):
    """A hand-made graph over WORLD.  kfs: dicts with slot, id and optionally flags and holds (its slots: points or -1); points: dicts with
    obs = {keyframe row: keypoint index or -1} and optionally flags.  Pose of row k: (0, 0, 0, 1, k, 0, 0); position of point p: (p, 0.5, 2)."""
    so = np.cumsum([0] + [len(k.get("holds", [])) for k in kfs])
    oo = np.cumsum([0] + [len(p["obs"]) for p in points])
    return dict(kf_slot=np.array([k["slot"] for k in kfs], np.int32), kf_id=np.array([k["id"] for k in kfs], np.int64),
                kf_flags=np.array([k.get("flags", 0) for k in kfs], np.uint8),
                poses7=np.array([[0, 0, 0, 1, i, 0, 0] for i in range(len(kfs))], np.float64), slot_offsets=so.astype(np.int32),
                slot_point=np.array([s for k in kfs for s in k.get("holds", [])], np.int32), cov_kf=np.array(cov, np.int32), current=current,
                init_kf_id=init, point_flags=np.array([p.get("flags", 0) for p in points], np.uint8),
                positions=np.array([[i, 0.5, 2] for i in range(len(points))], np.float64).reshape(-1, 3), obs_offsets=oo.astype(np.int32),
                obs_kf=np.array([k for p in points for k in sorted(p["obs"])], np.int32),
                obs_index=np.array([p["obs"][k] for p in points for k in sorted(p["obs"])], np.int32))


def edge(point, pose, slot, idx, views=WORLD):
    """the edge an observation of keypoint idx of the slot's keyframe must become"""
    k, ur = views[slot]["keys"][idx], views[slot]["u_right"][idx]
    return (point, pose, float(k["x"]), float(k["y"]), float(ur) if ur >= 0 else -1.0, float(SIGMA[k["octave"]]))


def from_window(w, first_id=100):
    """The flat graph and the store contents behind a synthetic BA window (synthetic.ba_window / ba_window_varied): keyframe row k = pose k
    in slot k with one keypoint per edge of the pose; the free poses are the current keyframe (the last) and its neighbours (latest first),
    each holding the points it observes; the keyframes of win_pose carry a cloud.  -> (views, problem, inv_level_sigma2)."""
    e = w["edges"]
    K, P = len(w["poses"]), len(w["points"])
    pt, po = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    sigma = (np.float32(1.0) / np.float32((1.2 ** np.arange(N_LEVELS)) ** 2)).astype(np.float32)     # the windows' own table
    level = np.argmin(np.abs(e[:, 5][:, None] - sigma.astype(np.float64)[None, :]), 1)
    assert np.array_equal(sigma[level].astype(np.float64), e[:, 5])
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
    flags = np.zeros(K, np.uint8)
    flags[list(w.get("win_pose", []))] |= 4
    order = np.lexsort((po, pt))                                                      # point-major, rows ascending
    n_obs = np.bincount(pt, minlength=P)
    slot_offsets, slot_point = [0], []
    for k in range(K):
        row = pt[po == k] if k in free else np.zeros(0, np.int64)                     # slot i = keypoint i
        slot_point.append(row)
        slot_offsets.append(slot_offsets[-1] + len(row))
    pr = dict(kf_slot=np.arange(K, dtype=np.int32), kf_id=np.arange(K, dtype=np.int64) + first_id, kf_flags=flags, poses7=np.asarray(w["poses"], np.float64),
              slot_offsets=np.array(slot_offsets, np.int32), slot_point=np.concatenate(slot_point).astype(np.int32),
              cov_kf=free[:-1][::-1].astype(np.int32), current=int(free[-1]), init_kf_id=-1, point_flags=np.zeros(P, np.uint8),
              positions=np.asarray(w["points"], np.float64), obs_offsets=np.r_[0, np.cumsum(n_obs)].astype(np.int32), obs_kf=po[order].astype(np.int32),
              obs_index=idx[order].astype(np.int32))
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

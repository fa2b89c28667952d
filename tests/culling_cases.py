"""Problems for the culling tests: a generator of covisibility graphs on which culls cascade, a builder for hand-made graphs of a few
keyframes, and the comparison (everything is an integer: equality)."""
import numpy as np

import culling_ref as ref

OUTPUTS = ("verdict", "n_mps", "n_redundant", "n_visited", "point_bad_after", "point_nobs_after")
TH_DEPTH = 40.0


def make_problem(seed, K=40, P=3000, run=(5, 9), inertial=False, abort_ba=False, sparse=False, special=True):
    """K keyframes in a chain, the newest is the current one; P points, each observed by a run of consecutive keyframes whose length is
    uniform in `run` (sparse: 2 or 3, which makes no keyframe redundant), octave = base +- 1, 85 % stereo observations with depth in
    [2, 60] m against th_depth 40, the rest mono with depth -1; every keyframe also has some NULL slots.  local = a permutation of the
    other keyframes.  special: keyframe 0 is the map's init keyframe, one keyframe is bad already and one has mbNotErase."""
    rng = np.random.default_rng(seed)
    lo, hi = (2, 3) if sparse else run
    slots = [[] for _ in range(K)]
    obs_offsets, obs_kf, obs_octave, obs_weight, nobs = [0], [], [], [], []
    for p in range(P):
        n = int(min(K, rng.integers(lo, hi + 1)))
        first = int(rng.integers(0, K - n + 1))
        base = int(rng.integers(1, 7))
        total = 0
        for kf in range(first, first + n):
            octave = base + int(rng.integers(-1, 2))
            stereo = rng.random() < 0.85
            slots[kf].append((p, float(rng.uniform(2.0, 60.0)) if stereo else -1.0, octave))
            obs_kf.append(kf); obs_octave.append(octave); obs_weight.append(2 if stereo else 1)
            total += 2 if stereo else 1
        obs_offsets.append(len(obs_kf))
        nobs.append(total)
    slot_offsets, slot_point, slot_depth, slot_octave = [0], [], [], []
    for kf in range(K):
        rows = slots[kf] + [(-1, -1.0, 0)] * int(rng.integers(0, 1 + len(slots[kf]) // 8))
        for j in rng.permutation(len(rows)):
            slot_point.append(rows[j][0]); slot_depth.append(rows[j][1]); slot_octave.append(rows[j][2])
        slot_offsets.append(len(slot_point))
    flags = np.zeros(K, np.uint8)
    if special:
        flags[0] |= 2
        if K > 8:
            flags[int(rng.integers(1, K - 1))] |= 1
            flags[int(rng.integers(1, K - 1))] |= 4
    kf_id = 7 + 2 * np.arange(K, dtype=np.int64)
    # steps between consecutive keyframes: many short in time and space, so that the inertial gates open in every way
    dt = rng.choice([0.1, 0.2, 0.4, 1.2, 2.5], K)
    step = rng.normal(size=(K, 3))
    step *= (np.where(rng.random(K) < 0.5, rng.uniform(0.001, 0.004, K), rng.uniform(0.1, 0.5, K)) / np.linalg.norm(step, axis=1))[:, None]
    pr = dict(kf_flags=flags, kf_id=kf_id, kf_prev=np.arange(K, dtype=np.int32) - 1, kf_next=np.r_[np.arange(1, K), -1].astype(np.int32),
              kf_time=100.0 + np.cumsum(dt), kf_imu_pos=np.cumsum(step, 0).astype(np.float32), kf_th_depth=np.full(K, TH_DEPTH, np.float32),
              slot_offsets=np.array(slot_offsets, np.int32), slot_point=np.array(slot_point, np.int32), slot_depth=np.array(slot_depth, np.float32),
              slot_octave=np.array(slot_octave, np.int8), local=rng.permutation(K - 1).astype(np.int32),
              point_bad=(rng.random(P) < 0.01).astype(np.uint8), point_nobs=np.array(nobs, np.int32), obs_offsets=np.array(obs_offsets, np.int32),
              obs_kf=np.array(obs_kf, np.int32), obs_octave=np.array(obs_octave, np.int8), obs_weight=np.array(obs_weight, np.uint8),
              inertial=int(inertial), imu_initialized=int(rng.random() < 0.7), inertial_ba2=int(rng.random() < 0.3), abort_ba=int(abort_ba),
              keyframes_in_map=K + int(rng.integers(0, 3)), current_id=int(kf_id[K - 1]), last_id=int(kf_id[max(0, K - 1 - ref.ND)]))
    return pr


def family():
    """The generated problems of test_culling.py: non-inertial and inertial, K from 5 to 130 (count > 100 is reached), with and without
    abort_ba, three run lengths."""
    out = []
    for i, (K, inertial, abort_ba, run) in enumerate([
            (5, False, False, (5, 9)), (12, False, False, (5, 9)), (24, False, True, (6, 10)), (40, False, False, (5, 9)),
            (40, False, False, (6, 10)), (40, False, False, (7, 12)), (40, False, True, (5, 9)), (64, False, False, (6, 10)),
            (101, False, False, (5, 9)), (110, False, False, (6, 10)), (130, False, False, (5, 9)), (130, False, True, (7, 12)),
            (5, True, False, (5, 9)), (22, True, False, (5, 9)), (23, True, False, (6, 10)), (30, True, True, (6, 10)),
            (40, True, False, (5, 9)), (40, True, False, (6, 10)), (40, True, False, (7, 12)), (40, True, True, (7, 12)),
            (64, True, False, (7, 12)), (102, True, False, (6, 10)), (120, True, False, (7, 12)), (130, True, True, (6, 10)),
            (40, False, False, (5, 9)), (40, True, False, (7, 12))]):
        out.append(make_problem(50 + i, K, 75 * K, run, inertial, abort_ba))
    out.append(make_problem(90, 40, 3000, sparse=True))
    return out


def hand(kfs, points, local, **scalars):
    """A hand-made graph.  kfs: dicts with slots = [(point, depth, octave)] and optionally flags, id, prev, next, time, pos, th_depth;
    points: dicts with obs = [(keyframe, octave, weight)] and optionally bad, nobs (default: the sum of the weights)."""
    K = len(kfs)
    so, oo = np.cumsum([0] + [len(k.get("slots", [])) for k in kfs]), np.cumsum([0] + [len(p.get("obs", [])) for p in points])
    sl = [s for k in kfs for s in k.get("slots", [])]
    ob = [o for p in points for o in p.get("obs", [])]
    col = lambda rows, j, t: np.array([r[j] for r in rows], t)
    pr = dict(kf_flags=np.array([k.get("flags", 0) for k in kfs], np.uint8), kf_id=np.array([k.get("id", 10 + i) for i, k in enumerate(kfs)], np.int64),
              kf_prev=np.array([k.get("prev", -1) for k in kfs], np.int32), kf_next=np.array([k.get("next", -1) for k in kfs], np.int32),
              kf_time=np.array([k.get("time", float(i)) for i, k in enumerate(kfs)], np.float64),
              kf_imu_pos=np.array([k.get("pos", (float(i), 0.0, 0.0)) for i, k in enumerate(kfs)], np.float32).reshape(K, 3),
              kf_th_depth=np.array([k.get("th_depth", TH_DEPTH) for k in kfs], np.float32), slot_offsets=so.astype(np.int32),
              slot_point=col(sl, 0, np.int32), slot_depth=col(sl, 1, np.float32), slot_octave=col(sl, 2, np.int8), local=np.array(local, np.int32),
              point_bad=np.array([p.get("bad", 0) for p in points], np.uint8),
              point_nobs=np.array([p.get("nobs", sum(o[2] for o in p.get("obs", []))) for p in points], np.int32), obs_offsets=oo.astype(np.int32),
              obs_kf=col(ob, 0, np.int32), obs_octave=col(ob, 1, np.int8), obs_weight=col(ob, 2, np.uint8),
              inertial=0, imu_initialized=0, inertial_ba2=0, abort_ba=0, keyframes_in_map=K, current_id=1000, last_id=0)
    pr.update(scalars)
    return pr


def star(n_slots, n_redundant, n_kf=6, depth=10.0, octave=2, **kf0):
    """Keyframe 0 holds n_slots points: the first n_redundant are also seen (stereo, same octave) by keyframes 1-4, the others by keyframes
    1 and 2 only.  Keyframes 1.. hold the points they observe.  -> (kfs, points)"""
    kfs = [dict(kf0, slots=[])] + [dict(slots=[]) for _ in range(n_kf - 1)]
    points = []
    for p in range(n_slots):
        seen = [0, 1, 2, 3, 4] if p < n_redundant else [0, 1, 2]
        points.append(dict(obs=[(k, octave, 2) for k in seen]))
        for k in seen:
            kfs[k]["slots"].append((p, depth, octave))
    return kfs, points


def chain(kfs, dt=0.1):
    """links the keyframes in index order and spaces them dt apart"""
    for i, k in enumerate(kfs):
        k.setdefault("prev", i - 1)
        k.setdefault("next", i + 1 if i + 1 < len(kfs) else -1)
        k.setdefault("time", dt * i)
    return kfs


def assert_equal(got, want, what=""):
    for k in OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])


def random_points(seed, n):
    """Inputs of MapPointCulling that reach every rule, zero denominators and ids beyond 32 bits included."""
    rng = np.random.default_rng(seed)
    first = rng.integers(0, 5000, n).astype(np.int64) + rng.choice([0, 1 << 32, 1 << 40], n, p=[0.9, 0.05, 0.05])
    return dict(bad=(rng.random(n) < 0.1).astype(np.uint8), n_found=rng.integers(0, 40, n).astype(np.int32),
                n_visible=rng.integers(0, 60, n).astype(np.int32), first_kf_id=first,
                n_obs=rng.integers(0, 8, n).astype(np.int32), current_kf_id=first + rng.integers(0, 5, n) + rng.choice([0, 1 << 32], n, p=[0.97, 0.03]))

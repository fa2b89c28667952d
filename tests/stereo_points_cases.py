"""Frames and decisions for the stereo-point / new-keyframe tests: hand-made ones that meet one rule each, a seeded family, and the
comparison.  Every output is an integer or a float compared by its bits."""
import functools

import numpy as np

import stereo_points_ref as ref

UNPROJECT4 = np.array([601.8873, 183.1104, 1.0 / 707.0912, 1.0 / 707.0912], np.float32)     # cx, cy, invfx, invfy
TH_DEPTH = 40.0
POINT_OUTPUTS = ("created_keypoint", "x3D", "n_created", "n_visited", "n_with_depth")
DECISION_OUTPUTS = ("need", "interrupt_ba", "conditions", "exit_rule", "n_tracked_close", "n_non_tracked_close", "n_ref_matches")
SIZES = (63, 64, 65, 257, 1000, 2000, 4096)


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]], np.float32)


def frame(depth, held=None, outlier=None, seed=0, th_depth=TH_DEPTH, max_point=100, mode=ref.CLOSEST):
    """A frame around the given depths: keypoints anywhere in a 1241 x 376 image, a random pose; held / outlier default to 0."""
    rng = np.random.default_rng(1000 + seed)
    depth = np.asarray(depth, np.float32).reshape(-1)
    n = len(depth)
    keys = np.stack([rng.uniform(0, 1241, n), rng.uniform(0, 376, n)], 1).astype(np.float32).reshape(n, 2)
    return dict(depth=depth, keys=keys, held=np.zeros(n, np.uint8) if held is None else np.asarray(held, np.uint8),
                outlier=np.zeros(n, np.uint8) if outlier is None else np.asarray(outlier, np.uint8), Rwc=rotation(rng),
                Ow=rng.normal(0, 30, 3).astype(np.float32), th_depth=np.float32(th_depth), max_point=max_point, mode=mode)


def depths(n_close, n_far, n_none=0, seed=0, th_depth=TH_DEPTH):
    """n_close depths in [1, th_depth), n_far in (th_depth, 150], n_none without depth (-1), shuffled"""
    rng = np.random.default_rng(2000 + seed)
    d = np.r_[rng.uniform(1.0, th_depth - 0.5, n_close), rng.uniform(th_depth + 0.5, 150.0, n_far), np.full(n_none, -1.0)].astype(np.float32)
    return d[rng.permutation(len(d))]


@functools.lru_cache(maxsize=None)
def hand_frames():
    """[(name, frame)]: one per rule of the creation"""
    rng = np.random.default_rng(7)
    out = [("n = 0", frame([])), ("n = 1", frame([5.0])), ("n = 1 without depth", frame([-1.0])),
           ("no positive depth", frame(np.r_[np.zeros(30), -rng.uniform(0, 9, 30), np.full(10, np.nan)])),
           ("M < max_point: all taken", frame(depths(30, 30, 20, 1), seed=1)),
           ("M = 101 exactly", frame(depths(40, 61, 9, 2), seed=2)),
           ("M > 101, c < 100: 101 taken", frame(depths(50, 200, 50, 3), seed=3)),
           ("c = 99: 101 taken", frame(depths(99, 100, 10, 4), seed=4)),
           ("c = 100: 101 taken", frame(depths(100, 100, 10, 5), seed=5)),
           ("c = 101: 102 taken", frame(depths(101, 100, 10, 6), seed=6)),
           ("c = 150: 151 taken", frame(depths(150, 100, 10, 7), seed=7)),
           ("c = M: all close", frame(depths(180, 0, 20, 8), seed=8)),
           ("c = M = 100", frame(depths(100, 0, 3, 9), seed=9)),
           ("max_point = 0, no close point: one taken", frame(depths(0, 50, 5, 10), seed=10, max_point=0)),
           ("max_point = 0, ten close points: eleven taken", frame(depths(10, 50, 5, 11), seed=11, max_point=0)),
           ("max_point = 101", frame(depths(20, 200, 5, 12), seed=12, max_point=101)),
           ("max_point = 102", frame(depths(20, 200, 5, 13), seed=13, max_point=102))]
    # depth exactly th_depth is close for the walk (> at :3199): 120 + 5 close ones and one far one are taken
    d = depths(120, 60, 10, 14)
    d[np.flatnonzero(d > TH_DEPTH)[:5]] = TH_DEPTH
    out.append(("depth == th_depth", frame(d, seed=14)))
    # five bit-equal depths around the end of the walk: entries 99..103 of the sorted list, of which 99 and 100 are taken, by index
    d = depths(99, 60, 10, 15)
    far = np.flatnonzero(d > TH_DEPTH)
    d[far[rng.permutation(len(far))[:5]]] = np.float32(TH_DEPTH + 0.25)
    out.append(("five equal depths", frame(d, seed=15)))
    d = depths(30, 30, 0, 16)
    d[::6] = [np.inf, np.nan, 0.0, -0.0, -3.0, -np.inf, np.inf, np.nan, 0.0, -1.0]
    out.append(("+inf, NaN, 0 and negative depths", frame(d, seed=16)))
    out.append(("all held with observations", frame(depths(60, 80, 10, 17), held=np.ones(150), seed=17)))
    out.append(("held without observations is created", frame(depths(60, 80, 10, 18), held=rng.choice([1, 2], 150), seed=18)))
    out.append(("ALL, n = 500: nothing", frame(depths(200, 200, 100, 19), held=rng.integers(0, 3, 500), seed=19, mode=ref.ALL)))
    out.append(("ALL, n = 501", frame(depths(200, 200, 101, 20), held=rng.integers(0, 3, 501), seed=20, mode=ref.ALL)))
    out.append(("ALL, n = 4096", frame(depths(2000, 1000, 1096, 21), seed=21, mode=ref.ALL)))
    out.append(("n = 4096, all with depth", frame(depths(3000, 1096, 0, 22), held=rng.integers(0, 3, 4096), seed=22)))
    return out


def decision(**kw):
    """Defaults on which only c2 holds: the answer is no by the conditions (:3049)."""
    d = dict(inertial=0, imu_initialized=1, only_tracking=0, mapper_stopped=0, mapper_idle=1, mapper_initializing=0, keyframes_in_queue=0,
             create_blocked=0, has_last_kf=1, frame_id=100, last_reloc_frame_id=0, last_keyframe_id=90, max_frames=30, min_frames=20, n_kfs=5,
             matches_inliers=50, n_ref_matches=100, time_frame=10.0, time_last_kf=9.875)
    d.update(kw)
    return d


def count_frame(n_tracked, n_non_tracked, seed=0):
    """A frame whose close counts (:2982-2998) are the given ones: outliers and keypoints without a point are not tracked; far points, points
    at th_depth exactly and points without depth count nowhere."""
    rng = np.random.default_rng(3000 + seed)
    half = n_non_tracked // 2
    d = np.r_[rng.uniform(1, TH_DEPTH - 1, n_tracked + n_non_tracked), np.full(7, TH_DEPTH), rng.uniform(TH_DEPTH + 1, 90, 40), np.full(9, -1.0)]
    held = np.r_[rng.choice([1, 2], n_tracked), np.zeros(half), rng.choice([1, 2], n_non_tracked - half), rng.integers(0, 3, 56)]
    outlier = np.r_[np.zeros(n_tracked), rng.integers(0, 2, half), np.ones(n_non_tracked - half), rng.integers(0, 2, 56)]
    p = rng.permutation(len(d))
    return frame(d[p], held[p], outlier[p], seed=100 + seed)


NOBS = np.array([-1, 0, 1, 2, 2, 3, 3, 3, 4, 9, -1, 1], np.int32)     # TrackedMapPoints(2) = 7, TrackedMapPoints(3) = 5, of 10 live points


@functools.lru_cache(maxsize=None)
def hand_decisions():
    """[(name, frame, decision, (need, exit_rule, conditions) or None)]: each early exit, each condition alone on both sides of its
    threshold.  The expectation is written by hand where the name states it."""
    R = ref
    f = count_frame(120, 30)
    T = lambda need, rule, cond: (need, rule, cond)
    out = [
        ("defaults: only c2", f, decision(), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("IMU not initialised, 0.25 s", f, decision(inertial=1, imu_initialized=0, time_frame=10.25, time_last_kf=10.0), T(1, R.EXIT_IMU_NOT_INITIALIZED, 0)),
        ("IMU not initialised, below 0.25 s", f, decision(inertial=1, imu_initialized=0, time_frame=10.2, time_last_kf=10.0), T(0, R.EXIT_IMU_NOT_INITIALIZED, 0)),
        ("IMU not initialised comes before only_tracking", f, decision(inertial=1, imu_initialized=0, only_tracking=1, time_frame=11.0), T(1, R.EXIT_IMU_NOT_INITIALIZED, 0)),
        ("only_tracking", f, decision(only_tracking=1, mapper_stopped=1, frame_id=200), T(0, R.EXIT_ONLY_TRACKING, 0)),
        ("mapper_stopped", f, decision(mapper_stopped=1, frame_id=200), T(0, R.EXIT_MAPPER_STOPPED, 0)),
        ("after relocalisation", f, decision(frame_id=129, last_reloc_frame_id=100, n_kfs=31), T(0, R.EXIT_AFTER_RELOC, 0)),
        ("after relocalisation, frame at the bound", f, decision(frame_id=130, last_reloc_frame_id=100, last_keyframe_id=125, n_kfs=31), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("after relocalisation, n_kfs == max_frames", f, decision(frame_id=129, last_reloc_frame_id=100, last_keyframe_id=125, n_kfs=30), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c1a on", f, decision(frame_id=120, mapper_idle=0), T(1, R.EXIT_MAPPER_BUSY, R.C1A | R.C2)),
        ("c1a off", f, decision(frame_id=119, mapper_idle=0), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c1b on", f, decision(frame_id=110), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1B | R.C2)),
        ("c1b off by a frame", f, decision(frame_id=109), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c1b off by the mapper", f, decision(frame_id=110, mapper_idle=0), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c1c on: 24 < 100 * 0.25", f, decision(matches_inliers=24), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1C | R.C2)),
        ("c1c off: 25 == 100 * 0.25", f, decision(matches_inliers=25), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c1c off: inertial", f, decision(matches_inliers=24, inertial=1, time_frame=10.0, time_last_kf=9.875), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("close: 99 tracked, 71 not", count_frame(99, 71, 1), decision(matches_inliers=90), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1C | R.C2)),
        ("not close: 100 tracked", count_frame(100, 71, 2), decision(matches_inliers=90), T(0, R.EXIT_CONDITIONS, 0)),
        ("not close: 70 not tracked", count_frame(99, 70, 3), decision(matches_inliers=90), T(0, R.EXIT_CONDITIONS, 0)),
        ("c2 on: 74 < 75", f, decision(matches_inliers=74), T(0, R.EXIT_CONDITIONS, R.C2)),
        ("c2 off: 75 == 100 * 0.75f", f, decision(matches_inliers=75), T(0, R.EXIT_CONDITIONS, 0)),
        ("c2 off: 15 inliers", f, decision(matches_inliers=15, frame_id=120), T(0, R.EXIT_CONDITIONS, R.C1A | R.C1B | R.C1C)),
        ("c2 on: 16 inliers", f, decision(matches_inliers=16, frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C1C | R.C2)),
        # (float)11184811 * 0.75f = 8388608 in float, 8388608.25 in double: 8388608 inliers are not below it
        ("c2 off in float, on in double", f, decision(matches_inliers=8388608, n_ref_matches=11184811, frame_id=120), T(0, R.EXIT_CONDITIONS, R.C1A | R.C1B)),
        ("c2 on one inlier less", f, decision(matches_inliers=8388607, n_ref_matches=11184811, frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        # n_kfs = 1: 50 * 0.4f = 20.0000003 in double, 20 in float
        ("n_kfs = 1: 0.4f, off in float", f, decision(n_kfs=1, matches_inliers=20, n_ref_matches=50, frame_id=120), T(0, R.EXIT_CONDITIONS, R.C1A | R.C1B)),
        ("n_kfs = 1: 0.4f, on", f, decision(n_kfs=1, matches_inliers=19, n_ref_matches=50, frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("n_kfs = 2: 0.75f", f, decision(n_kfs=2, matches_inliers=30, n_ref_matches=50, frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("c3 on: 0.5 s", f, decision(inertial=1, time_frame=10.5, time_last_kf=10.0, matches_inliers=90), T(1, R.EXIT_MAPPER_ACCEPTS, R.C3)),
        ("c3 off: below 0.5 s", f, decision(inertial=1, time_frame=10.4375, time_last_kf=10.0, matches_inliers=90), T(0, R.EXIT_CONDITIONS, 0)),
        ("c3 off: no last keyframe", f, decision(inertial=1, has_last_kf=0, time_frame=11.0, time_last_kf=10.0, matches_inliers=90), T(0, R.EXIT_CONDITIONS, 0)),
        ("c3 off: not inertial", f, decision(time_frame=11.0, time_last_kf=10.0, matches_inliers=90), T(0, R.EXIT_CONDITIONS, 0)),
        # unsigned: 5 - 10 is not a small negative difference, 5 >= 40 is simply false
        ("unsigned: frame_id below last_keyframe_id", f, decision(frame_id=5, last_keyframe_id=10, min_frames=0), T(0, R.EXIT_CONDITIONS, R.C2)),
        # unsigned int sum: (2^32 - 10) + 30 wraps to 20 (Tracking.h:335), and the unsigned long frame_id 25 is not below it
        ("unsigned: the 32-bit sum wraps", f, decision(frame_id=25, last_keyframe_id=(1 << 32) - 10, mapper_idle=0), T(1, R.EXIT_MAPPER_BUSY, R.C1A | R.C2)),
        ("unsigned: frame_id above 2^32", f, decision(frame_id=(1 << 32) + 5, last_keyframe_id=(1 << 32) - 10, last_reloc_frame_id=(1 << 32) - 40, n_kfs=31), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("unsigned: max_frames = -1", f, decision(frame_id=9, last_keyframe_id=10, max_frames=-1, mapper_idle=0, n_kfs=0), None),
        ("busy mapper, 2 in the queue", f, decision(frame_id=120, mapper_idle=0, keyframes_in_queue=2), T(1, R.EXIT_MAPPER_BUSY, R.C1A | R.C2)),
        ("busy mapper, 3 in the queue", f, decision(frame_id=120, mapper_idle=0, keyframes_in_queue=3), T(0, R.EXIT_MAPPER_BUSY, R.C1A | R.C2)),
        ("busy mapper that is initialising", f, decision(frame_id=120, mapper_idle=0, mapper_initializing=1, keyframes_in_queue=5), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C2)),
        ("create_blocked", f, decision(frame_id=120, create_blocked=1), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("ref_nobs, n_kfs = 1", f, decision(n_kfs=1, ref_nobs=NOBS, n_ref_matches=-5, matches_inliers=50), None),
        ("ref_nobs, n_kfs = 2", f, decision(n_kfs=2, ref_nobs=NOBS, n_ref_matches=-5, matches_inliers=50), None),
        ("ref_nobs, n_kfs = 3", f, decision(n_kfs=3, ref_nobs=NOBS, n_ref_matches=-5, matches_inliers=50), None),
        ("ref_nobs empty", f, decision(ref_nobs=np.zeros(0, np.int32), n_ref_matches=99, frame_id=120), None),
        ("yes on a frame without keypoints", frame([]), decision(frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("yes on a frame without depth", frame(-np.ones(70)), decision(frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C2)),
        ("yes, depth == th_depth", dict(hand_frames())["depth == th_depth"], decision(frame_id=120), T(1, R.EXIT_MAPPER_ACCEPTS, R.C1A | R.C1B | R.C1C | R.C2)),
    ]
    return out


@functools.lru_cache(maxsize=None)
def family(n_frames=70):
    """-> (frames, decisions): n from SIZES in turn; depths a mix of close and far with about 5 % copied from another keypoint (ties) and
    some missing; random held, outlier, poses; decisions that answer both ways through every rule."""
    frames, decisions = [], []
    for k in range(n_frames):
        rng = np.random.default_rng(400 + k)
        n = SIZES[k % len(SIZES)]
        close = rng.random(n) < rng.choice([0.02, 0.1, 0.5, 0.9])
        d = np.where(close, rng.uniform(0.5, TH_DEPTH, n), rng.uniform(TH_DEPTH, 300.0, n)).astype(np.float32)
        dup = rng.random(n) < 0.05
        d[dup] = d[rng.integers(0, n, int(dup.sum()))]
        d[rng.random(n) < rng.choice([0.0, 0.3, 0.6])] = rng.choice([-1.0, 0.0])
        frames.append(frame(d, rng.choice([0, 1, 2], n, p=[0.5, 0.4, 0.1]), rng.random(n) < 0.1, seed=500 + k))
        frame_id = int(rng.integers(0, 300))
        dec = decision(inertial=int(rng.random() < 0.3), imu_initialized=int(rng.random() < 0.8), only_tracking=int(rng.random() < 0.05),
                       mapper_stopped=int(rng.random() < 0.05), mapper_idle=int(rng.random() < 0.6), mapper_initializing=int(rng.random() < 0.1),
                       keyframes_in_queue=int(rng.integers(0, 6)), create_blocked=int(rng.random() < 0.1), frame_id=frame_id,
                       last_reloc_frame_id=int(rng.integers(0, 100)), last_keyframe_id=int(rng.integers(0, frame_id + 1)),
                       min_frames=int(rng.choice([0, 10])), n_kfs=int(rng.integers(1, 45)), matches_inliers=int(rng.integers(0, 200)),
                       n_ref_matches=int(rng.integers(0, 300)), time_frame=20.0 + 0.05 * frame_id, time_last_kf=20.0 + 0.05 * frame_id - float(rng.uniform(0.0, 0.8)))
        if k % 2:
            dec["ref_nobs"] = rng.integers(-1, 8, int(rng.integers(1, 2500))).astype(np.int32)
        decisions.append(dec)
    return frames, decisions


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same(a, b):
    """Equality of integers; of floats by their bits (the infinities and NaNs that a keypoint with infinite depth un-projects to included)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def assert_equal(got, want, what="", keys=POINT_OUTPUTS):
    for k in keys:
        assert same(got[k], want[k]), (what, k, got[k], want[k])

"""Tracking::NeedNewKeyFrame and the stereo map-point creation of CreateNewKeyFrame, UpdateLastFrame and StereoInitialization restated in
Python from the reference's source, the checker of tests/test_stereo_points.py and tests/test_stereo_points_gpu.py.  Line numbers are
SF/src/Tracking.cc unless a file is named.  A frame is the dict that tc2li_stereo_points_frame describes (include/tc2li_hip.h "tracking:
stereo map points and the keyframe decision"): depth, keys [n, 2] (x, y of mvKeysUn), held, outlier, Rwc [3, 3], Ow, th_depth, max_point,
mode; a decision the dict of tc2li_keyframe_decision's scalars and optionally ref_nobs.

The loops are the reference's: a list of (depth, index) tuples, sorted(), a walk with the exit test after the entry.  No closed form.  All
float arithmetic is on np.float32 scalars, one rounding per operation, in the order the header states."""
import numpy as np

CLOSEST, ALL = 0, 1
C1A, C1B, C1C, C2, C3 = 1, 2, 4, 8, 16
EXIT_IMU_NOT_INITIALIZED, EXIT_ONLY_TRACKING, EXIT_MAPPER_STOPPED, EXIT_AFTER_RELOC, EXIT_CONDITIONS, EXIT_MAPPER_ACCEPTS, EXIT_MAPPER_BUSY = range(1, 8)
F = np.float32
M32 = (1 << 32) - 1


def unproject_stereo(u, v, z, unproject4, R, Ow):
    """Frame::UnprojectStereo (SF/src/Frame.cc:1037-1050) -> [3] float32"""
    cx, cy, invfx, invfy = (F(t) for t in unproject4)
    with np.errstate(all="ignore"):                                                  # an infinite depth gives inf and NaN, as in C++
        x = ((F(u) - cx) * z) * invfx
        y = ((F(v) - cy) * z) * invfy
        return np.array([((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + Ow[r] for r in range(3)], F)


def stereo_points(f, unproject4, create=True):
    """-> dict(created_keypoint [n_created], x3D [n_created, 3], n_created, n_visited, n_with_depth) and, for the tests' own bookkeeping,
    ended_by_break (the exit test of :3199 fired) and ties (two visited neighbours with bit-equal depth)."""
    depth = np.asarray(f["depth"], F).reshape(-1)
    n = len(depth)
    xy = np.asarray(f["keys"], F).reshape(n, 2)
    held = np.asarray(f["held"], np.uint8)
    R, Ow = np.asarray(f["Rwc"], F).reshape(3, 3), np.asarray(f["Ow"], F).reshape(3)
    th_depth, max_point, mode = F(f["th_depth"]), int(f.get("max_point", 100)), int(f.get("mode", CLOSEST))
    created, x3d = [], []

    def make(i):
        created.append(i)
        x3d.append(unproject_stereo(xy[i, 0], xy[i, 1], depth[i], unproject4, R, Ow))

    n_with_depth = sum(1 for i in range(n) if depth[i] > 0)
    n_points, ended_by_break, ties = 0, False, 0
    if not create:
        pass
    elif mode == ALL:
        if n > 500:                                                                  # :2433
            for i in range(n):                                                       # :2479-2495
                if depth[i] > 0:
                    make(i)
        n_points = len(created)
    else:
        depth_idx = [(depth[i], i) for i in range(n) if depth[i] > 0]                # :3132-3142, :2676-2686
        depth_idx = sorted(depth_idx)                                                # :3146, :2691
        for j, (z, i) in enumerate(depth_idx):
            ties += j > 0 and depth_idx[j - 1][0] == z
            if held[i] != 1:                                                         # :3156-3162, :2704-2707: NULL, or Observations() < 1
                make(i)
            n_points += 1                                                            # :3192, :3196
            if z > th_depth and n_points > max_point:                                # :3199, :2731
                ended_by_break = True
                break
    return dict(created_keypoint=np.array(created, np.int32), x3D=np.array(x3d, F).reshape(len(created), 3), n_created=len(created),
                n_visited=n_points, n_with_depth=n_with_depth, ended_by_break=ended_by_break, ties=int(ties))


def tracked_map_points(ref_nobs, min_obs):
    """KeyFrame::TrackedMapPoints (SF/src/KeyFrame.cc:352-377) on Observations() per slot, -1 = NULL or bad"""
    n = 0
    for v in ref_nobs:
        if v >= 0 and (min_obs <= 0 or v >= min_obs):
            n += 1
    return n


def need_new_keyframe(f, d):
    """-> dict(need, interrupt_ba, conditions, exit_rule, n_tracked_close, n_non_tracked_close, n_ref_matches)"""
    depth = np.asarray(f["depth"], F).reshape(-1)
    held, outlier = np.asarray(f["held"], np.uint8), np.asarray(f["outlier"], np.uint8)
    th_depth = F(f["th_depth"])
    g = lambda k: int(d.get(k, 0))
    n_tracked = n_non_tracked = 0
    for i in range(len(depth)):                                                      # :2988-2998
        if depth[i] > 0 and depth[i] < th_depth:
            if held[i] != 0 and not outlier[i]:
                n_tracked += 1
            else:
                n_non_tracked += 1
    n_kfs, inl = g("n_kfs"), g("matches_inliers")
    ref = g("n_ref_matches")
    if d.get("ref_nobs") is not None:
        ref = tracked_map_points(d["ref_nobs"], 2 if n_kfs <= 2 else 3)              # :2973-2976
    out = dict(need=0, interrupt_ba=0, conditions=0, exit_rule=0, n_tracked_close=n_tracked, n_non_tracked_close=n_non_tracked, n_ref_matches=ref)
    inertial, idle = bool(g("inertial")), bool(g("mapper_idle"))
    dt = float(d.get("time_frame", 0.0)) - float(d.get("time_last_kf", 0.0))
    # mnLastRelocFrameId, mnLastKeyFrameId are unsigned int, mMaxFrames, mMinFrames int (SF/include/Tracking.h:316-336): the sums are
    # unsigned 32-bit; mnId is unsigned long
    plus = lambda a, b: (g(a) + g(b)) & M32
    if inertial and not g("imu_initialized"):                                        # :2944-2950
        out.update(exit_rule=EXIT_IMU_NOT_INITIALIZED, need=int(dt >= 0.25))
        return out
    if g("only_tracking"):                                                           # :2952
        out.update(exit_rule=EXIT_ONLY_TRACKING)
        return out
    if g("mapper_stopped"):                                                          # :2956
        out.update(exit_rule=EXIT_MAPPER_STOPPED)
        return out
    if g("frame_id") < plus("last_reloc_frame_id", "max_frames") and n_kfs > g("max_frames"):   # :2967
        out.update(exit_rule=EXIT_AFTER_RELOC)
        return out
    close = n_tracked < 100 and n_non_tracked > 70                                   # :3003
    th_ref_ratio = F(0.4) if n_kfs < 2 else F(0.75)                                  # :3006-3008
    c1a = g("frame_id") >= plus("last_keyframe_id", "max_frames")                    # :3023
    c1b = g("frame_id") >= plus("last_keyframe_id", "min_frames") and idle           # :3025
    c1c = (not inertial) and (float(inl) < float(ref) * 0.25 or close)               # :3027: int * double
    c2 = (bool(F(inl) < F(ref) * th_ref_ratio) or close) and inl > 15                # :3029: int * float
    c3 = bool(g("has_last_kf")) and inertial and dt >= 0.5                           # :3033-3041
    out["conditions"] = C1A * c1a + C1B * c1b + C1C * c1c + C2 * c2 + C3 * c3
    if not (((c1a or c1b or c1c) and c2) or c3):                                     # :3049, c4 is false (:3044)
        out.update(exit_rule=EXIT_CONDITIONS)
    elif idle or g("mapper_initializing"):                                           # :3053
        out.update(exit_rule=EXIT_MAPPER_ACCEPTS, need=1)
    else:                                                                            # :3059-3065
        out.update(exit_rule=EXIT_MAPPER_BUSY, interrupt_ba=1, need=int(g("keyframes_in_queue") < 3))
    return out


def new_keyframe(f, d, unproject4):
    """NeedNewKeyFrame, then CreateNewKeyFrame's points where it says yes and the gates of :3080-3084 are open."""
    out = need_new_keyframe(f, d)
    out.update(stereo_points(dict(f, mode=CLOSEST), unproject4, create=bool(out["need"]) and not int(d.get("create_blocked", 0))))
    return out

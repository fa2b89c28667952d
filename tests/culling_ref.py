"""LocalMapping::KeyFrameCulling and LocalMapping::MapPointCulling restated in Python from the reference's source, the checker of
tests/test_culling.py and tests/test_culling_gpu.py.  Line numbers are SF/src/LocalMapping.cc unless a file is named.  A problem is the
dict of arrays that tc2li_culling_problem describes (include/tc2li_hip.h "local mapping: culling").

The restatement keeps the objects' behaviour, not their layout: a point's observations are a dict keyframe -> (octave, weight) as
MapPoint::mObservations is a map, a keyframe's slots a list as mvpMapPoints is a vector.

effects=False decides every keyframe on the state the call started with (no erasure, no relink, no keyframe turns bad, KeyFramesInMap stays).
It exists only so that tests can show that the order dependence is exercised."""
import numpy as np

SKIPPED, NOT_VISITED = -1, -2
REDUNDANT, SET_BAD, MERGED, DEFERRED = 1, 2, 4, 8
ND = 21                                   # :919
M64 = (1 << 64) - 1
F = np.float32


def keyframe_culling(pr, effects=True):
    """-> dict(verdict, n_mps, n_redundant [n_local], n_visited, point_bad_after, point_nobs_after [n_points]) and, for the tests' own
    bookkeeping, dirty [n_local] (a decided keyframe one of whose points had lost an observation to an earlier cull), norms (every
    |imu_pos - imu_pos[prev]| that :1044 evaluated) and culled (erasures that went through)."""
    n_kf, n_pt = len(pr["kf_flags"]), len(pr["point_bad"])
    flags = [int(v) for v in pr["kf_flags"]]
    kf_id = [int(v) for v in pr["kf_id"]]
    prev, nxt = [int(v) for v in pr["kf_prev"]], [int(v) for v in pr["kf_next"]]
    time = [float(v) for v in pr["kf_time"]]
    pos = np.asarray(pr["kf_imu_pos"], F).reshape(n_kf, 3)
    th_depth = np.asarray(pr["kf_th_depth"], F)
    so = [int(v) for v in pr["slot_offsets"]]
    slot_point, slot_octave = [int(v) for v in pr["slot_point"]], [int(v) for v in pr["slot_octave"]]
    slot_depth = np.asarray(pr["slot_depth"], F)
    oo = [int(v) for v in pr["obs_offsets"]]
    bad = [bool(v) for v in pr["point_bad"]]
    nobs = [int(v) for v in pr["point_nobs"]]
    # mObservations per point.  A bad point has none (SF/src/MapPoint.cc:233).  A keyframe listed twice in a row (no map can hold that)
    # keeps every entry: all of them go when the keyframe is erased.
    obs = []
    for p in range(n_pt):
        row = {}
        if not bad[p]:
            for o in range(oo[p], oo[p + 1]):
                row.setdefault(int(pr["obs_kf"][o]), []).append((int(pr["obs_octave"][o]), int(pr["obs_weight"][o])))
        obs.append(row)
    inertial, imu_init, ba2, abort_ba = (bool(pr.get(k, 0)) for k in ("inertial", "imu_initialized", "inertial_ba2", "abort_ba"))
    in_map, current_id, last_id = int(pr.get("keyframes_in_map", 0)), int(pr.get("current_id", 0)), int(pr.get("last_id", 0))
    th = F(0.5) if inertial else F(0.9)                                              # :923-929, mbMonocular is false
    local = [int(v) for v in pr["local"]]
    verdict = np.full(len(local), NOT_VISITED, np.int32)
    n_mps_out, n_red_out = np.zeros(len(local), np.int32), np.zeros(len(local), np.int32)
    dirty = np.zeros(len(local), bool)
    kf_bad = [bool(f & 1) for f in flags]
    changed = [False] * n_pt
    norms, culled = [], 0
    count = 0
    for i, kf in enumerate(local):
        count += 1                                                                   # :952
        if (flags[kf] & 2) or kf_bad[kf]:                                            # :955
            verdict[i] = SKIPPED
            continue
        n_mps = n_red = 0
        for s in range(so[kf], so[kf + 1]):                                          # :963-1019
            p = slot_point[s]
            if p < 0:
                continue
            dirty[i] |= changed[p]
            if bad[p]:
                continue
            if slot_depth[s] > th_depth[kf] or slot_depth[s] < 0:                    # :972
                continue
            n_mps += 1
            if nobs[p] > 3:                                                          # :977
                n = sum(1 for k, entries in obs[p].items() if k != kf for (octave, _) in entries if octave <= slot_octave[s] + 1)
                n_red += n > 3                                                       # :1005-1015
        n_mps_out[i], n_red_out[i] = n_mps, n_red
        v, go_on = 0, False
        if F(n_red) > th * F(n_mps):                                                 # :1021
            v = REDUNDANT
            if not inertial:
                v |= SET_BAD                                                         # :1057
            elif in_map <= ND:                                                       # :1025
                go_on = True
            elif (kf_id[kf] & M64) > ((current_id - 2) & M64):                       # :1028
                go_on = True
            elif prev[kf] >= 0 and nxt[kf] >= 0:                                     # :1031
                t = F(time[nxt[kf]] - time[prev[kf]])
                merge = (imu_init and (kf_id[kf] & M64) < (last_id & M64) and float(t) < 3.0) or float(t) < 0.5   # :1035
                if not merge and not ba2 and t < F(3):                               # :1044
                    d = pos[kf] - pos[prev[kf]]
                    norm = np.sqrt(d[0] * d[0] + (d[1] * d[1] + d[2] * d[2]))
                    norms.append(float(norm))
                    merge = float(norm) < 0.02
                if merge:
                    v |= MERGED | SET_BAD
                    if effects:                                                      # :1038-1041
                        a, b = prev[kf], nxt[kf]
                        prev[b], nxt[a], nxt[kf], prev[kf] = a, b, -1, -1
        if v & SET_BAD:
            if flags[kf] & 4:                                                        # SF/src/KeyFrame.cc:593-597
                v |= DEFERRED
            elif effects:
                for s in range(so[kf], so[kf + 1]):                                  # KeyFrame.cc:605-611
                    p = slot_point[s]
                    if p < 0 or kf not in obs[p]:                                    # MapPoint.cc:182
                        continue
                    nobs[p] -= sum(w for _, w in obs[p].pop(kf))                     # :187-197
                    changed[p] = True
                    if nobs[p] <= 2:                                                 # :203-209, SetBadFlag :225-248
                        bad[p] = True
                        obs[p] = {}
                kf_bad[kf] = True
                in_map -= 1                                                          # Map::EraseKeyFrame
                culled += 1
        verdict[i] = v
        if go_on:
            continue
        if (count > 20 and abort_ba) or count > 100:                                 # :1060
            break
    return dict(verdict=verdict, n_mps=n_mps_out, n_redundant=n_red_out, n_visited=count, point_bad_after=np.array(bad, np.uint8).reshape(n_pt),
                point_nobs_after=np.array(nobs, np.int32).reshape(n_pt), dirty=dirty, norms=norms, culled=culled)


def map_point_culling(pt, th_obs=3):
    """LocalMapping::MapPointCulling (:360-399) per entry of mlpRecentAddedMapPoints -> action: 0 stays, 1 dropped because bad (:379),
    2 SetBadFlag by found ratio (:381), 3 SetBadFlag by observations (:386), 4 dropped by age (:391)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.asarray(pt["n_found"], np.int32).astype(F) / np.asarray(pt["n_visible"], np.int32).astype(F)   # MapPoint.cc:335
    # (int)nCurrentKFid - (int)mnFirstKFid: both truncated to 32 bits, then an int subtraction
    age = np.asarray(pt["current_kf_id"], np.int64).astype(np.int32) - np.asarray(pt["first_kf_id"], np.int64).astype(np.int32)
    n_obs = np.asarray(pt["n_obs"], np.int32)
    action = np.zeros(len(n_obs), np.uint8)
    free = np.ones(len(n_obs), bool)
    for code, rule in ((1, np.asarray(pt["bad"]) != 0), (2, ratio < F(0.25)), (3, (age >= 2) & (n_obs <= th_obs)), (4, age >= 3)):
        action[free & rule] = code
        free &= ~rule
    return action

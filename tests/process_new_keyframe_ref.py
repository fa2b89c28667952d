"""LocalMapping::ProcessNewKeyFrame (SF/src/LocalMapping.cc:312-352) restated in Python from the reference's lines, on the flat graph that
tc2li_process_new_keyframe_batch takes (pinhole stereo rig: NLeft == -1, no second camera).  AddObservation, IsInKeyFrame,
UpdateNormalAndDepth and ComputeDistinctiveDescriptors are written here from SF/src/MapPoint.cc:150-175, :429-433, :435-503, :338-412;
KeyFrame::UpdateConnections (SF/src/KeyFrame.cc:391-486) is connections_ref.update_connections, fed with the observations as they are after
the loop.  Floats are numpy float32 scalars in the order tc2li_map_points_refresh documents: a norm is sqrtf((x*x + y*y) + z*z), the normal
is the sum of v / |v| over the observations in row order divided by their number, max = dist * level scale, min = max / last level scale.

The restatement keeps the objects' behaviour, not their layout: a point's observations are a dict keyframe -> index, as mObservations is a
map (iterating it is iterating its keys in ascending order), and the refresh runs inside the slot loop, at the slot's turn -- so it does not
share the device path's argument for deferring it.

A problem is a dict with the arrays of tc2li_process_keyframe_problem (those of tc2li_connections_problem beside it) and `current`,
`last_level_scale`; `views[kf_slot[k]]` is the keyframe of row k (descriptors, u_right)."""
import numpy as np

import connections_ref
from search_in_neighbors_ref import median_choice, norm_f32

f32 = np.float32


def process_new_keyframe(pr, views):
    cur = int(pr["current"])
    kf_bad = (np.asarray(pr["kf_flags"], np.uint8) & 1).astype(bool)
    point_bad = np.asarray(pr["point_bad"], np.uint8).astype(bool)
    n = len(point_bad)
    oo = [int(v) for v in pr["obs_offsets"]]
    obs = [dict((int(pr["obs_kf"][o]), int(pr["obs_index"][o])) for o in range(oo[p], oo[p + 1])) for p in range(n)]
    centres = np.asarray(pr["centres"], f32).reshape(-1, 3)
    positions = np.asarray(pr["positions"], f32).reshape(-1, 3)
    nobs = np.array(pr["point_nobs"], np.int32).copy()
    desc_kf, desc_index = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    refreshed = np.zeros(n, np.uint8)
    normals, mn, mx = np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, f32)
    view = lambda kf: views[int(pr["kf_slot"][kf])]
    associated_slot, associated_point, recent = [], [], []
    for i, p in enumerate(int(v) for v in pr["slot_point"]):               # LocalMapping.cc:326
        if p < 0:                                                          # :329
            continue
        if point_bad[p]:                                                   # :331
            continue
        if cur in obs[p]:                                                  # :333; MapPoint.cc:429-433
            recent.append(p)                                               # :341
            continue
        # :335 AddObservation (MapPoint.cc:150-175)
        obs[p][cur] = i                                                    # MapPoint.cc:169
        nobs[p] += 2 if view(cur)["u_right"][i] >= 0 else 1                # MapPoint.cc:171-174
        associated_slot.append(i)
        associated_point.append(p)
        # :336 UpdateNormalAndDepth (MapPoint.cc:435-503)
        rows = sorted(obs[p].items())                                      # MapPoint.cc:445, :456: map order
        pos = positions[p]
        normal = [f32(0), f32(0), f32(0)]
        for kf, _ in rows:                                                 # MapPoint.cc:456-475: no isBad() test
            v = [pos[0] - centres[kf][0], pos[1] - centres[kf][1], pos[2] - centres[kf][2]]   # MapPoint.cc:465
            nr = norm_f32(v)
            normal = [normal[0] + v[0] / nr, normal[1] + v[1] / nr, normal[2] + v[2] / nr]    # MapPoint.cc:466
        ref = int(pr["point_ref_kf"][p])
        pc = [pos[0] - centres[ref][0], pos[1] - centres[ref][1], pos[2] - centres[ref][2]]   # MapPoint.cc:477
        dist = norm_f32(pc)                                                # MapPoint.cc:478
        mx[p] = dist * f32(pr["point_ref_level_scale"][p])                 # MapPoint.cc:499
        mn[p] = mx[p] / f32(pr["last_level_scale"])                        # MapPoint.cc:500
        count = f32(len(rows))
        normals[p] = [normal[0] / count, normal[1] / count, normal[2] / count]   # MapPoint.cc:501
        refreshed[p] = 1
        # :337 ComputeDistinctiveDescriptors (MapPoint.cc:338-412)
        good = [(kf, idx) for kf, idx in rows if not kf_bad[kf]]           # MapPoint.cc:361
        if good:                                                           # MapPoint.cc:374
            b = median_choice([view(kf)["descriptors"][idx] for kf, idx in good])   # MapPoint.cc:377-406
            desc_kf[p], desc_index[p] = good[b]                            # MapPoint.cc:410
    flat = [sorted(o.items()) for o in obs]
    obs_offsets_out = np.concatenate([[0], np.cumsum([len(r) for r in flat])]).astype(np.int32)
    obs_kf_out = np.array([kf for r in flat for kf, _ in r], np.int32)
    obs_index_out = np.array([idx for r in flat for _, idx in r], np.int32)
    # :348 UpdateConnections on the observations as they are now
    conn = connections_ref.update_connections(dict(pr, obs_offsets=obs_offsets_out, obs_kf=obs_kf_out))
    i32 = lambda v: np.array(v, np.int32)
    return dict(associated_slot=i32(associated_slot), associated_point=i32(associated_point), recent=i32(recent), point_nobs_out=nobs,
                obs_offsets_out=obs_offsets_out, obs_kf_out=obs_kf_out, obs_index_out=obs_index_out, desc_kf=desc_kf, desc_index=desc_index,
                refreshed=refreshed, normals_out=normals, min_distance_out=mn, max_distance_out=mx, connections=conn)

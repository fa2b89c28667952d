"""The window of the local BA restated from the reference, for the tests of tc2li_ba_window_batch / tc2li_host_ba_window_batch /
tc2li_ba_window_outliers: the graph walk of OptimizerWithLidar::LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc; the same gather is
Optimizer::LocalBundleAdjustment, SF/src/Optimizer.cc:1124-1190) on the flat graph of tc2li_ba_window_problem, with the reference's mark
fields (mnBALocalForKF, mnBAFixedForKF) kept as fields and its containers as lists.  Line numbers are OptimizerWithLidar.cc's.  Plain loops:
this is the yardstick, not an implementation."""
import numpy as np

OK, ABORTED, MAX_LIDAR = 0, 1, 6
EDGE_DTYPE = np.dtype([("point", "<i4"), ("pose", "<i4"), ("u", "<f8"), ("v", "<f8"), ("u_right", "<f8"), ("inv_sigma2", "<f8")])
OUTPUTS = ("status", "num_fixed_kf", "num_opt_kf", "n_lidar", "n_points_without_edge", "pose_row", "poses7", "fixed", "point_row", "points3",
           "edges", "lidar_pose_index")


def gather(pr, views, inv_level_sigma2):
    """pr: the arrays and scalars of tc2li_ba_window_problem; views: per store slot None or a dict with keys (x, y, octave) and u_right.
    -> the outputs of the entry cut to their counts, plus n_fixed_without_edge (fixed cameras that no edge names)."""
    kf_slot, kf_id, kf_flags = (np.asarray(pr[k]).reshape(-1) for k in ("kf_slot", "kf_id", "kf_flags"))
    poses7, positions = np.asarray(pr["poses7"], np.float64).reshape(-1, 7), np.asarray(pr["positions"], np.float64).reshape(-1, 3)
    slot_off, slot_point, obs_off, obs_kf, obs_index = (np.asarray(pr[k]).reshape(-1) for k in ("slot_offsets", "slot_point", "obs_offsets", "obs_kf",
                                                                                                "obs_index"))
    point_flags = np.asarray(pr["point_flags"]).reshape(-1)
    sigma = np.asarray(inv_level_sigma2, np.float32)
    n_kf, n_pt = len(kf_slot), len(point_flags)
    pKF, mnId, init_id = int(pr["current"]), int(kf_id[int(pr["current"])]), int(pr["init_kf_id"])
    is_bad = lambda k: bool(kf_flags[k] & 1)
    this_map = lambda k: not (kf_flags[k] & 2)                                        # GetMap() == pCurrentMap
    kf_local_for, kf_fixed_for, mp_local_for = [None] * n_kf, [None] * n_kf, [None] * n_pt   # mnBALocalForKF, mnBAFixedForKF; of a point
    observations = lambda p: [(int(obs_kf[o]), int(obs_index[o])) for o in range(obs_off[p], obs_off[p + 1])]   # map order = row order

    lLocalKeyFrames = [pKF]                                                           # :65
    kf_local_for[pKF] = mnId                                                          # :66
    for pKFi in [int(k) for k in np.asarray(pr["cov_kf"]).reshape(-1)]:               # :70-76
        kf_local_for[pKFi] = mnId                                                     # :73
        if not is_bad(pKFi) and this_map(pKFi):                                       # :74
            lLocalKeyFrames.append(pKFi)                                              # :75
    num_fixedKF = 0                                                                   # :79
    lLocalMapPoints = []
    for pKFi in lLocalKeyFrames:                                                      # :82
        if int(kf_id[pKFi]) == init_id:                                               # :85
            num_fixedKF = 1                                                           # :87
        for pMP in [int(p) for p in slot_point[slot_off[pKFi]:slot_off[pKFi + 1]]]:   # :89-90
            if pMP >= 0:                                                              # :93
                if not (point_flags[pMP] & 1) and not (point_flags[pMP] & 2):         # :94
                    if mp_local_for[pMP] != mnId:                                     # :97
                        lLocalMapPoints.append(pMP)                                   # :99
                        mp_local_for[pMP] = mnId                                      # :100
    lFixedCameras = []
    for pMP in lLocalMapPoints:                                                       # :108
        for pKFi, _ in observations(pMP):                                             # :111
            if kf_local_for[pKFi] != mnId and kf_fixed_for[pKFi] != mnId:             # :115
                kf_fixed_for[pKFi] = mnId                                             # :117
                if not is_bad(pKFi) and this_map(pKFi):                               # :118
                    lFixedCameras.append(pKFi)                                        # :119
    num_fixedKF = len(lFixedCameras) + num_fixedKF                                    # :123
    empty = dict(pose_row=np.zeros(0, np.int32), poses7=np.zeros((0, 7)), fixed=np.zeros(0, np.uint8), point_row=np.zeros(0, np.int32),
                 points3=np.zeros((0, 3)), edges=np.zeros(0, EDGE_DTYPE), lidar_pose_index=np.zeros(0, np.int32))
    if num_fixedKF == 0:                                                              # :126-130
        return dict(empty, status=ABORTED, num_fixed_kf=0, num_opt_kf=0, n_lidar=0, n_points_without_edge=0, n_fixed_without_edge=0)
    # vertices (:157-187): setId(mnId), the optimiser's pose array is in id order
    vertices = [(int(kf_id[k]), k, int(kf_id[k]) == init_id) for k in lLocalKeyFrames]          # :163-164
    vertices += [(int(kf_id[k]), k, True) for k in lFixedCameras]                               # :180-181
    vertices.sort(key=lambda v: (v[0], v[1]))
    pose_of = {k: i for i, (_, k, _) in enumerate(vertices)}
    num_OptKF = len(lLocalKeyFrames)                                                  # :171
    vOptKeyFrames = [k for k in lLocalKeyFrames if kf_flags[k] & 4]                   # :228-233
    win_size = 0
    if len(vOptKeyFrames) > 2:                                                        # :235
        win_size = min(len(vOptKeyFrames), 6)                                         # :244-245
    lidar = [pose_of[vOptKeyFrames[i]] for i in range(win_size)]                      # :247-253
    edges, without = [], 0
    for i, pMP in enumerate(lLocalMapPoints):                                         # :263
        n_before = len(edges)
        for pKFi, leftIndex in observations(pMP):                                     # :277
            if not is_bad(pKFi) and this_map(pKFi):                                   # :281
                view = views[int(kf_slot[pKFi])]
                if leftIndex != -1 and view["u_right"][leftIndex] < 0:                # :286
                    kpUn = view["keys"][leftIndex]
                    edges.append((i, pose_of[pKFi], float(kpUn["x"]), float(kpUn["y"]), -1.0, float(sigma[int(kpUn["octave"])])))   # :290, :297
                elif leftIndex != -1 and view["u_right"][leftIndex] >= 0:             # :313
                    kpUn = view["keys"][leftIndex]
                    edges.append((i, pose_of[pKFi], float(kpUn["x"]), float(kpUn["y"]), float(view["u_right"][leftIndex]),
                                  float(sigma[int(kpUn["octave"])])))                 # :317-318, :325
        without += len(edges) == n_before
    e = np.array(edges, EDGE_DTYPE) if edges else np.zeros(0, EDGE_DTYPE)
    named = set(e["pose"].tolist())
    return dict(status=OK, num_fixed_kf=num_fixedKF, num_opt_kf=num_OptKF, n_lidar=win_size, n_points_without_edge=without,
                pose_row=np.array([k for _, k, _ in vertices], np.int32), poses7=poses7[[k for _, k, _ in vertices]].reshape(-1, 7),
                fixed=np.array([f for _, _, f in vertices], np.uint8), point_row=np.array(lLocalMapPoints, np.int32),
                points3=positions[lLocalMapPoints].reshape(-1, 3), edges=e, lidar_pose_index=np.array(lidar, np.int32),
                n_fixed_without_edge=sum(pose_of[k] not in named for k in lFixedCameras))


def outliers(edges, chi2, depth_positive, point_bad_now):
    """vToErase of :402-449 as (pose, point) pairs: vpEdgesMono, then vpEdgesStereo, each in creation order."""
    mono = [i for i in range(len(edges)) if edges["u_right"][i] < 0]                  # the edges of :292-311
    stereo = [i for i in range(len(edges)) if edges["u_right"][i] >= 0]               # the edges of :320-344
    vToErase = []
    for i in mono:                                                                    # :406
        if point_bad_now[edges["point"][i]]:                                          # :411
            continue
        if chi2[i] > 5.991 or not depth_positive[i]:                                  # :414
            vToErase.append((int(edges["pose"][i]), int(edges["point"][i])))          # :417
    for i in stereo:                                                                  # :436
        if point_bad_now[edges["point"][i]]:                                          # :441
            continue
        if chi2[i] > 7.815 or not depth_positive[i]:                                  # :444
            vToErase.append((int(edges["pose"][i]), int(edges["point"][i])))          # :447
    return np.array(vToErase, np.int32).reshape(-1, 2)

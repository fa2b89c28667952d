"""The window of the inertial local BA restated from the reference, for the tests of tc2li_inertial_window_batch /
tc2li_host_inertial_window_batch / tc2li_inertial_window_outliers: the graph walk of OptimizerWithLidar::LocalLVIBA
(SF/src/OptimizerWithLidar.cc:489-1045; the same text is Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512 and on, without the LiDAR
edge) on the flat graph of tc2li_inertial_window_problem, with the reference's mark fields (mnBALocalForKF, mnBAFixedForKF) kept as per-row
values and its containers as lists.  Line numbers are OptimizerWithLidar.cc's.  Plain sequential loops: this is the yardstick, not an
implementation."""
import numpy as np

OK, EMPTY, MAX_LIDAR = 0, 1, 6
EDGE_DTYPE = np.dtype([("point", "<i4"), ("pose", "<i4"), ("u", "<f8"), ("v", "<f8"), ("u_right", "<f8"), ("inv_sigma2", "<f8")])
OUTPUTS = ("status", "n_fixed_kf", "n_opt_kf", "n_lidar", "n_points_without_edge", "n_vertices_under_3_edges", "kf_row", "kf33", "fixed", "has_imu",
           "point_row", "points3", "edges", "link4", "link_kf2_row", "lidar_pose_index")


def gather(pr, views, inv_level_sigma2):
    """pr: the arrays and scalars of tc2li_inertial_window_problem; views: per store slot None or a dict with keys (x, y, octave) and
    u_right.  -> the outputs of the entry cut to their counts, plus what the branch test asks about: popped (the arm of :549-553),
    n_bad_marked (bad observers that got the fixed mark at :597), capped (the break of :606 was taken)."""
    kf_slot, kf_id, kf_flags, prev_kf = (np.asarray(pr[k]).reshape(-1) for k in ("kf_slot", "kf_id", "kf_flags", "prev_kf"))
    states, positions = np.asarray(pr["states"], np.float64).reshape(-1, 33), np.asarray(pr["positions"], np.float64).reshape(-1, 3)
    slot_off, slot_point, obs_off, obs_kf, obs_index = (np.asarray(pr[k]).reshape(-1) for k in ("slot_offsets", "slot_point", "obs_offsets", "obs_kf",
                                                                                                "obs_index"))
    point_flags = np.asarray(pr["point_flags"]).reshape(-1)
    sigma = np.asarray(inv_level_sigma2, np.float32)
    n_kf, n_pt = len(kf_slot), len(point_flags)
    pKF = int(pr["current"])
    mnId = int(kf_id[pKF])
    bLarge, bRecInit, with_lidar = bool(pr.get("large", 0)), bool(pr.get("rec_init", 0)), bool(pr.get("with_lidar", 0))
    is_bad = lambda k: bool(kf_flags[k] & 1)
    this_map = lambda k: not (kf_flags[k] & 2)                                        # GetMap() == pCurrentMap
    bImu = lambda k: bool(kf_flags[k] & 4)
    has_preintegrated = lambda k: bool(kf_flags[k] & 8)                               # mpImuPreintegrated != NULL
    mPrevKF = lambda k: int(prev_kf[k]) if prev_kf[k] >= 0 else None
    # mnBALocalForKF, mnBAFixedForKF; of a point.  "unset" stands for whatever an earlier call left: not this keyframe's id
    kf_local_for, kf_fixed_for, mp_local_for = ["unset"] * n_kf, ["unset"] * n_kf, ["unset"] * n_pt
    observations = lambda p: [(int(obs_kf[o]), int(obs_index[o])) for o in range(obs_off[p], obs_off[p + 1])]   # map order = row order

    maxOpt = 10                                                                       # :493
    if bLarge:                                                                        # :495
        maxOpt = 25                                                                   # :497
    Nd = min(int(pr["keyframes_in_map"]) - 2, maxOpt)                                 # :500
    vpOptimizableKFs = [pKF]                                                          # :508
    kf_local_for[pKF] = mnId                                                          # :509
    for i in range(1, Nd):                                                            # :510
        if mPrevKF(vpOptimizableKFs[-1]) is not None:                                 # :512
            vpOptimizableKFs.append(mPrevKF(vpOptimizableKFs[-1]))                    # :514
            kf_local_for[vpOptimizableKFs[-1]] = mnId                                 # :515
        else:
            break                                                                     # :518
    N = len(vpOptimizableKFs)                                                         # :521
    lLocalMapPoints = []
    for i in range(N):                                                                # :525
        k = vpOptimizableKFs[i]
        for pMP in [int(p) for p in slot_point[slot_off[k]:slot_off[k + 1]]]:         # :527-528
            if pMP >= 0:                                                              # :531
                if not (point_flags[pMP] & 1):                                        # :532 -- isBad() alone
                    if mp_local_for[pMP] != mnId:                                     # :533
                        lLocalMapPoints.append(pMP)                                   # :535
                        mp_local_for[pMP] = mnId                                      # :536
    lFixedKeyFrames = []
    popped = False
    if mPrevKF(vpOptimizableKFs[-1]) is not None:                                     # :543
        lFixedKeyFrames.append(mPrevKF(vpOptimizableKFs[-1]))                         # :545
        kf_fixed_for[mPrevKF(vpOptimizableKFs[-1])] = mnId                            # :546
    else:
        kf_local_for[vpOptimizableKFs[-1]] = 0                                        # :550
        kf_fixed_for[vpOptimizableKFs[-1]] = mnId                                     # :551
        lFixedKeyFrames.append(vpOptimizableKFs[-1])                                  # :552
        vpOptimizableKFs.pop()                                                        # :553
        popped = True
    # :557-584: maxCovKF = 0, lpOptVisKFs.size() >= 0 breaks on entry
    empty = dict(kf_row=np.zeros(0, np.int32), kf33=np.zeros((0, 33)), fixed=np.zeros(0, np.uint8), has_imu=np.zeros(0, np.uint8),
                 point_row=np.zeros(0, np.int32), points3=np.zeros((0, 3)), edges=np.zeros(0, EDGE_DTYPE), link4=np.zeros((0, 4)),
                 link_kf2_row=np.zeros(0, np.int32), lidar_pose_index=np.zeros(0, np.int32))
    if not vpOptimizableKFs:                                                          # nothing left to optimise
        return dict(empty, status=EMPTY, n_fixed_kf=1, n_opt_kf=0, n_lidar=0, n_points_without_edge=0, n_vertices_under_3_edges=0, popped=True,
                    n_bad_marked=0, capped=False)
    maxFixKF = 200                                                                    # :586
    n_bad_marked, capped = 0, False
    for pMP in lLocalMapPoints:                                                       # :588
        for pKFi, _ in observations(pMP):                                             # :591
            if kf_local_for[pKFi] != mnId and kf_fixed_for[pKFi] != mnId:             # :595
                kf_fixed_for[pKFi] = mnId                                             # :597
                if not is_bad(pKFi):                                                  # :598
                    lFixedKeyFrames.append(pKFi)                                      # :600
                    break                                                             # :601
                n_bad_marked += 1
        if len(lFixedKeyFrames) >= maxFixKF:                                          # :605
            capped = True
            break                                                                     # :606
    N = len(vpOptimizableKFs)                                                         # :633
    # vertices (:634-696): setId(mnId), the optimiser's keyframe array is in id order
    vertices = [(int(kf_id[k]), k, False) for k in vpOptimizableKFs]                  # :639-640
    vertices += [(int(kf_id[k]), k, True) for k in lFixedKeyFrames]                   # :677-678
    vertices.sort(key=lambda v: (v[0], v[1]))
    vertex_of = {k: i for i, (_, k, _) in enumerate(vertices)}
    lidar = []
    N1 = N                                                                            # :709
    if with_lidar and N1 > 5:                                                         # :710
        if N1 > 6:
            N1 = 6                                                                    # :712
        lidar = [vertex_of[vpOptimizableKFs[i]] for i in range(N1)]                   # :715-720
    link4, link_kf2_row = [], []
    for i in range(N):                                                                # :734
        pKFi = vpOptimizableKFs[i]
        if mPrevKF(pKFi) is None:                                                     # :738
            continue
        if bImu(pKFi) and bImu(mPrevKF(pKFi)) and has_preintegrated(pKFi):            # :743
            if mPrevKF(pKFi) not in vertex_of:                                        # :746, :755 (cannot happen: see the header)
                continue
            robust = i == N - 1 or bRecInit                                           # :770
            link4.append([vertex_of[mPrevKF(pKFi)], vertex_of[pKFi], 1.0 if robust else 0.0, 1e-2 if i == N - 1 else 1.0])   # :778-779
            link_kf2_row.append(pKFi)
    mVisEdges = {k: 0 for _, k, _ in vertices}                                        # :834-843, by row
    edges, without = [], 0
    for i, pMP in enumerate(lLocalMapPoints):                                         # :845
        n_before = len(edges)
        for pKFi, leftIndex in observations(pMP):                                     # :858
            if kf_local_for[pKFi] != mnId and kf_fixed_for[pKFi] != mnId:             # :862
                continue
            if not is_bad(pKFi) and this_map(pKFi):                                   # :865
                view = views[int(kf_slot[pKFi])]
                if leftIndex != -1 and view["u_right"][leftIndex] < 0:                # :872
                    mVisEdges[pKFi] += 1                                              # :874
                    kpUn = view["keys"][leftIndex]
                    edges.append((i, vertex_of[pKFi], float(kpUn["x"]), float(kpUn["y"]), -1.0, float(sigma[int(kpUn["octave"])])))   # :878, :889
                elif leftIndex != -1:                                                 # :902
                    kpUn = view["keys"][leftIndex]
                    mVisEdges[pKFi] += 1                                              # :905
                    edges.append((i, vertex_of[pKFi], float(kpUn["x"]), float(kpUn["y"]), float(view["u_right"][leftIndex]),
                                  float(sigma[int(kpUn["octave"])])))                 # :907-909, :920
        without += len(edges) == n_before
    e = np.array(edges, EDGE_DTYPE) if edges else np.zeros(0, EDGE_DTYPE)
    rows = [k for _, k, _ in vertices]
    return dict(status=OK, n_fixed_kf=len(lFixedKeyFrames), n_opt_kf=N, n_lidar=len(lidar), n_points_without_edge=without,
                n_vertices_under_3_edges=sum(v < 3 for v in mVisEdges.values()),      # :972-975, counted and not asserted
                kf_row=np.array(rows, np.int32), kf33=states[rows].reshape(-1, 33), fixed=np.array([f for _, _, f in vertices], np.uint8),
                has_imu=np.array([bImu(k) for k in rows], np.uint8), point_row=np.array(lLocalMapPoints, np.int32),
                points3=positions[lLocalMapPoints].reshape(-1, 3), edges=e, link4=np.array(link4, np.float64).reshape(-1, 4),
                link_kf2_row=np.array(link_kf2_row, np.int32), lidar_pose_index=np.array(lidar, np.int32), popped=popped, n_bad_marked=n_bad_marked,
                capped=capped)


def outliers(edges, chi2, depth_positive, point_bad_now, track_depth, initial_chi2, final_chi2, large):
    """(vToErase of :985-1021 as (pose, point) pairs: vpEdgesMono, then vpEdgesStereo, each in creation order; the rejection of :1028)."""
    chi2Mono2 = np.float32(5.991)                                                     # :828
    chi2Stereo2 = np.float32(7.815)                                                   # :830
    with np.errstate(all="ignore"):
        err, err_end = np.float32(initial_chi2), np.float32(final_chi2)               # :979, :981
    mono = [i for i in range(len(edges)) if edges["u_right"][i] < 0]                  # the edges of :880-899
    stereo = [i for i in range(len(edges)) if edges["u_right"][i] >= 0]               # the edges of :911-930
    vToErase = []
    for i in mono:                                                                    # :990
        bClose = np.float32(track_depth[edges["point"][i]]) < np.float32(10.0)        # :994
        if point_bad_now[edges["point"][i]]:                                          # :996
            continue
        c = np.float64(chi2[i])
        if (c > np.float64(chi2Mono2) and not bClose) or (c > np.float64(np.float32(1.5) * chi2Mono2) and bClose) or not depth_positive[i]:   # :999
            vToErase.append((int(edges["pose"][i]), int(edges["point"][i])))          # :1002
    for i in stereo:                                                                  # :1008
        if point_bad_now[edges["point"][i]]:                                          # :1013
            continue
        if np.float64(chi2[i]) > np.float64(chi2Stereo2):                             # :1016
            vToErase.append((int(edges["pose"][i]), int(edges["point"][i])))          # :1019
    with np.errstate(all="ignore"):
        rejected = bool((np.float32(2) * err < err_end or np.isnan(err) or np.isnan(err_end)) and not large)   # :1028
    if rejected:
        return np.zeros((0, 2), np.int32), True                                      # :1031
    return np.array(vToErase, np.int32).reshape(-1, 2), False

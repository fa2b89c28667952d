"""Plain Python restatement of the matching loops of the two tracking overloads of ORBmatcher::SearchByProjection -- the checker of
tests/test_projection_cases.py and tests/test_projection_gates_gpu.py.  Written from the reference source, line by line and sequentially:
(Frame&, const Frame& LastFrame, th, bMono) SF/src/ORBmatcher.cc:1685-1896 and (Frame&, const vector<MapPoint*>&, th, bFarPoints,
thFarPoints) :52-222, with Frame::isInFrustum (SF/src/Frame.cc:542-603), MapPoint::PredictScale (SF/src/MapPoint.cc:540-555) and
ORBmatcher::RadiusByViewingCos (:224-230).  The grid and the Hamming distance are the oracle's (features_in_area, descriptor_distance), the
histogram is bow_ref's, the level reloc_ref's; nothing here goes through oracle.search_by_projection.  Float steps are numpy float32
scalars, doubles Python floats."""
import numpy as np

import bow_ref
import reloc_ref as R

F32 = np.float32
TH_HIGH = 100


def match_loop(oracle, keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio):
    """The sequential loop body of both overloads (:85-149 with mode 1, :1752-1802 with mode 0) over ready-made queries.
    occupied[i]: F.mvpMapPoints[i] holds a point with Observations() > 0 on entry.
    -> (nmatches, match_of_query, point_of_keypoint, rotHist as a list of (bin, keypoint) in the order of the push_backs of :1800)."""
    N, M = len(keys), len(queries)
    point = np.full(N, -1, np.int32)                   # mvpMapPoints: the query whose point the keypoint holds
    blocked = [False] * N                               # mvpMapPoints[i] && mvpMapPoints[i]->Observations() > 0
    if occupied is not None:
        blocked = [bool(o) for o in occupied]
    match = np.full(M, -1, np.int32)
    entries = []
    ratio = F32(nn_ratio)
    nmatches = 0
    octave = [int(o) for o in keys["octave"]]
    ur = [F32(x) for x in u_right]
    has_ur = [bool(x > 0) for x in ur]
    seen = {}                                           # oracle.descriptor_distance per (query descriptor, keypoint): one call each
    for q in range(M):
        Q = queries[q]
        if not Q["valid"]:
            continue
        radius = F32(Q["radius"])
        idx = oracle.features_in_area(keys, cols, rows, float(Q["u"]), float(Q["v"]), float(radius), int(Q["min_level"]), int(Q["max_level"]))
        if len(idx) == 0:
            continue
        best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
        q_ur = F32(Q["u_right"])
        row = seen.setdefault(Q["descriptor"].tobytes(), {})
        for i in idx.tolist():
            if blocked[i]:                                                     # :97-99, :1756-1758
                continue
            if has_ur[i]:                                                      # :101-106, :1760-1766
                er = F32(abs(F32(q_ur - ur[i])))
                if er > radius:
                    continue
            dist = row.get(i)
            if dist is None:
                dist = row[i] = int(oracle.descriptor_distance(Q["descriptor"], desc[i]))
            if mode == 0:                                                      # :1772-1776
                if dist < best_dist:
                    best_dist, best_idx = dist, i
            elif dist < best_dist:                                             # :112-121
                best_dist2, best_level2 = best_dist, best_level
                best_dist, best_level, best_idx = dist, octave[i], i
            elif dist < best_dist2:                                            # :122-128
                best_level2, best_dist2 = octave[i], dist
        if best_dist > TH_HIGH:                                                # :132, :1779
            continue
        if mode != 0:
            if best_level == best_level2 and F32(best_dist) > F32(ratio * F32(best_dist2)):          # :134-135
                continue
            if not (best_level != best_level2 or F32(best_dist) <= F32(ratio * F32(best_dist2))):   # :137
                continue
        point[best_idx] = q
        if Q["has_observations"]:
            blocked[best_idx] = True
        match[q] = best_idx
        nmatches += 1
        entries.append((bow_ref.rot_bin(Q["angle"], keys["angle"][best_idx]), best_idx))          # :1784-1801
    return nmatches, match, point, entries


def rotation_filter(nmatches, match, point, entries):
    """:1873-1892 on what match_loop left: mvpMapPoints is cleared by KEYPOINT index (:1888) and nmatches drops once per rejected
    histogram entry (:1889).  match_of_query[q] is the keypoint query q wrote to, -1 once the filter has cleared that keypoint."""
    match, point = match.copy(), point.copy()
    hist = [0] * bow_ref.HISTO_LENGTH
    for b, _ in entries:
        hist[b] += 1
    inds = bow_ref.compute_three_maxima(hist)
    for b in range(bow_ref.HISTO_LENGTH):
        if b in inds:
            continue
        for eb, i in entries:
            if eb == b:
                point[i] = -1
                nmatches -= 1
    for q in range(len(match)):
        if match[q] >= 0 and point[match[q]] < 0:
            match[q] = -1
    return nmatches, match, point


def search_queries(oracle, keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio, check_orientation):
    """match_loop, then with check_orientation the rotation filter (the reference applies it in the last-frame overload; here it follows
    the argument in either mode) -> (nmatches, match_of_query [M], point_of_keypoint [N]); point_of_keypoint is mvpMapPoints as the
    reference leaves it: written at the match (:138, :1781), cleared in the filter."""
    n, match, point, entries = match_loop(oracle, keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio)
    return rotation_filter(n, match, point, entries) if check_orientation else (n, match, point)


def search_queries_both(oracle, keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio):
    """search_queries without and with check_orientation from one pass of the loop, which does not depend on it -> {False: ..., True: ...}."""
    n, match, point, entries = match_loop(oracle, keys, desc, u_right, occupied, cols, rows, queries, mode, nn_ratio)
    return {False: (n, match, point), True: rotation_filter(n, match, point, entries)}


def rotation_matrix(q):
    """Eigen::Quaternionf::toRotationMatrix (mRcw of Frame::UpdatePoseMatrices), q = x y z w -> 9 floats, row-major."""
    q = [F32(x) for x in q]
    two = F32(2)
    tx, ty, tz = F32(two * q[0]), F32(two * q[1]), F32(two * q[2])
    twx, twy, twz = F32(tx * q[3]), F32(ty * q[3]), F32(tz * q[3])
    txx, txy, txz = F32(tx * q[0]), F32(ty * q[0]), F32(tz * q[0])
    tyy, tyz, tzz = F32(ty * q[1]), F32(tz * q[1]), F32(tz * q[2])
    one = F32(1)
    return [F32(one - F32(tyy + tzz)), F32(txy - twz), F32(txz + twy),
            F32(txy + twz), F32(one - F32(txx + tzz)), F32(tyz - twx),
            F32(txz - twy), F32(tyz + twx), F32(one - F32(txx + tyy))]


def in_frustum(point, pose7, cam, cols, rows, log_scale, n_levels, cos_limit=0.5):
    """Frame::isInFrustum(pMP, viewingCosLimit) with Nleft == -1 for one tc2li_map_point record -> None (not in view) or a dict of what
    the reference stores in the MapPoint: u, v (mTrackProjX/Y), u_right (mTrackProjXR), depth (mTrackDepth), level, view_cos, dist."""
    q = [F32(x) for x in pose7]
    fx, fy, cx, cy, bf = [F32(x) for x in cam[:5]]
    Rm = rotation_matrix(q[:4])
    Ow = R.quat_rotate([F32(-q[0]), F32(-q[1]), F32(-q[2]), q[3]], [F32(q[4] * F32(-1)), F32(q[5] * F32(-1)), F32(q[6] * F32(-1))])
    P = [F32(x) for x in point["pos"]]
    Pc = [F32(F32(F32(F32(Rm[3 * r] * P[0]) + F32(Rm[3 * r + 1] * P[1])) + F32(Rm[3 * r + 2] * P[2])) + q[4 + r]) for r in range(3)]
    pc_dist = F32(np.sqrt(F32(F32(F32(Pc[0] * Pc[0]) + F32(Pc[1] * Pc[1])) + F32(Pc[2] * Pc[2]))))
    if Pc[2] < F32(0):
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        invz = F32(F32(1) / Pc[2])
        u = F32(F32(F32(fx * Pc[0]) / Pc[2]) + cx)
        v = F32(F32(F32(fy * Pc[1]) / Pc[2]) + cy)
    if u < F32(0) or u > F32(cols) or v < F32(0) or v > F32(rows):
        return None
    PO = [F32(P[k] - Ow[k]) for k in range(3)]
    dist = F32(np.sqrt(F32(F32(F32(PO[0] * PO[0]) + F32(PO[1] * PO[1])) + F32(PO[2] * PO[2]))))
    if dist < F32(point["min_distance"]) or dist > F32(point["max_distance"]):
        return None
    n = [F32(x) for x in point["normal"]]
    view_cos = F32(F32(F32(F32(PO[0] * n[0]) + F32(PO[1] * n[1])) + F32(PO[2] * n[2])) / dist)
    if view_cos < F32(cos_limit):
        return None
    level = R.predict_scale(point["max_distance_raw"], dist, log_scale, n_levels)
    return dict(u=u, v=v, u_right=F32(u - F32(bf * invz)), depth=pc_dist, level=level, view_cos=view_cos, dist=dist)


def radius_by_viewing_cos(view_cos):
    """ORBmatcher::RadiusByViewingCos (:224-230): `viewCos > 0.998` compares the float with the DOUBLE constant."""
    return F32(2.5) if float(view_cos) > 0.998 else F32(4.0)


def local_queries(oracle, points, pose7, cam, scales, log_scale, cols, rows, th, far, th_far):
    """The queries of SearchLocalPoints: isInFrustum(pMP, 0.5), then the window of ORBmatcher.cc:62-81 -> (queries, views); views[k] is
    in_frustum's dict or None."""
    qs = np.zeros(len(points), oracle.QUERY_DTYPE)
    qs["u_right"], qs["min_level"], qs["max_level"], qs["has_observations"] = -1, -1, -1, 1
    views = []
    factor = float(F32(th)) != 1.0
    for k in range(len(points)):
        view = in_frustum(points[k], pose7, cam, cols, rows, log_scale, len(scales))
        views.append(view)
        if view is None:
            continue
        if far and view["depth"] > F32(th_far):                                # :64-65
            continue
        r = radius_by_viewing_cos(view["view_cos"])                            # :75
        if factor:
            r = F32(r * F32(th))                                               # :77-78
        Q = qs[k]
        Q["u"], Q["v"], Q["u_right"] = view["u"], view["v"], view["u_right"]
        Q["radius"] = F32(r * F32(scales[view["level"]]))                      # :81
        Q["min_level"], Q["max_level"] = view["level"] - 1, view["level"]
        Q["valid"] = 1
        Q["descriptor"] = points[k]["descriptor"]
    return qs, views


def search_local_points(oracle, frame, points, pose7, cam, scales, log_scale, th, far, th_far):
    """Tracking::SearchLocalPoints' data path for one frame: frame = dict(keys, descriptors, u_right, held, cols, rows), held as in
    tc2li_track_local_map_batch (1 = a point with observations, it blocks); points: tc2li_map_point records; cam = fx fy cx cy bf.
    -> (local_of_keypoint [N], n_matches): mode 1 with ORBmatcher(0.8), no orientation check (:52-222 has none)."""
    qs, _ = local_queries(oracle, points, pose7, cam, scales, log_scale, frame["cols"], frame["rows"], th, far, th_far)
    occupied = np.asarray(frame["held"]) == 1
    n, _, point = search_queries(oracle, frame["keys"], frame["descriptors"], frame["u_right"], occupied, frame["cols"], frame["rows"], qs, 1, 0.8, False)
    return point, n

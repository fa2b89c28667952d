"""An independent float64 restatement of local mapping's geometric front half, for the directed tests of mapping_kernels.hip.

Written from the reference text -- ORBmatcher::SearchForTriangulation (ORBmatcher.cc:916-1155), Pinhole::epipolarConstrain
(Pinhole.cpp:116-138), LocalMapping::CreateNewMapPoints (LocalMapping.cc:448-725), ORBmatcher::Fuse (ORBmatcher.cc:1157-1330),
KeyFrame::GetFeaturesInArea / IsInImage / UnprojectStereo (KeyFrame.cc:716-784), MapPoint::PredictScale (MapPoint.cc:523-538),
GeometricTools::Triangulate (GeometricTools.cc:56-75) -- and not from oracle/mapping.cpp or the kernels: float64 throughout, rotation
matrices (a pose's quaternion is turned into one once, on entry), np.linalg.svd for the triangulation.  Stereo / pinhole branch only, as
the product.  Keyframes are the dicts of capi.pack_keyframe_views; results come in the product's shapes."""
import numpy as np

TH_LOW, HISTO_LENGTH = 50, 30
GRID_COLS, GRID_ROWS = 64, 48


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def pose_Rt(pose7):
    """Tcw = (x, y, z, w, tx, ty, tz) -> (Rcw, tcw), float64; R = I + 2 w [v]x + 2 [v]x^2 of the normalised quaternion."""
    p = np.asarray(pose7, np.float64)
    q = p[:4] / np.linalg.norm(p[:4])
    V = hat(q[:3])
    return np.eye(3) + 2.0 * q[3] * V + 2.0 * (V @ V), p[4:7].copy()


def K_of(cam4):
    fx, fy, cx, cy = [float(v) for v in np.asarray(cam4)[:4]]
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def feature_vector(kf):
    """node -> keypoint indices in the order of the feature vector"""
    off = np.asarray(kf["fv_offset"])
    return {int(n): [int(i) for i in kf["fv_index"][off[a]:off[a + 1]]] for a, n in enumerate(kf["fv_node"])}


def xy(kf, i):
    return float(kf["keys"]["x"][i]), float(kf["keys"]["y"][i])


def search_for_triangulation(kf1, kf2, cam4, sf, sigma2, only_stereo=False, coarse=False, check_orientation=False, has_point1=None):
    """-> (nmatches, match12 [n1])"""
    K = K_of(cam4)
    Kinv = np.linalg.inv(K)
    R1, t1 = pose_Rt(kf1["pose7"])
    R2, t2 = pose_Rt(kf2["pose7"])
    Cw = -R1.T @ t1                                   # GetCameraCenter
    C2 = R2 @ Cw + t2
    ep = (K[0, 0] * C2[0] / C2[2] + K[0, 2], K[1, 1] * C2[1] / C2[2] + K[1, 2]) if C2[2] != 0 else (np.inf, np.inf)
    R12 = R1 @ R2.T                                   # T12 = T1w * Tw2
    t12 = t1 - R12 @ t2
    F12 = Kinv.T @ hat(t12) @ R12 @ Kinv
    hp1 = kf1["has_point"] if has_point1 is None else has_point1
    fv1, fv2 = feature_vector(kf1), feature_vector(kf2)
    match = np.full(len(kf1["keys"]), -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    for node in sorted(set(fv1) & set(fv2)):
        for idx1 in fv1[node]:
            if hp1[idx1]:
                continue
            stereo1 = kf1["u_right"][idx1] >= 0
            if only_stereo and not stereo1:
                continue
            x1, y1 = xy(kf1, idx1)
            best_dist, best = TH_LOW, -1
            for idx2 in fv2[node]:
                if kf2["has_point"][idx2]:
                    continue
                stereo2 = kf2["u_right"][idx2] >= 0
                if only_stereo and not stereo2:
                    continue
                dist = hamming(kf1["descriptors"][idx1], kf2["descriptors"][idx2])
                if dist > TH_LOW or dist > best_dist:
                    continue
                x2, y2 = xy(kf2, idx2)
                o2 = int(kf2["keys"]["octave"][idx2])
                if not stereo1 and not stereo2:
                    if (ep[0] - x2) ** 2 + (ep[1] - y2) ** 2 < 100.0 * float(sf[o2]):
                        continue
                ok = bool(coarse)
                if not ok:                            # Pinhole::epipolarConstrain
                    a = x1 * F12[0, 0] + y1 * F12[1, 0] + F12[2, 0]
                    b = x1 * F12[0, 1] + y1 * F12[1, 1] + F12[2, 1]
                    c = x1 * F12[0, 2] + y1 * F12[1, 2] + F12[2, 2]
                    den = a * a + b * b
                    ok = den != 0 and (a * x2 + b * y2 + c) ** 2 / den < 3.84 * float(sigma2[o2])
                if ok:
                    best, best_dist = idx2, dist
            if best >= 0:
                match[idx1] = best
                if check_orientation:
                    rot = float(kf1["keys"]["angle"][idx1]) - float(kf2["keys"]["angle"][best])
                    if rot < 0.0:
                        rot += 360.0
                    b = int(np.floor(rot / HISTO_LENGTH + 0.5))
                    hist[0 if b == HISTO_LENGTH else b].append(idx1)
    if check_orientation:                             # ComputeThreeMaxima (ORBmatcher.cc:2021-2062)
        m1 = m2 = m3 = 0
        i1 = i2 = i3 = -1
        for i, h in enumerate(hist):
            s = len(h)
            if s > m1:
                m3, m2, m1, i3, i2, i1 = m2, m1, s, i2, i1, i
            elif s > m2:
                m3, m2, i3, i2 = m2, s, i2, i
            elif s > m3:
                m3, i3 = s, i
        if m2 < 0.1 * m1:
            i2 = i3 = -1
        elif m3 < 0.1 * m1:
            i3 = -1
        for i, h in enumerate(hist):
            if i not in (i1, i2, i3):
                match[h] = -1
    return int((match >= 0).sum()), match


def triangulate(xn1, xn2, T1, T2):
    A = np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]])
    h = np.linalg.svd(A)[2][3]
    return None if h[3] == 0 else h[:3] / h[3]


def create_new_map_points(cur, neighbours, cam4, mb, mbf, sf, sigma2, scale_factor=1.2, inertial=False, far_points=False, th_far_points=0.0,
                          coarse=False):
    """-> (idx [k, 4] = idx1, neighbour, idx2, stereo in creation order; x3D [k, 3] float64)"""
    fx, fy, cx, cy = [float(v) for v in np.asarray(cam4)[:4]]
    R1, t1 = pose_Rt(cur["pose7"])
    O1 = -R1.T @ t1
    T1 = np.hstack([R1, t1[:, None]])
    ratio_factor = 1.5 * scale_factor
    has1 = np.array(cur["has_point"], np.uint8).copy()
    rows, pts = [], []

    def gate(R, t, X, kx, ky, stereo, ur, sig):
        x, y, z = R @ X + t
        if z <= 0:
            return False
        u, v = fx * x / z + cx, fy * y / z + cy
        if not stereo:
            return not ((u - kx) ** 2 + (v - ky) ** 2 > 5.991 * sig)
        return not ((u - kx) ** 2 + (v - ky) ** 2 + (u - mbf / z - ur) ** 2 > 7.8 * sig)

    for j, kf2 in enumerate(neighbours):
        R2, t2 = pose_Rt(kf2["pose7"])
        O2 = -R2.T @ t2
        if np.linalg.norm(O2 - O1) < mb:
            continue
        _, match = search_for_triangulation(cur, kf2, cam4, sf, sigma2, False, coarse, False, has_point1=has1)
        T2 = np.hstack([R2, t2[:, None]])
        for idx1 in np.nonzero(match >= 0)[0]:
            idx2 = int(match[idx1])
            (x1, y1), (x2, y2) = xy(cur, idx1), xy(kf2, idx2)
            ur1, ur2 = float(cur["u_right"][idx1]), float(kf2["u_right"][idx2])
            stereo1, stereo2 = ur1 >= 0, ur2 >= 0
            xn1 = np.array([(x1 - cx) / fx, (y1 - cy) / fy, 1.0])
            xn2 = np.array([(x2 - cx) / fx, (y2 - cy) / fy, 1.0])
            ray1, ray2 = R1.T @ xn1, R2.T @ xn2
            cos_rays = ray1 @ ray2 / (np.linalg.norm(ray1) * np.linalg.norm(ray2))
            cos_s1 = cos_s2 = cos_rays + 1
            if stereo1:
                cos_s1 = np.cos(2 * np.arctan2(mb / 2, float(cur["depth"][idx1])))
            elif stereo2:
                cos_s2 = np.cos(2 * np.arctan2(mb / 2, float(kf2["depth"][idx2])))
            cos_s = min(cos_s1, cos_s2)
            point_stereo = False
            if cos_rays < cos_s and cos_rays > 0 and (stereo1 or stereo2 or (cos_rays < 0.9996 and inertial) or (cos_rays < 0.9998 and not inertial)):
                X = triangulate(xn1, xn2, T1, T2)
                if X is None:
                    continue
            elif stereo1 and cos_s1 < cos_s2:
                point_stereo = True
                z = float(cur["depth"][idx1])
                if not z > 0:
                    continue
                X = R1.T @ np.array([(x1 - cx) * z / fx, (y1 - cy) * z / fy, z]) + O1
            elif stereo2 and cos_s2 < cos_s1:
                point_stereo = True
                z = float(kf2["depth"][idx2])
                if not z > 0:
                    continue
                X = R2.T @ np.array([(x2 - cx) * z / fx, (y2 - cy) * z / fy, z]) + O2
            else:
                continue
            if not gate(R1, t1, X, x1, y1, stereo1, ur1, float(sigma2[cur["keys"]["octave"][idx1]])):
                continue
            if not gate(R2, t2, X, x2, y2, stereo2, ur2, float(sigma2[kf2["keys"]["octave"][idx2]])):
                continue
            dist1, dist2 = np.linalg.norm(X - O1), np.linalg.norm(X - O2)
            if dist1 == 0 or dist2 == 0:
                continue
            if far_points and (dist1 >= th_far_points or dist2 >= th_far_points):
                continue
            ratio_dist = dist2 / dist1
            ratio_octave = float(sf[cur["keys"]["octave"][idx1]]) / float(sf[kf2["keys"]["octave"][idx2]])
            if ratio_dist * ratio_factor < ratio_octave or ratio_dist > ratio_octave * ratio_factor:
                continue
            rows.append((int(idx1), j, idx2, int(point_stereo)))
            pts.append(X)
            has1[idx1] = 1                             # mpCurrentKeyFrame->AddMapPoint(pMP, idx1)
    return np.array(rows, np.int32).reshape(-1, 4), np.array(pts, np.float64).reshape(-1, 3)


def fuse_search(keys, desc, u_right, bounds, pose7, cam4, bf, sf, inv_sigma2, log_scale_factor, points, valid, th=3.0):
    """bounds = (min_x, max_x, min_y, max_y) -> (n_fused, best_idx [m], best_dist [m])"""
    fx, fy, cx, cy = [float(v) for v in np.asarray(cam4)[:4]]
    min_x, max_x, min_y, max_y = [float(np.float32(b)) for b in bounds]
    inv_w, inv_h = GRID_COLS / (max_x - min_x), GRID_ROWS / (max_y - min_y)
    grid = {}
    for i in range(len(keys)):                         # AssignFeaturesToGrid / PosInGrid
        px = int(np.floor((float(keys["x"][i]) - min_x) * inv_w + 0.5))
        py = int(np.floor((float(keys["y"][i]) - min_y) * inv_h + 0.5))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid.setdefault((px, py), []).append(i)
    R, t = pose_Rt(pose7)
    Ow = -R.T @ t
    n_levels = len(sf)
    m = len(points)
    best_idx, best_dist = np.full(m, -1, np.int32), np.full(m, 256, np.int32)
    for i in range(m):
        if not valid[i]:
            continue
        P = points[i]
        Xw = np.asarray(P["pos"], np.float64)
        x, y, z = R @ Xw + t
        if z < 0.0:
            continue
        u, v = fx * x / z + cx, fy * y / z + cy
        if not (min_x <= u < max_x and min_y <= v < max_y):
            continue
        ur = u - bf / z
        PO = Xw - Ow
        dist3D = np.linalg.norm(PO)
        if dist3D < float(P["min_distance"]) or dist3D > float(P["max_distance"]):
            continue
        if PO @ np.asarray(P["normal"], np.float64) < 0.5 * dist3D:
            continue
        level = int(np.ceil(np.log(float(P["max_distance_raw"]) / dist3D) / log_scale_factor))
        level = min(max(level, 0), n_levels - 1)
        r = th * float(sf[level])
        c0, c1 = max(0, int(np.floor((u - min_x - r) * inv_w))), min(GRID_COLS - 1, int(np.ceil((u - min_x + r) * inv_w)))
        r0, r1 = max(0, int(np.floor((v - min_y - r) * inv_h))), min(GRID_ROWS - 1, int(np.ceil((v - min_y + r) * inv_h)))
        if c0 >= GRID_COLS or c1 < 0 or r0 >= GRID_ROWS or r1 < 0:
            continue
        bd, bi = 256, -1
        for ix in range(c0, c1 + 1):
            for iy in range(r0, r1 + 1):
                for k in grid.get((ix, iy), ()):
                    kx, ky, ko = float(keys["x"][k]), float(keys["y"][k]), int(keys["octave"][k])
                    if not (abs(kx - u) < r and abs(ky - v) < r):
                        continue
                    if ko < level - 1 or ko > level:
                        continue
                    e2 = (u - kx) ** 2 + (v - ky) ** 2
                    if u_right[k] >= 0:
                        if (e2 + (ur - float(u_right[k])) ** 2) * float(inv_sigma2[ko]) > 7.8:
                            continue
                    elif e2 * float(inv_sigma2[ko]) > 5.99:
                        continue
                    d = hamming(P["descriptor"], desc[k])
                    if d < bd:
                        bd, bi = d, k
        if bi < 0:
            continue                                   # vIndices empty, or no keypoint passed the gates: bestDist stays 256
        best_dist[i] = bd
        if bd <= TH_LOW:
            best_idx[i] = bi
    return int((best_idx >= 0).sum()), best_idx, best_dist

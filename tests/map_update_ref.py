"""Restatement in numpy float32 of the two map updates of IMU initialisation, written from the reference's source:
Map::ApplyScaledRotation (SF/src/Map.cc:256-287) with KeyFrame::SetPose (SF/src/KeyFrame.cc:121-134) and MapPoint::UpdateNormalAndDepth
(SF/src/MapPoint.cc:444-503), and the map update after a global BA (SF/src/LocalMapping.cc:1346-1425).  Every operation is one float32
operation of numpy, so every intermediate is rounded; the Sophus operations are spelt out as so3.hpp / se3.hpp write them.  Where Eigen
leaves a summation order to its build the order is the one include/tc2li_hip.h states.  A quaternion is a tuple (x, y, z, w) and a vector a
tuple of three, of float32 scalars or of float32 arrays (then the operation runs over all rows at once)."""
import numpy as np

F = np.float32
ONE, TWO, MINUS_ONE = F(1), F(2), F(-1)


# ---- Sophus / Eigen -------------------------------------------------------------------------------------------------------------------
def normalize(q):
    """SO3::normalize: length = norm(), coefficients /= length"""
    x, y, z, w = q
    length = np.sqrt(x * x + y * y + z * z + w * w)
    return (x / length, y / length, z / length, w / length)


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def so3_point(q, p):
    """SO3 * point (so3.hpp:358-367)"""
    vec, w = q[:3], q[3]
    uv = cross(vec, p)
    uv = tuple(c + c for c in uv)
    c2 = cross(vec, uv)
    return tuple(p[i] + w * uv[i] + c2[i] for i in range(3))


def so3_inverse(q):
    """SO3::inverse: SO3(unit_quaternion().conjugate()); the constructor normalises"""
    x, y, z, w = q
    return normalize((-x, -y, -z, w))


def so3_so3(a, b):
    """SO3 * SO3 (so3.hpp:325-339): the product goes through the SO3(Quaternion) constructor"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return normalize((aw * bx + ax * bw + ay * bz - az * by,
                      aw * by + ay * bw + az * bx - ax * bz,
                      aw * bz + az * bw + ax * by - ay * bx,
                      aw * bw - ax * bx - ay * by - az * bz))


def se3_inverse(T):
    """se3.hpp:208-211: invR = so3().inverse(); SE3(invR, invR * (translation() * -1))"""
    q, t = T
    inv = so3_inverse(q)
    return inv, so3_point(inv, tuple(c * MINUS_ONE for c in t))


def se3_se3(A, B):
    """se3.hpp:304-308: SE3(so3() * other.so3(), translation() + so3() * other.translation())"""
    r = so3_point(A[0], B[1])
    return so3_so3(A[0], B[0]), tuple(A[1][i] + r[i] for i in range(3))


def se3_point(T, p):
    """se3.hpp: so3() * p + translation()"""
    r = so3_point(T[0], p)
    return tuple(r[i] + T[1][i] for i in range(3))


def rotation_matrix(q):
    """Eigen QuaternionBase::toRotationMatrix -> rows of three"""
    x, y, z, w = q
    tx, ty, tz = TWO * x, TWO * y, TWO * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return ((ONE - (tyy + tzz), txy - twz, txz + twy), (txy + twz, ONE - (txx + tzz), tyz - twx), (txz - twy, tyz + twx, ONE - (txx + tyy)))


def mat_vec(M, v):
    """a row sum is ((a*x + b*y) + c*z)"""
    return tuple((M[r][0] * v[0] + M[r][1] * v[1]) + M[r][2] * v[2] for r in range(3))


def norm(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def pose_of(a):
    """[..., 7] -> ((x, y, z, w), (tx, ty, tz))"""
    a = np.asarray(a, F)
    return tuple(a[..., i] for i in range(4)), tuple(a[..., 4 + i] for i in range(3))


def pose7(T):
    return np.stack([np.asarray(c, F) for c in T[0] + T[1]], axis=-1)


def vec_of(a):
    a = np.asarray(a, F)
    return tuple(a[..., i] for i in range(3))


def filled(shape, dtype, fill):
    a = np.empty(shape, dtype)
    a.view(np.uint8)[...] = fill
    return a


# ---- Map::ApplyScaledRotation ---------------------------------------------------------------------------------------------------------
def apply_scaled_rotation(p, fill=0):
    nk, npts = len(np.asarray(p["kf_pose7"]).reshape(-1, 7)), len(np.asarray(p["point_pos"]).reshape(-1, 3))
    s = F(p["s"])
    Tyw = pose_of(np.asarray(p["T7"], F))
    Ryw, tyw = rotation_matrix(Tyw[0]), Tyw[1]
    out = dict(kf_imu_pos_out=filled((nk, 3), F, fill), point_normal=filled((npts, 3), F, fill), point_min_distance=filled(npts, F, fill),
               point_max_distance=filled(npts, F, fill))
    with np.errstate(all="ignore"):
        # the keyframes, all rows at once (Map.cc:265-278)
        Tcw = pose_of(np.asarray(p["kf_pose7"], F).reshape(-1, 7))
        Twc = se3_inverse(Tcw)                                                           # GetPoseInverse(): mTwc of the last SetPose
        Twc = (Twc[0], tuple(c * s for c in Twc[1]))                                     # Twc.translation() *= s
        Tyc = se3_se3(Tyw, Twc)
        Tcy = se3_inverse(Tyc)
        new_Twc = se3_inverse(Tcy)                                                       # SetPose: mTwc = mTcw.inverse()
        out["kf_pose7_out"] = pose7(Tcy).reshape(nk, 7)
        out["kf_inv_pose7_out"] = pose7(new_Twc).reshape(nk, 7)
        if p.get("has_tcb", 0):                                                          # mOwb = mRwc * mTcb.translation() + mTwc.translation()
            r = mat_vec(rotation_matrix(new_Twc[0]), tuple(F(v) for v in p["tcb3"]))
            out["kf_imu_pos_out"] = np.stack([r[i] + new_Twc[1][i] for i in range(3)], axis=-1).astype(F).reshape(nk, 3)
        v = mat_vec(Ryw, vec_of(np.asarray(p["kf_vel"], F).reshape(-1, 3)))              # Ryw * Vw, * s with bScaledVel
        if p.get("scaled_vel", 0):
            v = tuple(c * s for c in v)
        out["kf_vel_out"] = np.stack(v, axis=-1).astype(F).reshape(nk, 3)
        # the points (:279-285): SetWorldPos(s * Ryw * pos + tyw) whatever the bad flag says
        M = tuple(tuple(s * Ryw[r][c] for c in range(3)) for r in range(3))
        x = mat_vec(M, vec_of(np.asarray(p["point_pos"], F).reshape(-1, 3)))
        pos = np.stack([x[r] + tyw[r] for r in range(3)], axis=-1).astype(F).reshape(npts, 3)
        out["point_pos_out"] = pos
        # UpdateNormalAndDepth, point by point, observation by observation
        centre = out["kf_inv_pose7_out"][:, 4:7]
        off, obs_kf, bad = np.asarray(p["obs_offsets"]), np.asarray(p["obs_kf"]), np.asarray(p["point_bad"])
        last = F(p["last_level_scale"])
        for i in range(npts):
            if bad[i]:                                                                   # MapPoint.cc:450
                continue
            kfs = obs_kf[off[i]:off[i + 1]]
            if len(kfs) == 0:                                                            # :458
                continue
            P = vec_of(pos[i])
            normal = (F(0), F(0), F(0))
            n = 0
            for kf in kfs:                                                               # :463-483, left index only
                ni = tuple(P[c] - centre[kf, c] for c in range(3))
                d = norm(ni)
                normal = tuple(normal[c] + ni[c] / d for c in range(3))
                n += 1
            ref = int(p["point_ref_kf"][i])
            dist = norm(tuple(P[c] - centre[ref, c] for c in range(3)))                  # :485-486
            mx = dist * F(p["point_ref_level_scale"][i])                                 # :499
            out["point_max_distance"][i] = mx
            out["point_min_distance"][i] = mx / last                                     # :500
            out["point_normal"][i] = [normal[c] / F(n) for c in range(3)]                # :501
    return out


# ---- the map update after a global BA -----------------------------------------------------------------------------------------------------
def gba_map_correction(p):
    """LocalMapping.cc:1346-1425 on objects, with the reference's list and pop_front"""
    n = len(p["kf_parent"])
    kfs = []
    for k in range(n):
        kfs.append(dict(Tcw=pose_of(p["kf_pose7"][k]), TcwGBA=pose_of(p["kf_gba_pose7"][k]), TcwBefGBA=pose_of(p["kf_bef_gba_pose7"][k]),
                        V=vec_of(p["kf_vel"][k]), VwbGBA=vec_of(p["kf_gba_vel"][k]), bias=np.asarray(p["kf_bias"][k], F).copy(),
                        BiasGBA=np.asarray(p["kf_gba_bias"][k], F).copy(), in_gba=bool(p["kf_in_gba"][k]), childs=[], visited=0))
        kfs[k]["Twc"] = None
    for k in range(n):
        if p["kf_parent"][k] >= 0:
            kfs[int(p["kf_parent"][k])]["childs"].append(k)
    with np.errstate(all="ignore"):
        for kf in kfs:
            kf["Twc"] = se3_inverse(kf["Tcw"])                                           # what the last SetPose left
        to_check = [k for k in range(n) if p["kf_origin"][k]]                            # :1347
        while to_check:
            KF = kfs[to_check[0]]
            Twc = KF["Twc"]                                                              # :1353
            for c in KF["childs"]:
                child = kfs[c]
                if p["kf_bad"][c]:                                                       # :1356
                    continue
                if not child["in_gba"]:                                                  # :1359
                    Tchildc = se3_se3(child["Tcw"], Twc)
                    child["TcwGBA"] = se3_se3(Tchildc, KF["TcwGBA"])
                    Rcor = so3_so3(so3_inverse(child["TcwGBA"][0]), child["Tcw"][0])
                    if p["kf_vel_set"][c]:
                        child["VwbGBA"] = so3_point(Rcor, child["V"])
                    child["BiasGBA"] = child["bias"].copy()
                    child["in_gba"] = True
                to_check.append(c)
            KF["TcwBefGBA"] = KF["Tcw"]                                                  # :1379
            KF["Tcw"] = KF["TcwGBA"]                                                     # SetPose(mTcwGBA)
            KF["Twc"] = se3_inverse(KF["Tcw"])
            if p["kf_imu"][to_check[0]]:                                                 # :1382-1388
                KF["V"] = KF["VwbGBA"]
                KF["bias"] = KF["BiasGBA"].copy()
            KF["visited"] += 1
            to_check.pop(0)
        npts = len(p["point_bad"])
        pos_out = np.asarray(p["point_pos"], F).reshape(npts, 3).copy()
        moved = np.zeros(npts, np.uint8)
        for i in range(npts):
            if p["point_bad"][i]:                                                        # :1403
                continue
            if p["point_in_gba"][i]:                                                     # :1406-1410
                pos_out[i] = p["point_gba_pos"][i]
                moved[i] = 1
                continue
            ref = kfs[int(p["point_ref_kf"][i])]
            if not ref["in_gba"]:                                                        # :1416
                continue
            Xc = se3_point(ref["TcwBefGBA"], vec_of(pos_out[i]))                         # :1420
            pos_out[i] = se3_point(ref["Twc"], Xc)                                       # :1423
            moved[i] = 2
    assert all(kf["visited"] <= 1 for kf in kfs)
    return dict(kf_visited=np.array([kf["visited"] for kf in kfs], np.uint8), kf_in_gba_out=np.array([kf["in_gba"] for kf in kfs], np.uint8),
                kf_pose7_out=np.array([pose7(kf["Tcw"]) for kf in kfs], F).reshape(n, 7),
                kf_bef_gba_pose7_out=np.array([pose7(kf["TcwBefGBA"]) for kf in kfs], F).reshape(n, 7),
                kf_vel_out=np.array([np.stack(kf["V"]) for kf in kfs], F).reshape(n, 3),
                kf_bias_out=np.array([kf["bias"] for kf in kfs], F).reshape(n, 6), point_pos_out=pos_out, point_moved=moved)

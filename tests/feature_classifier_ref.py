"""CPU restatement of Preprocess::velodyne_handler's feature branch (SF/include/lidar_front_end/preprocess.cpp:100-143) with
give_feature (:169-482), plane_judge (:484-584) and edge_jump_judge (:586-623): the checker of the device classifier.

Test infrastructure only.  Float where the reference computes in float (np.float32), double elsewhere (Python floats); sums left to
right as written.  Eigen's norm / dot / normalize on Vector3d are ((a0*b0 + a1*b1) + a2*b2) and / sqrt.
"""
import math

import numpy as np

# Feature (preprocess.h:40), E_jump (:42)
NOR, POSS_PLANE, REAL_PLANE, EDGE_JUMP, EDGE_PLANE, WIRE = range(6)
NR_NOR, NR_ZERO, NR_180, NR_INF, NR_BLIND = range(5)

# Preprocess::Preprocess (:32-58).  disA is assigned twice (0.01, then 0.1); disB never (a parameter here, default 0.0).
GROUP_SIZE = 8
DIS_A = 0.1
P2L_RATIO = 225.0
LIMIT_MAXMIN = 3.24
INF_BOUND = 10.0
EDGE_A = 2.0
EDGE_B = 0.1
SMALLP_RATIO = 1.2
JUMP_UP_LIMIT = math.cos(170.0 / 180 * math.pi)
JUMP_DOWN_LIMIT = math.cos(8.0 / 180 * math.pi)
COS160 = math.cos(160.0 / 180 * math.pi)
SMALLP_INTERSECT = math.cos(172.5 / 180 * math.pi)

F32 = np.float32
# velodyne_ros::Point as the library lays it out (tc2li_velodyne_point, 32 B)
VELODYNE_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("intensity", "<f4"),
                           ("time", "<f4"), ("ring", "<u2"), ("pad1", "<u2"), ("pad2", "<f4")])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _norm(a):
    return math.sqrt(_dot(a, a))


def _div(a, b):
    """IEEE double division (b may be 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


class _Line:
    """pl_buff[j] and typess[j] of one line."""

    def __init__(self, x, y, z, intensity, curvature):
        self.x, self.y, self.z = x, y, z  # np.float32 arrays
        self.intensity, self.curvature = intensity, curvature
        n = len(x)
        self.n = n
        # :133-141 -- range: std::sqrt(float), widened; dista: float differences in the double members vx, vy, vz
        self.range = [float(r) for r in np.sqrt(x * x + y * y)]
        dx, dy, dz = (x[:-1] - x[1:]).astype(np.float64), (y[:-1] - y[1:]).astype(np.float64), (z[:-1] - z[1:]).astype(np.float64)
        d = (dx * dx + dy * dy) + dz * dz
        # the last point's dista is never written (orgtype() does not set it), yet plane_judge can push it into disarr: 0.0 here
        self.dista = [float(v) for v in d] + [0.0]
        self.ftype = [NOR] * n
        self.intersect = [2.0] * n
        self.xf = [float(v) for v in x]  # widened copies for the double arithmetic
        self.yf = [float(v) for v in y]
        self.zf = [float(v) for v in z]

    def fdiff(self, a, b):
        """(pl[a] - pl[b]) per axis in float, widened."""
        return (float(self.x[a] - self.x[b]), float(self.y[a] - self.y[b]), float(self.z[a] - self.z[b]))


def plane_judge(L, i_cur, blind, dis_b):
    """:484-584 -> (plane_type, i_nex, curr_direct)."""
    group_dis = DIS_A * L.range[i_cur] + dis_b
    group_dis = group_dis * group_dis
    disarr = []
    i_nex = i_cur
    while i_nex < i_cur + GROUP_SIZE:
        if L.range[i_nex] < blind:
            return 2, i_nex, (0.0, 0.0, 0.0)
        disarr.append(L.dista[i_nex])
        i_nex += 1
    vx = vy = vz = two_dis = None
    while True:
        if i_cur >= L.n or i_nex >= L.n:
            break
        if L.range[i_nex] < blind:
            return 2, i_nex, (0.0, 0.0, 0.0)
        vx, vy, vz = L.fdiff(i_nex, i_cur)
        two_dis = vx * vx + vy * vy + vz * vz
        if two_dis >= group_dis:
            break
        disarr.append(L.dista[i_nex])
        i_nex += 1
    leng_wid = 0.0
    for j in range(i_cur + 1, i_nex):
        if j >= L.n or i_cur >= L.n:
            break
        v1 = L.fdiff(j, i_cur)
        v2 = (v1[1] * vz - vy * v1[2], v1[2] * vx - v1[0] * vz, v1[0] * vy - vx * v1[1])
        lw = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2]
        if lw > leng_wid:
            leng_wid = lw
    if _div(two_dis * two_dis, leng_wid) < P2L_RATIO:  # leng_wid 0: inf or NaN, both fail
        return 0, i_nex, (0.0, 0.0, 0.0)
    # the descending bubble sort (:553-564): disarr[0] is the maximum, disarr[size - 2] the second-smallest element
    srt = sorted(disarr)
    if srt[1] < 1e-16:
        return 0, i_nex, (0.0, 0.0, 0.0)
    if srt[-1] / srt[1] >= LIMIT_MAXMIN:
        return 0, i_nex, (0.0, 0.0, 0.0)
    cd = (vx, vy, vz)
    sq = _dot(cd, cd)
    if sq > 0:
        nrm = math.sqrt(sq)
        cd = (vx / nrm, vy / nrm, vz / nrm)
    return 1, i_nex, cd


def edge_jump_judge(L, i, nor_dir, blind):
    """:586-623."""
    if nor_dir == 0:
        if L.range[i - 1] < blind or L.range[i - 2] < blind:
            return False
    else:
        if L.range[i + 1] < blind or L.range[i + 2] < blind:
            return False
    d1 = L.dista[i + nor_dir - 1]
    d2 = L.dista[i + 3 * nor_dir - 2]
    if d1 < d2:
        d1, d2 = d2, d1
    d1 = math.sqrt(d1)
    d2 = math.sqrt(d2)
    return not (d1 > EDGE_A * d2 or (d1 - d2) > EDGE_B)


def give_feature(L, blind, dis_b):
    """Passes 1-3 of :169-429 on one line; returns head."""
    n = L.n
    head = 0
    while head < n and L.range[head] < blind:  # :180, stopped at the line's end (the reference reads past it)
        head += 1
    # pass 1, planes (:186-293)
    plsize2 = n - GROUP_SIZE if n > GROUP_SIZE else 0
    last_direct = (0.0, 0.0, 0.0)
    last_state = 0
    i = head
    while i < plsize2:
        if L.range[i] < blind:
            i += 1
            continue
        plane_type, i_nex, curr_direct = plane_judge(L, i, blind, dis_b)
        if plane_type == 1:
            for j in range(i, i_nex + 1):
                if j >= n:  # a walk that reached the line's end: the reference writes types[n], out of bounds
                    break
                L.ftype[j] = REAL_PLANE if (j != i and j != i_nex) else POSS_PLANE
            if last_state == 1 and _norm(last_direct) > 0.1:
                mod = _dot(last_direct, curr_direct)
                L.ftype[i] = EDGE_PLANE if (-0.707 < mod < 0.707) else REAL_PLANE
            i = i_nex - 1
            last_state = 1
        else:
            i = i_nex
            last_state = 0
        last_direct = curr_direct
        i += 1
    # pass 2, edges (:295-389)
    for i in range(head + 3, n - 3 if n > 3 else 0):
        if L.range[i] < blind or L.ftype[i] >= REAL_PLANE:
            continue
        if L.dista[i - 1] < 1e-16 or L.dista[i] < 1e-16:
            continue
        vec_a = (L.xf[i], L.yf[i], L.zf[i])
        vecs = [None, None]
        edj = [NR_NOR, NR_NOR]
        for j in range(2):
            m = 1 if j == 1 else -1
            if L.range[i + m] < blind:
                edj[j] = NR_INF if L.range[i] > INF_BOUND else NR_BLIND
                continue
            vecs[j] = (L.xf[i + m] - vec_a[0], L.yf[i + m] - vec_a[1], L.zf[i + m] - vec_a[2])
            angle = _div(_div(_dot(vec_a, vecs[j]), _norm(vec_a)), _norm(vecs[j]))
            if angle < JUMP_UP_LIMIT:
                edj[j] = NR_180
            elif angle > JUMP_DOWN_LIMIT:
                edj[j] = NR_ZERO
        # with a blind neighbour the reference computes it from an unset vector; nothing reads it then
        if vecs[0] is not None and vecs[1] is not None:
            L.intersect[i] = _div(_div(_dot(vecs[0], vecs[1]), _norm(vecs[0])), _norm(vecs[1]))
        it, d = L.intersect[i], L.dista
        if edj[0] == NR_NOR and edj[1] == NR_ZERO and d[i] > 0.0225 and d[i] > 4 * d[i - 1]:
            if it > COS160 and edge_jump_judge(L, i, 0, blind):
                L.ftype[i] = EDGE_JUMP
        elif edj[0] == NR_ZERO and edj[1] == NR_NOR and d[i - 1] > 0.0225 and d[i - 1] > 4 * d[i]:
            if it > COS160 and edge_jump_judge(L, i, 1, blind):
                L.ftype[i] = EDGE_JUMP
        elif edj[0] == NR_NOR and edj[1] == NR_INF:
            if edge_jump_judge(L, i, 0, blind):
                L.ftype[i] = EDGE_JUMP
        elif edj[0] == NR_INF and edj[1] == NR_NOR:
            if edge_jump_judge(L, i, 1, blind):
                L.ftype[i] = EDGE_JUMP
        elif edj[0] > NR_NOR and edj[1] > NR_NOR:
            if L.ftype[i] == NOR:
                L.ftype[i] = WIRE
    # pass 3, small planes (:391-429), in order: a point relabelled by its predecessor is skipped
    for i in range(head + 1, n - 1):
        if L.range[i] < blind or L.range[i - 1] < blind or L.range[i + 1] < blind:
            continue
        if L.dista[i - 1] < 1e-8 or L.dista[i] < 1e-8:
            continue
        if L.ftype[i] == NOR:
            if L.dista[i - 1] > L.dista[i]:
                ratio = L.dista[i - 1] / L.dista[i]
            else:
                ratio = L.dista[i] / L.dista[i - 1]
            if L.intersect[i] < SMALLP_INTERSECT and ratio < SMALLP_RATIO:
                if L.ftype[i - 1] == NOR:
                    L.ftype[i - 1] = REAL_PLANE
                if L.ftype[i + 1] == NOR:
                    L.ftype[i + 1] = REAL_PLANE
                L.ftype[i] = REAL_PLANE
    return head


def _point(x, y, z, intensity, curvature):
    return (x, y, z, 1.0, 0.0, 0.0, 0.0, 0.0, intensity, curvature, 0.0, 0.0)  # PCL_ADD_POINT4D's data[3] = 1


def emit(L, head, point_filter_num, surf, corn):
    """Pass 4 (:431-482)."""
    last_surface = -1
    for j in range(head, L.n):
        ft = L.ftype[j]
        if ft == POSS_PLANE or ft == REAL_PLANE:
            if last_surface == -1:
                last_surface = j
            if j == last_surface + point_filter_num - 1:
                surf.append(_point(L.x[j], L.y[j], L.z[j], L.intensity[j], L.curvature[j]))
                last_surface = -1
        else:
            if ft == EDGE_JUMP or ft == EDGE_PLANE:
                corn.append(_point(L.x[j], L.y[j], L.z[j], L.intensity[j], L.curvature[j]))
            if last_surface != -1:
                acc = [F32(0.0)] * 5  # PointXYZINormal ap: zeros, summed in float in line order
                for k in range(last_surface, j):
                    acc[0] = F32(acc[0] + L.x[k])
                    acc[1] = F32(acc[1] + L.y[k])
                    acc[2] = F32(acc[2] + L.z[k])
                    acc[3] = F32(acc[3] + L.intensity[k])
                    acc[4] = F32(acc[4] + L.curvature[k])
                cnt = F32(j - last_surface)
                surf.append(_point(*[F32(a / cnt) for a in acc]))
            last_surface = -1


def classify(raw, n_lines=64, point_filter_num=1, blind=0.01, time_unit_scale=1e-3, dis_b=0.0):
    """velodyne_handler with feature_enabled (:100-143) on a structured array of velodyne_ros::Point ->
    (pl_surf, pl_corn as records of POINT_DTYPE's 12 float32 fields, labels uint8 in line order, line offsets int32 [n_lines + 1])."""
    raw = np.asarray(raw)
    ring = raw["ring"].astype(np.int64)
    tus = F32(time_unit_scale)
    surf, corn, labels = [], [], []
    offsets = [0]
    for j in range(n_lines):
        sel = np.nonzero(ring == j)[0]  # `if (layer >= N_SCANS) continue;` -- the rest in input order
        x, y, z = (raw[f][sel].astype(np.float32) for f in ("x", "y", "z"))
        intensity = raw["intensity"][sel].astype(np.float32)
        curvature = (raw["time"][sel].astype(np.float32) * tus).astype(np.float32)
        n = len(sel)
        offsets.append(offsets[-1] + n)
        if n < 2:  # `if (linesize < 2) continue;`
            labels.extend([NOR] * n)
            continue
        L = _Line(x, y, z, intensity, curvature)
        head = give_feature(L, blind, dis_b)
        emit(L, head, point_filter_num, surf, corn)
        labels.extend(L.ftype)

    def arr(rows):
        return np.array(rows, np.float32).reshape(-1, 12)

    return arr(surf), arr(corn), np.array(labels, np.uint8), np.array(offsets, np.int32)


def make_raw(points, ring=0, time=None):
    """A structured velodyne_ros::Point array from [n, 3] positions (intensity = index, time = index unless given)."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), VELODYNE_DTYPE)
    out["x"], out["y"], out["z"] = pts[:, 0], pts[:, 1], pts[:, 2]
    out["intensity"] = np.arange(len(pts), dtype=np.float32)
    out["time"] = np.arange(len(pts), dtype=np.float32) if time is None else time
    out["ring"] = ring
    return out

"""MLPnPsolver of the reference (SF/src/MLPnPsolver.cpp, SF/include/MLPnPsolver.h) restated in numpy, function by function, float32
where the reference is float.  It is the checker of tc2li_mlpnp_ransac_batch / tc2li_host_mlpnp_ransac_batch.

The rand() values are an input (``draws``): DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) is a pure function of
rand()'s return value, and nothing else in the solver is random.

Three things are CHOICES here, because the reference leaves them to Eigen and Eigen is not restated:

* the null-space basis of a bearing vector (:351-353 take columns 1, 2 of the V of a 1 x 3 JacobiSVD: some orthonormal basis of the
  complement).  ``basis=0``: the first two columns of the Householder reflection that maps f / |f| to -e3 (what the library uses);
  ``basis=1``: rows 1, 2 of numpy's SVD of the 1 x 3 matrix.  A^T A, J^T J and J^T r do not depend on the basis; the Gauss-Newton stop test
  max |J dx| < 1e-5 does, slightly.
* the sign of singular vectors and eigenvectors.  Here every such vector is normalised so that its entry of largest magnitude is
  positive, then multiplied by the matching entry of ``signs`` = (eigenvector 0, 1, 2 of the planar frame, result1).  The non-planar
  branch does not depend on the sign of result1: R = U V^T is negated back by the determinant test and both signs of t are tried.  The
  planar branch does depend on it (the cross product in tmp's first row keeps its sign when the other two rows flip, so the four
  candidate poses differ) and on the signs of the planar frame; ``SIGN_CHOICES`` enumerates them and a result equal to any passes.
* FullPivHouseholderQR's rank rule (:362, :369), restated in ``fullpiv_rank``: pivot = the entry of largest magnitude of the remaining
  corner, rows and columns swapped, one Householder reflection per column, stop at a corner <= epsilon * 3 * the first pivot, rank = the
  number of diagonal entries above epsilon * 3 * |largest pivot|.

``evec`` selects how the eigenvector of A^T A for the smallest singular value is found: "svd" (numpy's SVD, the reference's route
:503-504) or "eigh".  ``jac`` selects the analytic Jacobian (derived, see ``residuals_and_jacs``) or central differences.  The spread of
the results between these variants is the yardstick of the tests' tolerances.
"""
import itertools
import math

import numpy as np

F32 = np.float32
EPS = np.finfo(np.float64).eps
SIGN_CHOICES = [s for s in itertools.product((1.0, -1.0), repeat=4)]
REFERENCE_PARAMS = dict(probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, th2=5.991)   # Tracking.cc:3526


def random_int(r, lo, hi):
    """DUtils::Random::RandomInt (Random.cpp:47-50), RAND_MAX = 2^31 - 1"""
    d = hi - lo + 1
    return int((float(r) / (2147483647.0 + 1.0)) * d) + lo


def ransac_parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5, th2=5.991):
    """SetRansacParameters (:205-240) -> (mRansacMinInliers, mRansacMaxIts)"""
    eps = F32(epsilon)
    n_min = int(F32(N) * eps)                                        # :217 int times float, truncated
    n_min = max(n_min, min_inliers, min_set)                         # :218-221
    if N > 0 and eps < F32(n_min) / F32(N):                          # :224-225
        eps = F32(n_min) / F32(N)
    if n_min == N or N <= 0:                                         # :230-231
        n_it = 1
    else:
        arg = 1 - math.pow(float(eps), 3)
        # N < min_inliers: the logarithm of a negative number; the reference's int conversion of NaN is INT_MIN on x86-64 -> 1 after :235
        n_it = 1 if arg <= 0 else int(math.ceil(math.log(1 - probability) / math.log(arg)))   # :233
    return n_min, max(1, min(n_it, max_iterations))                  # :235


def fix_sign(v):
    k = int(np.argmax(np.abs(v)))
    return -v if v[k] < 0 else v


def null_space(f, basis=0):
    """:351-353 -> (r, s), an orthonormal basis of the complement of f"""
    if basis == 0:
        v = f / math.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
        v = np.array([v[0], v[1], v[2] + 1.0])
        k = 2.0 / (v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
        H = np.eye(3) - k * np.outer(v, v)
        return H[:, 0].copy(), H[:, 1].copy()
    Vt = np.linalg.svd(f[None, :])[2]
    return Vt[1].copy(), Vt[2].copy()


def fullpiv_rank(M):
    """FullPivHouseholderQR<Matrix3d>(M).rank() with the default threshold"""
    Q = np.array(M, np.float64)
    n = Q.shape[0]
    precision = EPS * n
    nonzero, maxpivot, biggest = n, 0.0, 0.0
    for k in range(n):
        corner = np.abs(Q[k:, k:])
        big, br, bc = -1.0, k, k
        for c in range(corner.shape[1]):            # column-major scan, the first of the largest
            for r in range(corner.shape[0]):
                if corner[r, c] > big:
                    big, br, bc = corner[r, c], r + k, c + k
        if k == 0:
            biggest = big
        if abs(big) <= abs(biggest) * precision:
            nonzero = k
            break
        Q[[k, br], k:] = Q[[br, k], k:]
        Q[:, [k, bc]] = Q[:, [bc, k]]
        c0 = Q[k, k]
        tail = float(np.sum(Q[k + 1:, k] ** 2))
        if tail <= np.finfo(np.float64).tiny:
            tau, beta = 0.0, c0
            Q[k + 1:, k] = 0.0
        else:
            beta = math.sqrt(c0 * c0 + tail)
            if c0 >= 0:
                beta = -beta
            Q[k + 1:, k] = Q[k + 1:, k] / (c0 - beta)
            tau = (beta - c0) / beta
        Q[k, k] = beta
        maxpivot = max(maxpivot, abs(beta))
        ess = Q[k + 1:, k].copy()
        for c in range(k + 1, n):
            w = Q[k, c] + float(ess @ Q[k + 1:, c])
            Q[k, c] -= tau * w
            Q[k + 1:, c] -= tau * w * ess
    return sum(1 for i in range(nonzero) if abs(Q[i, i]) > maxpivot * precision)


def rodrigues2rot(w):
    """:640-655"""
    R = np.eye(3)
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    th = math.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if th > EPS:
        R = R + math.sin(th) / th * K + (1 - math.cos(th)) / (th * th) * (K @ K)
    return R


def rot2rodrigues(R):
    """:657-672"""
    w = np.zeros(3)
    trace = R[0, 0] + R[1, 1] + R[2, 2] - 1.0
    c = trace / 2.0
    wnorm = math.acos(c) if -1.0 <= c <= 1.0 else float("nan")
    if wnorm > EPS:
        w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) * (wnorm / (2.0 * math.sin(wnorm)))
    return w


def residuals(x, pts, nulls):
    """mlpnp_residuals_and_jacs (:740-786) without the Jacobian"""
    R = rodrigues2rot(x[:3])
    r = np.zeros(2 * len(pts))
    for i, X in enumerate(pts):
        p = R @ X + x[3:]
        p = p / math.sqrt(p @ p)
        r[2 * i] = nulls[i][0] @ p
        r[2 * i + 1] = nulls[i][1] @ p
    return r


def residuals_and_jacs(x, pts, nulls, jac="analytic"):
    """mlpnp_residuals_and_jacs with mlpnpJacs (:788-1036) derived instead of transcribed: res = n^T p / |p|, p = R(w) X + t, so
    d res / dt = n^T (I - u u^T) / |p| with u = p / |p|, and d res / dw_k is that row times d(R(w) X) / dw_k of
    R = I + a K + b K^2, a = sin th / th, b = (1 - cos th) / th^2 (K X = w x X, K^2 X = w (w.X) - th^2 X).  At |w| <= epsilon the limit
    e_k x X is taken (the reference's generated expression divides by zero there)."""
    r = residuals(x, pts, nulls)
    J = np.zeros((2 * len(pts), 6))
    if jac == "fd":
        for k in range(6):
            h = 1e-6
            d = np.zeros(6); d[k] = h
            J[:, k] = (residuals(x + d, pts, nulls) - residuals(x - d, pts, nulls)) / (2 * h)
        return r, J
    w, t = x[:3], x[3:]
    R = rodrigues2rot(w)
    th2 = float(w @ w)
    th = math.sqrt(th2)
    small = not th > EPS
    if not small:
        s, c = math.sin(th), math.cos(th)
        a, b = s / th, (1 - c) / th2
        da, db = (th * c - s) / (th2 * th), (th * s - 2 * (1 - c)) / (th2 * th2)
    for i, X in enumerate(pts):
        p = R @ X + t
        n = math.sqrt(p @ p)
        u = p / n
        D = np.zeros((3, 3))        # column k = d(R X) / dw_k
        for k in range(3):
            e = np.zeros(3); e[k] = 1.0
            if small:
                D[:, k] = np.cross(e, X)
            else:
                D[:, k] = (da * w[k] * np.cross(w, X) + a * np.cross(e, X) + db * w[k] * (w * (w @ X) - th2 * X)
                           + b * (e * (w @ X) + w * X[k] - 2.0 * w[k] * X))
        for j in range(2):
            g = (nulls[i][j] - (nulls[i][j] @ u) * u) / n
            J[2 * i + j, :3] = g @ D
            J[2 * i + j, 3:] = g
    return r, J


def mlpnp_gn(x, pts, nulls, jac="analytic"):
    """:674-738"""
    x = x.copy()
    for _ in range(5):
        r, J = residuals_and_jacs(x, pts, nulls, jac)
        A = J.T @ J
        g = J.T @ r
        try:
            dx = np.linalg.solve(A, g)          # :720-721 LDLT
        except np.linalg.LinAlgError:
            dx = np.full(6, np.nan)
        if np.abs(dx).max() > 5.0 or np.abs(dx).min() > 1.0:      # :724
            break
        dl = J @ dx
        x = x - dx                                                # :730 / :733
        if np.abs(dl).max() < 1e-5:                               # :728
            break
    return x


def compute_pose(f, p, evec="svd", basis=0, jac="analytic", signs=(1.0, 1.0, 1.0, 1.0)):
    """computePose (:336-638) without covariances -> ([R | t] 3 x 4, planar)"""
    n = len(p)
    nulls = [null_space(f[i], basis) for i in range(n)]
    points3 = np.array(p, np.float64).T.copy()
    planar_test = points3 @ points3.T                              # :361
    planar = fullpiv_rank(planar_test) == 2                        # :362, :369
    eigen_rot = np.eye(3)
    if planar:
        _, vec = np.linalg.eigh(planar_test)                       # :374 ascending
        eigen_rot = np.array([fix_sign(vec[:, k]) * signs[k] for k in range(3)])   # :375-376 transposed
        points3 = eigen_rot @ points3
    cols = 9 if planar else 12
    A = np.zeros((2 * n, cols))
    for i in range(n):
        X = points3[:, i]
        for j in range(2):
            nv = nulls[i][j]
            if planar:                                             # :420-450
                A[2 * i + j, :6] = np.outer(nv, X[1:]).ravel()
                A[2 * i + j, 6:] = nv
            else:                                                  # :452-491
                A[2 * i + j, :9] = np.outer(nv, X).ravel()
                A[2 * i + j, 9:] = nv
    AtA = A.T @ A                                                  # :501
    if evec == "svd":
        res = np.linalg.svd(AtA)[2][cols - 1]                      # :503-504
    else:
        res = np.linalg.eigh(AtA)[1][:, 0]
    res = fix_sign(res) * signs[3]
    pts = [np.array(q, np.float64) for q in p]

    def direction_error(R, t):
        e = 0.0
        for k in range(6):
            v = R @ pts[k] + t
            v = v / math.sqrt(v @ v)
            e += 1.0 - v @ f[k]
        return e

    if planar:                                                     # :514-573
        tmp = np.array([[0.0, res[0], res[1]], [0.0, res[2], res[3]], [0.0, res[4], res[5]]])
        tmp[:, 0] = np.cross(tmp[:, 1], tmp[:, 2])
        tmp = tmp.T.copy()
        scale = 1.0 / math.sqrt(abs(math.sqrt(tmp[:, 1] @ tmp[:, 1]) * math.sqrt(tmp[:, 2] @ tmp[:, 2])))
        U, _, Vt = np.linalg.svd(tmp)
        R1 = U @ Vt
        if np.linalg.det(R1) < 0:
            R1 = -R1
        R1 = eigen_rot.T @ R1
        t = scale * res[6:9]
        R1 = -R1.T
        if np.linalg.det(R1) < 0:
            R1[:, 2] *= -1
        R2 = R1.copy(); R2[:, 0] *= -1; R2[:, 1] *= -1
        Ts = [(R1, t), (R1, -t), (R2, t), (R2, -t)]
        errs = [direction_error(R, tt) for R, tt in Ts]
        Rout, tout = Ts[int(np.argmin(errs))]                      # min_element: the first of the smallest
    else:                                                          # :576-616
        tmp = res[:9].reshape(3, 3).T.copy()
        scale = 1.0 / math.pow(abs(math.sqrt(tmp[:, 0] @ tmp[:, 0]) * math.sqrt(tmp[:, 1] @ tmp[:, 1]) * math.sqrt(tmp[:, 2] @ tmp[:, 2])), 1.0 / 3.0)
        U, _, Vt = np.linalg.svd(tmp)
        R = U @ Vt
        if np.linalg.det(R) < 0:
            R = -R
        t0 = R @ (scale * res[9:12])
        Ri = R.T.copy()                                            # Ts[s].inverse(): [R^T | -+ R^T t]
        cand = [-(Ri @ t0), Ri @ t0]
        errs = [direction_error(Ri, tt) for tt in cand]
        tout = cand[0] if errs[0] < errs[1] else cand[1]
        Rout = Ri
    x = np.concatenate([rot2rodrigues(Rout), tout])                # :622-629
    x = mlpnp_gn(x, pts, nulls, jac)                               # :631
    return np.hstack([rodrigues2rot(x[:3]), x[3:, None]]), planar  # :633-637


def pose7_of(Rt):
    """Tcw as qx qy qz qw tx ty tz: the quaternion in double (the library's branches), then float32"""
    m = Rt
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        t = math.sqrt(t + 1.0); qw = 0.5 * t; t = 0.5 / t
        qx, qy, qz = (m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t
    elif m[0, 0] >= m[1, 1] and m[0, 0] >= m[2, 2]:
        t = math.sqrt(m[0, 0] - m[1, 1] - m[2, 2] + 1.0); qx = 0.5 * t; t = 0.5 / t
        qw, qy, qz = (m[2, 1] - m[1, 2]) * t, (m[1, 0] + m[0, 1]) * t, (m[2, 0] + m[0, 2]) * t
    elif m[1, 1] >= m[2, 2]:
        t = math.sqrt(m[1, 1] - m[2, 2] - m[0, 0] + 1.0); qy = 0.5 * t; t = 0.5 / t
        qw, qz, qx = (m[0, 2] - m[2, 0]) * t, (m[2, 1] + m[1, 2]) * t, (m[0, 1] + m[1, 0]) * t
    else:
        t = math.sqrt(m[2, 2] - m[0, 0] - m[1, 1] + 1.0); qz = 0.5 * t; t = 0.5 / t
        qw, qx, qy = (m[1, 0] - m[0, 1]) * t, (m[0, 2] + m[2, 0]) * t, (m[1, 2] + m[2, 1]) * t
    return np.array([qx, qy, qz, qw, m[0, 3], m[1, 3], m[2, 3]]).astype(np.float32)


class Solver:
    """MLPnPsolver: the constructor (:35-77), SetRansacParameters, iterate (:80-203), CheckInliers (:242-273), Refine (:275-333)."""

    def __init__(self, keys, match, Xw, level_sigma2, cam4, params=None, **switches):
        params = dict(REFERENCE_PARAMS, **(params or {}))
        self.switches = switches
        self.cam = [F32(v) for v in cam4]                          # fx fy cx cy as Pinhole holds them
        fx, fy, cx, cy = self.cam
        self.n_keypoints = len(keys)
        idx = [i for i in range(len(keys)) if match[i] >= 0]
        self.kp_index = np.array(idx, np.int64)                    # mvKeyPointIndices
        self.p2d = np.array([[keys["x"][i], keys["y"][i]] for i in idx], np.float32).reshape(-1, 2)
        sigma2 = np.array([level_sigma2[keys["octave"][i]] for i in idx], np.float32)
        self.Xw = np.asarray(Xw, np.float32).reshape(-1, 3)[[match[i] for i in idx]].reshape(-1, 3)
        x = (self.p2d[:, 0] - cx) / fx                             # :58-59 unproject in float, / z
        y = (self.p2d[:, 1] - cy) / fy
        self.f = np.stack([x, y, np.ones_like(x)], 1).astype(np.float64)
        self.N = len(idx)
        self.min_inliers, self.max_its = ransac_parameters(self.N, **params)
        self.max_error = (sigma2 * F32(params["th2"])).astype(np.float32)     # :239
        self.iterations, self.best_inliers = 0, 0
        self.best_flags = np.zeros(self.N, bool)
        self.best_Tcw = np.zeros((3, 4), np.float32)
        self.best_Rt = None

    def check_inliers(self, Rt):
        """:242-273 -> (flags, count, error2 / maxError)"""
        X = self.Xw.astype(np.float64)
        cam = []
        for r in range(3):
            cam.append((((Rt[r, 0] * X[:, 0] + Rt[r, 1] * X[:, 1]) + Rt[r, 2] * X[:, 2]) + Rt[r, 3]).astype(np.float32))
        fx, fy, cx, cy = self.cam
        with np.errstate(all="ignore"):
            u = fx * cam[0] / cam[2] + cx
            v = fy * cam[1] / cam[2] + cy
            dx = self.p2d[:, 0] - u
            dy = self.p2d[:, 1] - v
            e2 = dx * dx + dy * dy
            flags = e2 < self.max_error
            ratio = e2.astype(np.float64) / self.max_error.astype(np.float64)
        return flags, int(flags.sum()), ratio

    def iterate(self, n_iterations, draws):
        """-> dict(found, no_more, n_inliers, inlier [n_keypoints], Rt (double 3 x 4 the returned pose was rounded from), used (draws
        consumed), log: per iteration run (Rt, count, flags, ratio))"""
        out = dict(found=0, no_more=0, n_inliers=0, inlier=np.zeros(self.n_keypoints, np.uint8), Rt=np.hstack([np.eye(3), np.zeros((3, 1))]),
                   used=0, log=[], ret=-2)
        if self.N < self.min_inliers:                              # :86-90
            out["no_more"] = 1
            return out
        cur, d = 0, 0
        while self.iterations < self.max_its or cur < n_iterations:        # :95
            cur += 1
            self.iterations += 1
            avail = list(range(self.N))
            pick = []
            for _ in range(6):                                     # :108-120
                r = random_int(int(draws[d]), 0, len(avail) - 1); d += 1
                pick.append(avail[r])
                avail[r] = avail[-1]
                avail.pop()
            Rt, _ = compute_pose(self.f[pick], self.Xw[pick].astype(np.float64), **self.switches)
            flags, count, ratio = self.check_inliers(Rt)
            out["log"].append((Rt, count, flags, ratio))
            out["used"] = d
            if count >= self.min_inliers:                          # :149
                if count > self.best_inliers:                      # :152-167
                    self.best_flags, self.best_inliers = flags.copy(), count
                    self.best_Tcw, self.best_Rt = Rt.astype(np.float32), Rt.copy()
                # Refine() (:275-333): computePose on the best set is discarded, CheckInliers re-tests this iteration's pose
                if count > self.min_inliers:                       # :316
                    out.update(found=1, n_inliers=count, Rt=Rt, ret=cur - 1)
                    out["inlier"][self.kp_index[flags]] = 1
                    return out
        if self.iterations >= self.max_its:                        # :185-200
            out["no_more"] = 1
            if self.best_inliers >= self.min_inliers:
                out.update(found=1, n_inliers=self.best_inliers, ret=-1)
                out["inlier"][self.kp_index[self.best_flags]] = 1
                out["Rt"] = self.best_Rt if self.best_Rt is not None else self.best_Tcw.astype(np.float64)
        return out

    def forget_double_best(self):
        """what a caller that carries only tc2li_mlpnp_state between calls has: mBestTcw in float"""
        self.best_Rt = None

// MLPnPsolver (SF/src/MLPnPsolver.cpp) as arithmetic shared by the host entry (mlpnp_host.cpp) and the kernels (mlpnp_kernels.hip):
// the six draws of an iteration (:108-120), computePose on six points (:336-638), one correspondence of CheckInliers (:242-273),
// the selection of iterate() (:80-203) and the pose conversion.  Every array a solve indexes with a run-time index lives in a strided
// work space (Ws): on the device one lane's column of an LDS tile, on the host a plain array.  What stays in locals is indexed by
// compile-time constants only, so the kernels need no private memory.  Compile with -ffp-contract=off.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MLPNP_HD __host__ __device__ inline
#else
#define MLPNP_HD inline
#endif

namespace tc2li {
namespace mlpnp {

constexpr int kWsDoubles = 288;   // two 12 x 12 matrices: the largest thing a solve holds at once
constexpr int kMaxSweeps = 30;
constexpr double kEps = 2.220446049250313e-16;

struct Ws {
    double* p;
    int stride;
    MLPNP_HD double& operator[](int i) const { return p[(size_t)i * stride]; }
    MLPNP_HD Ws at(int off) const { return Ws{p + (size_t)off * stride, stride}; }
};

// What a solve reads of its problem: the correspondences (constructor, :35-77) and the camera (float, as Pinhole holds it).
struct Corr {
    const float* p2d;    // [N][2] mvP2D
    const float* Xw;     // [N][3] mvP3Dw
    float fx, fy, cx, cy;
};

// DUtils::Random::RandomInt(0, size - 1) from one rand() value (Thirdparty/DBoW2/DUtils/Random.cpp:47-50; RAND_MAX = 2^31 - 1)
MLPNP_HD int random_int(uint32_t r, int size) {
    const int d = (size - 1) - 0 + 1;
    return int(((double)r / (2147483647.0 + 1.0)) * d) + 0;
}

// :58-60 unproject(pt) / z in float, widened
MLPNP_HD void bearing(const Corr& c, int i, double f[3]) {
    const float x = (c.p2d[2 * i] - c.cx) / c.fx, y = (c.p2d[2 * i + 1] - c.cy) / c.fy, z = 1.f;
    f[0] = (double)(x / z); f[1] = (double)(y / z); f[2] = (double)(z / z);
}
MLPNP_HD void world_point(const Corr& c, int i, double X[3]) {
    X[0] = (double)c.Xw[3 * i]; X[1] = (double)c.Xw[3 * i + 1]; X[2] = (double)c.Xw[3 * i + 2];
}
// An orthonormal basis of the complement of f (:351-353 takes columns 1, 2 of the V of a 1 x 3 SVD: any such basis).  Here the first two
// columns of the Householder reflection that maps f / |f| to -e3; f[2] = 1 > 0, so v = f / |f| + e3 never cancels.
MLPNP_HD void nullspace(const double f[3], double r[3], double s[3]) {
    const double n = sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
    const double v0 = f[0] / n, v1 = f[1] / n, v2 = f[2] / n + 1.0;
    const double k = 2.0 / (v0 * v0 + v1 * v1 + v2 * v2);
    r[0] = 1.0 - k * v0 * v0; r[1] = -k * v1 * v0; r[2] = -k * v2 * v0;
    s[0] = -k * v0 * v1; s[1] = 1.0 - k * v1 * v1; s[2] = -k * v2 * v1;
}

// One-sided Jacobi (Hestenes) on the n x n column-major W: on return W = W0 * V with orthogonal columns, V orthogonal.  For the
// symmetric positive semi-definite A^T A the column norms are the eigenvalues and V the eigenvectors, each accurate to rounding relative
// to its own size; for a general 3 x 3 it is the SVD W0 = (W D^-1) D V^T.  Stands for the JacobiSVD of :503 and :526 / :585.
MLPNP_HD void jacobi_onesided(Ws W, Ws V, int n) {
    for (int c = 0; c < n; ++c)
        for (int r = 0; r < n; ++r) V[c * n + r] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < n - 1; ++p)
            for (int q = p + 1; q < n; ++q) {
                double a = 0.0, b = 0.0, c = 0.0;
                for (int r = 0; r < n; ++r) {
                    const double wp = W[p * n + r], wq = W[q * n + r];
                    a += wp * wp; b += wq * wq; c += wp * wq;
                }
                if (!(fabs(c) > kEps * sqrt(a * b))) continue;
                rotated = true;
                const double zeta = (b - a) / (2.0 * c);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
                for (int r = 0; r < n; ++r) {
                    const double wp = W[p * n + r], wq = W[q * n + r];
                    W[p * n + r] = cs * wp - sn * wq; W[q * n + r] = sn * wp + cs * wq;
                    const double vp = V[p * n + r], vq = V[q * n + r];
                    V[p * n + r] = cs * vp - sn * vq; V[q * n + r] = sn * vp + cs * vq;
                }
            }
        if (!rotated) break;
    }
}
MLPNP_HD double col_norm2(Ws W, int n, int c) {
    double a = 0.0;
    for (int r = 0; r < n; ++r) a += W[c * n + r] * W[c * n + r];
    return a;
}
// The sign of an eigenvector or singular vector is the decomposition's choice; here: the entry of largest magnitude (the first of them)
// is positive.
MLPNP_HD void fix_sign(Ws v, int n, int step) {
    int best = 0;
    for (int i = 1; i < n; ++i)
        if (fabs(v[i * step]) > fabs(v[best * step])) best = i;
    if (v[best * step] < 0.0)
        for (int i = 0; i < n; ++i) v[i * step] = -v[i * step];
}

// FullPivHouseholderQR<Matrix3d>::rank() with the default threshold (:362, :369): pivot = the entry of largest magnitude of the remaining
// corner (column-major scan, first wins), rows and columns swapped, a Householder reflection per column; the decomposition stops at a
// corner no larger than epsilon * 3 * the first pivot; rank = the diagonal entries above epsilon * 3 * the largest of them.  Q [c*3+r]
// is destroyed.
MLPNP_HD int fullpiv_rank3(Ws Q) {
    const double precision = kEps * 3.0;
    int nonzero = 3;
    double maxpivot = 0.0, biggest = 0.0;
    for (int k = 0; k < 3; ++k) {
        int br = k, bc = k;
        double big = -1.0;
        for (int c = k; c < 3; ++c)
            for (int r = k; r < 3; ++r) {
                const double a = fabs(Q[c * 3 + r]);
                if (a > big) { big = a; br = r; bc = c; }
            }
        if (k == 0) biggest = big;
        if (fabs(big) <= fabs(biggest) * precision) { nonzero = k; break; }
        for (int c = k; c < 3; ++c) { const double t = Q[c * 3 + k]; Q[c * 3 + k] = Q[c * 3 + br]; Q[c * 3 + br] = t; }
        for (int r = 0; r < 3; ++r) { const double t = Q[k * 3 + r]; Q[k * 3 + r] = Q[bc * 3 + r]; Q[bc * 3 + r] = t; }
        const double c0 = Q[k * 3 + k];
        double tail = 0.0;
        for (int r = k + 1; r < 3; ++r) tail += Q[k * 3 + r] * Q[k * 3 + r];
        double tau, beta;
        if (tail <= 2.2250738585072014e-308) { tau = 0.0; beta = c0; for (int r = k + 1; r < 3; ++r) Q[k * 3 + r] = 0.0; }
        else {
            beta = sqrt(c0 * c0 + tail);
            if (c0 >= 0.0) beta = -beta;
            for (int r = k + 1; r < 3; ++r) Q[k * 3 + r] = Q[k * 3 + r] / (c0 - beta);
            tau = (beta - c0) / beta;
        }
        Q[k * 3 + k] = beta;
        if (fabs(beta) > maxpivot) maxpivot = fabs(beta);
        for (int c = k + 1; c < 3; ++c) {
            double w = Q[c * 3 + k];
            for (int r = k + 1; r < 3; ++r) w += Q[k * 3 + r] * Q[c * 3 + r];
            Q[c * 3 + k] -= tau * w;
            for (int r = k + 1; r < 3; ++r) Q[c * 3 + r] -= tau * w * Q[k * 3 + r];
        }
    }
    int rank = 0;
    for (int i = 0; i < nonzero; ++i) rank += fabs(Q[i * 3 + i]) > maxpivot * precision ? 1 : 0;
    return rank;
}

// ---- 3 x 3 helpers on locals, row-major, constant indices only ----
struct M3 { double m[9]; };
MLPNP_HD double det3(const M3& a) {
    return a.m[0] * (a.m[4] * a.m[8] - a.m[5] * a.m[7]) - a.m[1] * (a.m[3] * a.m[8] - a.m[5] * a.m[6]) + a.m[2] * (a.m[3] * a.m[7] - a.m[4] * a.m[6]);
}
MLPNP_HD M3 mul3(const M3& a, const M3& b) {
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[3 * i] * b.m[j] + a.m[3 * i + 1] * b.m[3 + j] + a.m[3 * i + 2] * b.m[6 + j];
    return o;
}
MLPNP_HD M3 transpose3(const M3& a) {
    M3 o;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) o.m[3 * i + j] = a.m[3 * j + i];
    return o;
}
MLPNP_HD M3 scale3(const M3& a, double s) {
    M3 o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.m[i] = a.m[i] * s;
    return o;
}
MLPNP_HD void mulv3(const M3& a, const double x[3], double o[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) o[i] = a.m[3 * i] * x[0] + a.m[3 * i + 1] * x[1] + a.m[3 * i + 2] * x[2];
}
// U * V^T of the SVD of G (:526-527, :585-586): the orthogonal polar factor, through the one-sided Jacobi in work space T (18 doubles)
MLPNP_HD M3 polar3(const M3& G, Ws T) {
    Ws W = T, V = T.at(9);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) W[c * 3 + r] = G.m[3 * r + c];
    jacobi_onesided(W, V, 3);
    M3 o;
#pragma unroll
    for (int i = 0; i < 9; ++i) o.m[i] = 0.0;
    for (int c = 0; c < 3; ++c) {
        const double n = sqrt(col_norm2(W, 3, c));
        const double u0 = W[c * 3] / n, u1 = W[c * 3 + 1] / n, u2 = W[c * 3 + 2] / n;
        const double v0 = V[c * 3], v1 = V[c * 3 + 1], v2 = V[c * 3 + 2];
        o.m[0] += u0 * v0; o.m[1] += u0 * v1; o.m[2] += u0 * v2;
        o.m[3] += u1 * v0; o.m[4] += u1 * v1; o.m[5] += u1 * v2;
        o.m[6] += u2 * v0; o.m[7] += u2 * v1; o.m[8] += u2 * v2;
    }
    return o;
}

// rodrigues2rot (:640-655)
MLPNP_HD M3 rodrigues2rot(const double w[3]) {
    M3 R = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    const double th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    if (th > kEps) {
        const double a = sin(th) / th, b = (1 - cos(th)) / (th * th);
        const M3 K = {{0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0}};
        const M3 K2 = mul3(K, K);
#pragma unroll
        for (int i = 0; i < 9; ++i) R.m[i] = R.m[i] + a * K.m[i] + b * K2.m[i];
    }
    return R;
}
// rot2rodrigues (:657-672)
MLPNP_HD void rot2rodrigues(const M3& R, double w[3]) {
    w[0] = w[1] = w[2] = 0.0;
    const double trace = R.m[0] + R.m[4] + R.m[8] - 1.0;
    const double wnorm = acos(trace / 2.0);
    if (wnorm > kEps) {
        const double sc = wnorm / (2.0 * sin(wnorm));
        w[0] = (R.m[7] - R.m[5]) * sc; w[1] = (R.m[2] - R.m[6]) * sc; w[2] = (R.m[3] - R.m[1]) * sc;
    }
}

// The two residual rows of one point and their derivatives (mlpnp_residuals_and_jacs :740-786; mlpnpJacs :788-1036 derived, not
// transcribed): res = n^T p / |p| with p = R(w) X + t, so d res / dt = n^T (I - u u^T) / |p| with u = p / |p|, and d res / dw_k is that
// row times d(R(w) X) / dw_k of R = I + a K + b K^2 (a = sin th / th, b = (1 - cos th) / th^2, K X = w x X, K^2 X = w (w.X) - th^2 X).
// At |w| <= epsilon the limit e_k x X is taken, where the generated expression of the reference divides by zero.
MLPNP_HD void residual_jac(const double w[3], const double t[3], const M3& R, const double X[3], const double nr[3], const double ns[3],
                           double res[2], double Jr[6], double Js[6]) {
    double p[3];
    mulv3(R, X, p);
    p[0] += t[0]; p[1] += t[1]; p[2] += t[2];
    const double np = sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2]);
    const double u[3] = {p[0] / np, p[1] / np, p[2] / np};
    res[0] = nr[0] * u[0] + nr[1] * u[1] + nr[2] * u[2];
    res[1] = ns[0] * u[0] + ns[1] * u[1] + ns[2] * u[2];
    double gr[3], gs[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { gr[i] = (nr[i] - res[0] * u[i]) / np; gs[i] = (ns[i] - res[1] * u[i]) / np; }
    const double th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], th = sqrt(th2);
    double a = 1.0, b = 0.5, da = 0.0, db = 0.0;   // da = a' / th, db = b' / th
    const bool small = !(th > kEps);
    if (!small) {
        const double s = sin(th), c = cos(th);
        a = s / th; b = (1 - c) / th2;
        da = (th * c - s) / (th2 * th); db = (th * s - 2 * (1 - c)) / (th2 * th2);
    }
    const double wX[3] = {w[1] * X[2] - w[2] * X[1], w[2] * X[0] - w[0] * X[2], w[0] * X[1] - w[1] * X[0]};
    const double wdX = w[0] * X[0] + w[1] * X[1] + w[2] * X[2];
    const double wwX[3] = {w[0] * wdX - th2 * X[0], w[1] * wdX - th2 * X[1], w[2] * wdX - th2 * X[2]};
    const double eX[3][3] = {{0.0, -X[2], X[1]}, {X[2], 0.0, -X[0]}, {-X[1], X[0], 0.0}};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double d[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            d[i] = a * eX[k][i];
            if (!small) d[i] += da * w[k] * wX[i] + db * w[k] * wwX[i] + b * ((i == k ? wdX : 0.0) + w[i] * X[k] - 2.0 * w[k] * X[i]);
        }
        Jr[k] = gr[0] * d[0] + gr[1] * d[1] + gr[2] * d[2];
        Js[k] = gs[0] * d[0] + gs[1] * d[1] + gs[2] * d[2];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) { Jr[3 + i] = gr[i]; Js[3 + i] = gs[i]; }
}

// sum over the six points of 1 - v . f, v = (R X + t) / |R X + t| (:559-567, :605-609; f is not of unit length)
MLPNP_HD double direction_error(const Corr& c, const int idx[6], const M3& R, const double t[3]) {
    double e = 0.0;
    for (int p = 0; p < 6; ++p) {
        double X[3], f[3], v[3];
        world_point(c, idx[p], X); bearing(c, idx[p], f);
        mulv3(R, X, v);
        v[0] += t[0]; v[1] += t[1]; v[2] += t[2];
        const double n = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n;
        e += (1.0 - (v[0] * f[0] + v[1] * f[1] + v[2] * f[2]));
    }
    return e;
}

// mlpnp_gn (:674-738) on the six points.  Work space G: J 72, JtJ 36, g 6, dx 6.
MLPNP_HD void gauss_newton(const Corr& c, const int idx[6], double x[6], Ws G) {
    Ws J = G, A = G.at(72), g = G.at(108), dx = G.at(114);
    for (int it = 0; it < 5; ++it) {
        const double w[3] = {x[0], x[1], x[2]}, t[3] = {x[3], x[4], x[5]};
        const M3 R = rodrigues2rot(w);
        for (int i = 0; i < 36; ++i) A[i] = 0.0;
        for (int i = 0; i < 6; ++i) g[i] = 0.0;
        for (int p = 0; p < 6; ++p) {
            double X[3], f[3], nr[3], ns[3], res[2], Jr[6], Js[6];
            world_point(c, idx[p], X); bearing(c, idx[p], f); nullspace(f, nr, ns);
            residual_jac(w, t, R, X, nr, ns, res, Jr, Js);
#pragma unroll
            for (int i = 0; i < 6; ++i) { J[(2 * p) * 6 + i] = Jr[i]; J[(2 * p + 1) * 6 + i] = Js[i]; }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 6; ++j) A[i * 6 + j] += Jr[i] * Jr[j];
                g[i] += Jr[i] * res[0];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
#pragma unroll
                for (int j = 0; j < 6; ++j) A[i * 6 + j] += Js[i] * Js[j];
                g[i] += Js[i] * res[1];
            }
        }
        // LDL^T of the 6 x 6 normal matrix in place (:720-721; no pivoting: J^T J is positive definite wherever the step is used)
        for (int j = 0; j < 6; ++j) {
            double d = A[j * 6 + j];
            for (int k = 0; k < j; ++k) d -= A[j * 6 + k] * A[j * 6 + k] * A[k * 6 + k];
            A[j * 6 + j] = d;
            for (int i = j + 1; i < 6; ++i) {
                double l = A[i * 6 + j];
                for (int k = 0; k < j; ++k) l -= A[i * 6 + k] * A[j * 6 + k] * A[k * 6 + k];
                A[i * 6 + j] = l / d;
            }
        }
        for (int i = 0; i < 6; ++i) {
            double s = g[i];
            for (int k = 0; k < i; ++k) s -= A[i * 6 + k] * dx[k];
            dx[i] = s;
        }
        for (int i = 0; i < 6; ++i) dx[i] = dx[i] / A[i * 6 + i];
        for (int i = 5; i >= 0; --i) {
            double s = dx[i];
            for (int k = i + 1; k < 6; ++k) s -= A[k * 6 + i] * dx[k];
            dx[i] = s;
        }
        double amax = fabs(dx[0]), amin = fabs(dx[0]);
        for (int i = 1; i < 6; ++i) { const double a = fabs(dx[i]); if (a > amax) amax = a; if (a < amin) amin = a; }
        if (amax > 5.0 || amin > 1.0) break;
        double dl = 0.0;
        for (int r = 0; r < 12; ++r) {
            double s = 0.0;
            for (int i = 0; i < 6; ++i) s += J[r * 6 + i] * dx[i];
            if (r == 0 || fabs(s) > dl) dl = fabs(s);
        }
#pragma unroll
        for (int i = 0; i < 6; ++i) x[i] = x[i] - dx[i];
        if (dl < 1e-5) break;
    }
}

// computePose (:336-638) on the six correspondences idx of c: Rt = [R | t] row-major 3 x 4.  ws: kWsDoubles.
MLPNP_HD void compute_pose6(const Corr& c, const int idx[6], Ws ws, double Rt[12]) {
    Ws W = ws, V = ws.at(144);
    // 1. planar test on the uncentred second moment (:361-369)
    double S[6] = {0, 0, 0, 0, 0, 0};   // xx xy xz yy yz zz
    for (int p = 0; p < 6; ++p) {
        double X[3];
        world_point(c, idx[p], X);
        S[0] += X[0] * X[0]; S[1] += X[0] * X[1]; S[2] += X[0] * X[2]; S[3] += X[1] * X[1]; S[4] += X[1] * X[2]; S[5] += X[2] * X[2];
    }
    const double Sfull[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]};
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = Sfull[i];
    const bool planar = fullpiv_rank3(V) == 2;
    M3 E = {{1, 0, 0, 0, 1, 0, 0, 0, 1}};   // eigenRot
    if (planar) {
        // SelfAdjointEigenSolver (:374-376): eigenvalues ascending, eigenRot = eigenvectors^T
        Ws Sw = V.at(16), Sv = V.at(32);
#pragma unroll
        for (int i = 0; i < 9; ++i) Sw[i] = Sfull[i];
        jacobi_onesided(Sw, Sv, 3);
        double l0 = col_norm2(Sw, 3, 0), l1 = col_norm2(Sw, 3, 1), l2 = col_norm2(Sw, 3, 2);
        int o0 = 0, o1 = 1, o2 = 2;
        if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; const int k = o0; o0 = o1; o1 = k; }
        if (l2 < l1) { const double t = l1; l1 = l2; l2 = t; const int k = o1; o1 = o2; o2 = k; }
        if (l1 < l0) { const double t = l0; l0 = l1; l1 = t; const int k = o0; o0 = o1; o1 = k; }
        fix_sign(Sv.at(o0 * 3), 3, 1); fix_sign(Sv.at(o1 * 3), 3, 1); fix_sign(Sv.at(o2 * 3), 3, 1);
#pragma unroll
        for (int j = 0; j < 3; ++j) { E.m[j] = Sv[o0 * 3 + j]; E.m[3 + j] = Sv[o1 * 3 + j]; E.m[6 + j] = Sv[o2 * 3 + j]; }
    }
    // 3. + 4. A^T A accumulated row by row (:408-501); a row sits in V until the decomposition needs V
    const int n = planar ? 9 : 12;
    for (int i = 0; i < n * n; ++i) W[i] = 0.0;
    for (int p = 0; p < 6; ++p) {
        double X[3], f[3], nv[2][3], Xr[3];
        world_point(c, idx[p], X); bearing(c, idx[p], f); nullspace(f, nv[0], nv[1]);
        mulv3(E, X, Xr);
        if (!planar) { Xr[0] = X[0]; Xr[1] = X[1]; Xr[2] = X[2]; }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            if (planar) {
#pragma unroll
                for (int i = 0; i < 3; ++i) { V[2 * i] = nv[j][i] * Xr[1]; V[2 * i + 1] = nv[j][i] * Xr[2]; V[6 + i] = nv[j][i]; }
            } else {
#pragma unroll
                for (int i = 0; i < 3; ++i) { V[3 * i] = nv[j][i] * Xr[0]; V[3 * i + 1] = nv[j][i] * Xr[1]; V[3 * i + 2] = nv[j][i] * Xr[2]; V[9 + i] = nv[j][i]; }
            }
            for (int a = 0; a < n; ++a) {
                const double va = V[a];
                for (int b = 0; b < n; ++b) W[a * n + b] += va * V[b];
            }
        }
    }
    jacobi_onesided(W, V, n);
    int cmin = 0;
    double lmin = col_norm2(W, n, 0);
    for (int k = 1; k < n; ++k) { const double l = col_norm2(W, n, k); if (l < lmin) { lmin = l; cmin = k; } }
    Ws res = W;   // result1 (:504)
    for (int i = 0; i < n; ++i) res[i] = V[cmin * n + i];
    fix_sign(res, n, 1);
    Ws T = ws.at(16);   // 18 doubles for the 3 x 3 SVD
    M3 Rout;
    double tout[3];
    if (planar) {
        // :514-573
        const double c1[3] = {res[0], res[2], res[4]}, c2[3] = {res[1], res[3], res[5]};
        const double cr[3] = {c1[1] * c2[2] - c1[2] * c2[1], c1[2] * c2[0] - c1[0] * c2[2], c1[0] * c2[1] - c1[1] * c2[0]};
        const M3 tmp = {{cr[0], cr[1], cr[2], c1[0], c1[1], c1[2], c2[0], c2[1], c2[2]}};   // after transposeInPlace
        const double n1 = sqrt(tmp.m[1] * tmp.m[1] + tmp.m[4] * tmp.m[4] + tmp.m[7] * tmp.m[7]);
        const double n2 = sqrt(tmp.m[2] * tmp.m[2] + tmp.m[5] * tmp.m[5] + tmp.m[8] * tmp.m[8]);
        const double scale = 1.0 / sqrt(fabs(n1 * n2));
        const double tr[3] = {res[6], res[7], res[8]};
        M3 R1 = polar3(tmp, T);
        if (det3(R1) < 0) R1 = scale3(R1, -1.0);
        R1 = mul3(transpose3(E), R1);
        const double t[3] = {scale * tr[0], scale * tr[1], scale * tr[2]};
        R1 = scale3(transpose3(R1), -1.0);
        if (det3(R1) < 0.0) { R1.m[2] *= -1; R1.m[5] *= -1; R1.m[8] *= -1; }
        const M3 R2 = {{-R1.m[0], -R1.m[1], R1.m[2], -R1.m[3], -R1.m[4], R1.m[5], -R1.m[6], -R1.m[7], R1.m[8]}};
        const double tn[3] = {-t[0], -t[1], -t[2]};
        const double e0 = direction_error(c, idx, R1, t), e1 = direction_error(c, idx, R1, tn);
        const double e2 = direction_error(c, idx, R2, t), e3 = direction_error(c, idx, R2, tn);
        int best = 0;   // std::min_element: the first of the smallest
        double eb = e0;
        if (e1 < eb) { eb = e1; best = 1; }
        if (e2 < eb) { eb = e2; best = 2; }
        if (e3 < eb) { eb = e3; best = 3; }
        Rout = best < 2 ? R1 : R2;
#pragma unroll
        for (int i = 0; i < 3; ++i) tout[i] = (best & 1) ? tn[i] : t[i];
    } else {
        // :576-616
        const M3 tmp = {{res[0], res[3], res[6], res[1], res[4], res[7], res[2], res[5], res[8]}};
        const double n0 = sqrt(tmp.m[0] * tmp.m[0] + tmp.m[3] * tmp.m[3] + tmp.m[6] * tmp.m[6]);
        const double n1 = sqrt(tmp.m[1] * tmp.m[1] + tmp.m[4] * tmp.m[4] + tmp.m[7] * tmp.m[7]);
        const double n2 = sqrt(tmp.m[2] * tmp.m[2] + tmp.m[5] * tmp.m[5] + tmp.m[8] * tmp.m[8]);
        const double scale = 1.0 / pow(fabs(n0 * n1 * n2), 1.0 / 3.0);
        const double tr[3] = {scale * res[9], scale * res[10], scale * res[11]};
        M3 R = polar3(tmp, T);
        if (det3(R) < 0) R = scale3(R, -1.0);
        double t0[3];
        mulv3(R, tr, t0);
        // Ts[s].inverse() of [R | +-t0]: [R^T | -+ R^T t0]
        const M3 Ri = transpose3(R);
        double ta[3];
        mulv3(Ri, t0, ta);
        const double tneg[3] = {-ta[0], -ta[1], -ta[2]};
        const double e0 = direction_error(c, idx, Ri, tneg), e1 = direction_error(c, idx, Ri, ta);
        Rout = Ri;
#pragma unroll
        for (int i = 0; i < 3; ++i) tout[i] = e0 < e1 ? tneg[i] : ta[i];
    }
    // 5. Gauss-Newton (:622-637)
    double x[6];
    rot2rodrigues(Rout, x);
    x[3] = tout[0]; x[4] = tout[1]; x[5] = tout[2];
    gauss_newton(c, idx, x, ws.at(40));
    const M3 Rf = rodrigues2rot(x);
#pragma unroll
    for (int i = 0; i < 3; ++i) { Rt[4 * i] = Rf.m[3 * i]; Rt[4 * i + 1] = Rf.m[3 * i + 1]; Rt[4 * i + 2] = Rf.m[3 * i + 2]; Rt[4 * i + 3] = x[3 + i]; }
}

// One correspondence of CheckInliers (:247-263): double rotation times float point, each camera coordinate rounded to float,
// Pinhole::project in float, error2 < mvMaxError[i].
MLPNP_HD bool is_inlier(const Corr& c, int i, const double Rt[12], float max_error) {
    const float X = c.Xw[3 * i], Y = c.Xw[3 * i + 1], Z = c.Xw[3 * i + 2];
    const float xc = (float)(Rt[0] * X + Rt[1] * Y + Rt[2] * Z + Rt[3]);
    const float yc = (float)(Rt[4] * X + Rt[5] * Y + Rt[6] * Z + Rt[7]);
    const float zc = (float)(Rt[8] * X + Rt[9] * Y + Rt[10] * Z + Rt[11]);
    const float u = c.fx * xc / zc + c.cx, v = c.fy * yc / zc + c.cy;
    const float dx = c.p2d[2 * i] - u, dy = c.p2d[2 * i + 1] - v;
    const float e2 = dx * dx + dy * dy;
    return e2 < max_error;
}

// What one iterate() call does with the inlier counts of the iterations it may run (:95-202).  count(j) is mnInliersi of the call's j-th
// iteration.  Out: `ret` the iteration whose pose and flags are returned (Refine() succeeds iff its count > min_inliers: :311-316 re-test the
// iteration's own pose), -1 for the best so far, -2 for none; `best` the iteration that became the best, -1 when the state's stays.
struct Selection { int found, no_more, n_inliers, ret, best, iterations, best_inliers; };
template <typename CountFn>
MLPNP_HD Selection select(int n_corr, int min_inliers, int max_its, int n_iterations, int state_iterations, int state_best, CountFn count) {
    Selection s = {0, 0, 0, -2, -1, state_iterations, state_best};
    if (n_corr < min_inliers) { s.no_more = 1; return s; }
    int cur = 0;
    while (s.iterations < max_its || cur < n_iterations) {
        const int j = cur;
        ++cur; ++s.iterations;
        const int cnt = count(j);
        if (cnt >= min_inliers) {
            if (cnt > s.best_inliers) { s.best_inliers = cnt; s.best = j; }
            if (cnt > min_inliers) { s.found = 1; s.n_inliers = cnt; s.ret = j; return s; }
        }
    }
    if (s.iterations >= max_its) {
        s.no_more = 1;
        if (s.best_inliers >= min_inliers) { s.found = 1; s.n_inliers = s.best_inliers; s.ret = -1; }
    }
    return s;
}
// the iterations a call runs when none of them returns early
MLPNP_HD int iterations_of_call(int max_its, int n_iterations, int state_iterations) {
    int k = max_its - state_iterations;
    if (n_iterations > k) k = n_iterations;
    return k > 0 ? k : 0;
}

// Tcw as qx qy qz qw tx ty tz: the quaternion of the rotation in double (by the trace or the largest diagonal entry), then float
MLPNP_HD void pose7_of(const double Rt[12], float pose7[7]) {
    const double m00 = Rt[0], m01 = Rt[1], m02 = Rt[2], m10 = Rt[4], m11 = Rt[5], m12 = Rt[6], m20 = Rt[8], m21 = Rt[9], m22 = Rt[10];
    double qx, qy, qz, qw, t = m00 + m11 + m22;
    if (t > 0.0) {
        t = sqrt(t + 1.0); qw = 0.5 * t; t = 0.5 / t;
        qx = (m21 - m12) * t; qy = (m02 - m20) * t; qz = (m10 - m01) * t;
    } else if (m00 >= m11 && m00 >= m22) {
        t = sqrt(m00 - m11 - m22 + 1.0); qx = 0.5 * t; t = 0.5 / t;
        qw = (m21 - m12) * t; qy = (m10 + m01) * t; qz = (m20 + m02) * t;
    } else if (m11 >= m22) {
        t = sqrt(m11 - m22 - m00 + 1.0); qy = 0.5 * t; t = 0.5 / t;
        qw = (m02 - m20) * t; qz = (m21 + m12) * t; qx = (m01 + m10) * t;
    } else {
        t = sqrt(m22 - m00 - m11 + 1.0); qz = 0.5 * t; t = 0.5 / t;
        qw = (m10 - m01) * t; qx = (m02 + m20) * t; qy = (m12 + m21) * t;
    }
    pose7[0] = (float)qx; pose7[1] = (float)qy; pose7[2] = (float)qz; pose7[3] = (float)qw;
    pose7[4] = (float)Rt[3]; pose7[5] = (float)Rt[7]; pose7[6] = (float)Rt[11];
}

}  // namespace mlpnp
}  // namespace tc2li

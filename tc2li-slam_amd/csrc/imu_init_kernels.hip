// tc2li_inertial_optimization_batch on the device (imu_init_device.hpp has the edge, the chain step and the tables).  One workgroup of 256
// threads per map; the whole optimisation runs inside the launch, as k_pose_inertial's does.
//   k_ii_optimize  Optimizer::InertialOptimization, first overload: Levenberg-Marquardt with g2o's control (trials, backup and restore, stop
//                  rules).  Per linearisation, sixteen links at a time: lane 0 of a link's sixteen forms the edge with J [9 x 15] in LDS, the
//                  sixteen lanes then Omega J (one column each, the last lane Omega e) and row a of J' Omega J (lane a).  The rows that
//                  belong to velocities go to the work table per LINK -- D_i is the sum of exactly two of them, L_i is one, and the solver adds
//                  them where it reads them --; the rows of the shared unknowns are summed per lane over the passes in link order and then
//                  over the sixteen lanes in lane order.  The arrow solve: the chain over keyframes runs on ONE wavefront, every lane with
//                  the 3 x 3 carry (S^-1) in its own registers -- the same operations on the same operands in all lanes, so nothing is
//                  exchanged and no step waits for the LDS or a barrier -- and lane c with column c of Y = (B | bv).  The Schur complement of
//                  the border is one thread per entry over the rows in order, its LDL' one thread (ldlt_solve_small), the back substitution
//                  the first wavefront again.
//   k_ii_refine    the second overload: Gauss-Newton with Huber(1) on the gravity direction and the scale.  One lane per link with the three
//                  Jacobian columns it needs (parked in LDS for the products with Omega); the 3 x 3 system and the costs are summed as below.
// Sums over links: a lane adds its links in link order, the 256 partial sums go through one fixed tree in LDS.  No atomics; nothing depends on
// where a map sits in the grid, so a map's results are the same bits in any batch.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <float.h>
#include <stdint.h>

#include "imu_init_device.hpp"

namespace tc2li {
namespace {

struct IiShared {  // the shared unknowns
    double Rwg[9], s, bg[3], ba[3];
};
struct IiCtl {
    IiShared x, backup;
    double C[81], bc[9], Cs[81], rhs[9], xc[9];
    double lambda, ni;
    int ok;  // the trial's solve went through
};

// the sum of v over the workgroup in a fixed tree; every thread gets it.  red: kIiThreads doubles.
__device__ __forceinline__ double ii_block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int d = kIiThreads / 2; d > 0; d >>= 1) {
        if (t < d) red[t] += red[t + d];
        __syncthreads();
    }
    return red[0];
}
__device__ __forceinline__ double ii_block_max(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int d = kIiThreads / 2; d > 0; d >>= 1) {
        if (t < d) red[t] = fmax(red[t], red[t + d]);
        __syncthreads();
    }
    return red[0];
}

struct IiMap {  // the rows of one map
    const double *Rwb, *twb;
    double* vel;
    const PiPreint* pre;
    const uint8_t* ok;
    double* work;
    int N;
};
__device__ __forceinline__ IiMap ii_map(const IiBatch& B, const IiProblem& P) {
    const size_t o = (size_t)P.kf_off;
    return IiMap{B.Rwb + 9 * o, B.twb + 3 * o, B.vel + 3 * o, B.pre + o, B.link_ok + o, B.work + (size_t)P.work_off * kIiWorkPerKf, P.n_kf};
}
__device__ __forceinline__ double* ii_row(const IiMap& M, int i) { return M.work + (size_t)i * kIiWorkPerKf; }

// chi2 of the first form at (vel, x): the edges, then the two bias priors
__device__ double ii_chi2(const IiMap& M, const IiProblem& P, const IiShared& x, double* red) {
    double part = 0;
    for (int i = 1 + (int)threadIdx.x; i < M.N; i += kIiThreads) {
        if (!M.ok[i]) continue;
        double e[9], chi = 0;
        ii_gs_edge<0>(M.pre[i], M.Rwb + 9 * (i - 1), M.twb + 3 * (i - 1), M.vel + 3 * (i - 1), M.Rwb + 9 * i, M.twb + 3 * i, M.vel + 3 * i, x.bg, x.ba, x.Rwg,
                      x.s, e, nullptr);
        const double* O = M.pre[i].info;
        for (int r = 0; r < 9; ++r) for (int c = 0; c < 9; ++c) chi += e[r] * O[9 * r + c] * e[c];
        part += chi;
    }
    double chi = ii_block_sum(part, red);
    for (int k = 0; k < 3; ++k) chi += P.prior_a * x.ba[k] * x.ba[k] + P.prior_g * x.bg[k] * x.bg[k];
    return chi;
}

// entries of the tridiagonal part and the border from the per-link rows: keyframe k takes link k's V2 rows, then link k + 1's V1 rows
__device__ __forceinline__ double ii_pair(const IiMap& M, int k, int r, int col2, int col1) {
    double d = 0.0;
    if (k >= 1) d += ii_row(M, k)[(3 + r) * kIiEdgeRow + col2];
    if (k + 1 < M.N) d += ii_row(M, k + 1)[r * kIiEdgeRow + col1];
    return d;
}
__device__ __forceinline__ double ii_D(const IiMap& M, int k, int r, int c) { return ii_pair(M, k, r, 9 + c, c); }
__device__ __forceinline__ double ii_B(const IiMap& M, int k, int r, int col) { return ii_pair(M, k, r, col, col); }
__device__ __forceinline__ double ii_bv(const IiMap& M, int k, int r) {
    double d = 0.0;
    if (k >= 1) d -= ii_row(M, k)[(3 + r) * kIiEdgeRow + 15];
    if (k + 1 < M.N) d -= ii_row(M, k + 1)[r * kIiEdgeRow + 15];
    return d;
}
__device__ __forceinline__ double ii_L(const IiMap& M, int k, int r, int c) { return ii_row(M, k)[(3 + r) * kIiEdgeRow + c]; }  // T(k, k - 1), k >= 1

}  // namespace

__global__ __launch_bounds__(kIiThreads) void k_ii_optimize(IiBatch B) {
    // [link of the pass][J 135 | Omega J 135 | e 9 | Omega e 9]; the lanes' sums of row a of J' Omega J over their links [group][a][15 | gradient]
    // (in LDS, not in registers: thirty-two registers less across the edge's chain of 3 x 3 products)
    constexpr int kSlot = 135 + 135 + 9 + 9;
    __shared__ double s_buf[kIiEdgesPerPass * kSlot];
    __shared__ double s_part[kIiThreads * 16];
    __shared__ double s_red[kIiThreads];
    __shared__ IiCtl s;
    const int tid = threadIdx.x, grp = tid / kIiEdgeLanes, a = tid % kIiEdgeLanes;
    const int p = B.which[blockIdx.x];
    const IiProblem& P = B.problems[p];
    const IiMap M = ii_map(B, P);
    const int N = M.N;
    const bool mono = P.mono != 0, fixed_vel = P.fixed_vel != 0;
    const int m = ii_shared_count(mono, fixed_vel), w = m + 1, Nv = fixed_vel ? 0 : N;
    const int o_bg = fixed_vel ? -1 : 0, o_ba = fixed_vel ? -1 : 3, o_g = fixed_vel ? 0 : 6, o_s = mono ? o_g + 2 : -1;
    if (tid == 0) {
        for (int k = 0; k < 9; ++k) s.x.Rwg[k] = P.Rwg[k];
        for (int k = 0; k < 3; ++k) { s.x.bg[k] = P.bg[k]; s.x.ba[k] = P.ba[k]; }
        s.x.s = P.scale;
        s.lambda = 0; s.ni = 2;
    }
    __syncthreads();
    const double err0 = ii_chi2(M, P, s.x, s_red);
    int n_bad = 0, done = 0, trials = 0;
    for (int it = 0; it < P.iterations; ++it) {
        const double ini_chi = ii_chi2(M, P, s.x, s_red);
        double current_chi = ini_chi;
        // ---- linearise: J' Omega J and the gradient, sixteen links per pass ----
        double* const part = s_part + tid * 16;
        for (int c = 0; c < 16; ++c) part[c] = 0;
        for (int i0 = 1; i0 < N; i0 += kIiEdgesPerPass) {
            const int i = i0 + grp;
            const bool in = i < N, live = in && M.ok[i];
            double* const J = s_buf + grp * kSlot;
            double *const OJ = J + 135, *const e = OJ + 135, *const Oe = e + 9;
            __syncthreads();
            if (live && a == 0)
                ii_gs_edge<1>(M.pre[i], M.Rwb + 9 * (i - 1), M.twb + 3 * (i - 1), M.vel + 3 * (i - 1), M.Rwb + 9 * i, M.twb + 3 * i, M.vel + 3 * i, s.x.bg, s.x.ba,
                              s.x.Rwg, s.x.s, e, J);
            __syncthreads();
            if (live) {
                const double* O = M.pre[i].info;
                for (int r = 0; r < 9; ++r) {
                    double t = 0;
                    if (a < 15) { for (int k = 0; k < 9; ++k) t += O[9 * r + k] * J[15 * k + a]; OJ[15 * r + a] = t; }
                    else { for (int k = 0; k < 9; ++k) t += O[9 * r + k] * e[k]; Oe[r] = t; }
                }
            }
            __syncthreads();
            if (in && a < 15) {
                const bool vel_col = a < 3 || (a >= 9 && a < 12);
                double* const out = ii_row(M, i) + (a < 3 ? a : a - 6) * kIiEdgeRow;
                double grad = 0;
                if (live) for (int r = 0; r < 9; ++r) grad += J[15 * r + a] * Oe[r];
                if (vel_col) out[15] = grad; else part[15] += grad;
                for (int c = 0; c < 15; ++c) {
                    double h = 0;
                    if (live) for (int r = 0; r < 9; ++r) h += J[15 * r + a] * OJ[15 * r + c];
                    if (vel_col) out[c] = h; else part[c] += h;
                }
            }
        }
        __syncthreads();
        {   // the shared rows: over the sixteen groups' lanes that had the row, in group order
            if (tid < m * w) {
                const int r = tid / w, c = tid % w, cr = ii_shared_column(r, fixed_vel), cc = c < m ? ii_shared_column(c, fixed_vel) : 15;
                double t = 0;
                for (int g = 0; g < kIiEdgesPerPass; ++g) t += s_part[(g * 16 + cr) * 16 + cc];
                if (c < m) {
                    // EdgePriorAcc / EdgePriorGyro: error = 0 - b, Jacobian as the reference declares it: +I (SF/src/G2oTypes.cc:769-781)
                    if (r == c && o_ba >= 0 && r >= o_ba && r < o_ba + 3) t += P.prior_a;
                    if (r == c && o_bg >= 0 && r >= o_bg && r < o_bg + 3) t += P.prior_g;
                    s.C[r * m + c] = t;
                } else {
                    t = 0.0 - t;
                    if (o_ba >= 0 && r >= o_ba && r < o_ba + 3) t -= P.prior_a * (0.0 - s.x.ba[r - o_ba]);
                    if (o_bg >= 0 && r >= o_bg && r < o_bg + 3) t -= P.prior_g * (0.0 - s.x.bg[r - o_bg]);
                    s.bc[r] = t;
                }
            }
            __syncthreads();
        }
        if (it == 0) {
            double lambda0 = 1e3;
            if (P.prior_g == 0.0) {  // tau times the largest diagonal entry
                double md = 0;
                for (int q = tid; q < 3 * Nv; q += kIiThreads) md = fmax(md, fabs(ii_D(M, q / 3, q % 3, q % 3)));
                if (tid < m) md = fmax(md, fabs(s.C[tid * m + tid]));
                lambda0 = 1e-5 * ii_block_max(md, s_red);
            }
            __syncthreads();
            if (tid == 0) { s.lambda = lambda0; s.ni = 2; }
            n_bad = 0;
            __syncthreads();
        }
        double rho = 0;
        int qmax = 0;
        do {
            const double lambda = s.lambda;
            // ---- backup ----
            for (int q = tid; q < 3 * Nv; q += kIiThreads) ii_row(M, q / 3)[kIiOffBackup + q % 3] = M.vel[q];
            if (tid == 0) { s.backup = s.x; s.ok = 1; }
            __syncthreads();
            // ---- the chain: S_i, Y_i = (B_i | bv_i) - G Y_{i-1}, Z_i = S_i^-1 Y_i; first wavefront, lane c has column c ----
            if (tid < 64 && Nv > 0) {
                const int c = tid < w ? tid : m, col = c < m ? ii_shared_column(c, fixed_vel) : 15;
                double Sinv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, D[9], L[9], y[3], y_prev[3] = {0, 0, 0};
                bool ok = true;
                for (int i = 0; i < Nv && ok; ++i) {
                    for (int r = 0; r < 3; ++r)
                        for (int q = 0; q < 3; ++q) { D[3 * r + q] = ii_D(M, i, r, q); L[3 * r + q] = i > 0 ? ii_L(M, i, r, q) : 0.0; }
                    for (int r = 0; r < 3; ++r) y[r] = c < m ? ii_B(M, i, r, col) : ii_bv(M, i, r);
                    double Sp[9];
                    for (int k = 0; k < 9; ++k) Sp[k] = Sinv[k];
                    ok = ii_arrow_pivot(D, L, Sp, i == 0, lambda, G, Sinv);
                    if (!ok) break;
                    if (i > 0) ii_arrow_eliminate(G, y_prev, y);
                    double* const row = ii_row(M, i);
                    if (tid < w)
                        for (int r = 0; r < 3; ++r) {
                            row[kIiOffY + r * kIiYw + c] = y[r];
                            row[kIiOffZ + r * kIiYw + c] = Sinv[3 * r] * y[0] + Sinv[3 * r + 1] * y[1] + Sinv[3 * r + 2] * y[2];
                            y_prev[r] = y[r];
                        }
                    else for (int r = 0; r < 3; ++r) y_prev[r] = y[r];
                    if (tid == 0) for (int k = 0; k < 9; ++k) row[kIiOffSinv + k] = Sinv[k];
                }
                if (tid == 0 && !ok) s.ok = 0;
            }
            __syncthreads();
            // ---- the Schur complement of the border: Cs = C + lambda I - Y' Z, rhs = bc - Y' z ----
            if (s.ok && tid < m * w) {
                const int r = tid / w, c = tid % w;
                double t = c < m ? s.C[r * m + c] + (r == c ? lambda : 0.0) : s.bc[r];
                for (int q = 0; q < 3 * Nv; ++q) {
                    const double* row = ii_row(M, q / 3);
                    t -= row[kIiOffY + (q % 3) * kIiYw + r] * row[kIiOffZ + (q % 3) * kIiYw + c];
                }
                if (c < m) s.Cs[r * m + c] = t; else s.rhs[r] = t;
            }
            __syncthreads();
            if (tid == 0 && s.ok) {
                for (int k = 0; k < m; ++k) s.xc[k] = 0;
                if (!ldlt_solve_small(s.Cs, m, s.rhs, s.xc, false)) s.ok = 0;
            }
            __syncthreads();
            const bool ok2 = s.ok != 0;
            double sc = 0;
            if (ok2) {
                // ---- back substitution: x_i = S_i^-1 (Y_i(:, m) - Y_i(:, :m) xc - L_{i+1}' x_{i+1}) ----
                for (int q = tid; q < 3 * Nv; q += kIiThreads) {
                    double* const row = ii_row(M, q / 3);
                    double t = row[kIiOffY + (q % 3) * kIiYw + m];
                    for (int c = 0; c < m; ++c) t -= row[kIiOffY + (q % 3) * kIiYw + c] * s.xc[c];
                    row[kIiOffT + q % 3] = t;
                }
                __syncthreads();
                if (tid < 64) {
                    double x_next[3] = {0, 0, 0};
                    for (int i = Nv - 1; i >= 0; --i) {
                        double* const row = ii_row(M, i);
                        double r3[3], x[3];
                        for (int r = 0; r < 3; ++r) {
                            double t = row[kIiOffT + r];
                            if (i + 1 < Nv) for (int k = 0; k < 3; ++k) t -= ii_L(M, i + 1, k, r) * x_next[k];
                            r3[r] = t;
                        }
                        r3_vec(row + kIiOffSinv, r3, x);
                        for (int r = 0; r < 3; ++r) x_next[r] = x[r];
                        if (tid == 0) for (int r = 0; r < 3; ++r) row[kIiOffX + r] = x[r];
                    }
                }
                __syncthreads();
                // ---- apply ----
                double part = 0;
                for (int q = tid; q < 3 * Nv; q += kIiThreads) {
                    const double xq = ii_row(M, q / 3)[kIiOffX + q % 3];
                    M.vel[q] += xq;
                    part += xq * (lambda * xq + ii_bv(M, q / 3, q % 3));
                }
                if (tid == 0) {
                    if (!fixed_vel) for (int k = 0; k < 3; ++k) { s.x.bg[k] += s.xc[o_bg + k]; s.x.ba[k] += s.xc[o_ba + k]; }
                    const double wv[3] = {s.xc[o_g], s.xc[o_g + 1], 0.0};  // GDirection::Update
                    double E[9], R[9];
                    exp_so3(wv, E);
                    r3_mul(s.x.Rwg, E, R);
                    for (int k = 0; k < 9; ++k) s.x.Rwg[k] = R[k];
                    if (mono) s.x.s *= exp(s.xc[o_s]);
                }
                sc = ii_block_sum(part, s_red);
                for (int k = 0; k < m; ++k) sc += s.xc[k] * (lambda * s.xc[k] + s.bc[k]);
            }
            __syncthreads();
            const double temp_chi = ok2 ? ii_chi2(M, P, s.x, s_red) : DBL_MAX;
            rho = current_chi - temp_chi;
            sc += 1e-3;
            rho /= sc;
            const bool accept = rho > 0 && temp_chi - temp_chi == 0.0;  // g2o: rho > 0 && g2o_isfinite(tempChi)
            __syncthreads();
            if (accept) {
                if (tid == 0) {
                    double alpha = 1. - pow((2 * rho - 1), 3);
                    alpha = fmin(alpha, 2. / 3.);
                    s.lambda *= fmax(1. / 3., alpha);
                    s.ni = 2;
                }
                current_chi = temp_chi;
            } else {
                if (tid == 0) { s.lambda *= s.ni; s.ni *= 2; s.x = s.backup; }
                for (int q = tid; q < 3 * Nv; q += kIiThreads) M.vel[q] = ii_row(M, q / 3)[kIiOffBackup + q % 3];
            }
            __syncthreads();
            ++qmax; ++trials;
        } while (rho < 0 && qmax < 10);
        ++done;
        if (qmax == 10 || rho == 0) break;
        if ((ini_chi - current_chi) * 1e3 < ini_chi) n_bad++; else n_bad = 0;
        if (n_bad >= 3) break;
    }
    const double err1 = ii_chi2(M, P, s.x, s_red);
    if (tid == 0) {
        IiResult& R = B.results[p];
        for (int k = 0; k < 9; ++k) R.Rwg[k] = s.x.Rwg[k];
        for (int k = 0; k < 3; ++k) { R.bg[k] = s.x.bg[k]; R.ba[k] = s.x.ba[k]; }
        R.scale = s.x.s; R.chi2[0] = err0; R.chi2[1] = err1; R.lambda = s.lambda; R.iterations = done; R.trials = trials;
    }
}

// ---- the second overload -------------------------------------------------------------------------------------------------------------------
namespace {
__device__ __forceinline__ void ii_huber1(double c, double& r0, double& r1) {  // RobustKernelHuber, delta 1
    const float dsqr = 1.f;
    if (c <= dsqr) { r0 = c; r1 = 1.0; } else { const double q = sqrt(c); r0 = 2 * q * 1.0 - dsqr; r1 = 1.0 / q; }
}
// activeRobustChi2 at (Rwg, s)
__device__ double ii_robust_chi2(const IiMap& M, const double* bg3, const double* ba3, const double* Rwg, double sc, double* red) {
    double part = 0;
    for (int i = 1 + (int)threadIdx.x; i < M.N; i += kIiThreads) {
        if (!M.ok[i]) continue;
        double e[9], c = 0, r0, r1;
        ii_gs_edge<0>(M.pre[i], M.Rwb + 9 * (i - 1), M.twb + 3 * (i - 1), M.vel + 3 * (i - 1), M.Rwb + 9 * i, M.twb + 3 * i, M.vel + 3 * i, bg3 + 3 * (i - 1),
                      ba3 + 3 * (i - 1), Rwg, sc, e, nullptr);
        const double* O = M.pre[i].info;
        for (int r = 0; r < 9; ++r) for (int q = 0; q < 9; ++q) c += e[r] * O[9 * r + q] * e[q];
        ii_huber1(c, r0, r1);
        part += r0;
    }
    return ii_block_sum(part, red);
}
}  // namespace

__global__ __launch_bounds__(kIiThreads) void k_ii_refine(IiBatch B) {
    __shared__ double s_red[kIiThreads];
    __shared__ double s_acc[12][kIiThreads];  // H [9] | b [3]: every lane's sums over its links
    __shared__ double s_eJ[36][kIiThreads];   // e [9] | J [9 x 3] of the lane's link
    __shared__ double s_Rwg[9], s_scale, s_H[9], s_b[3];
    __shared__ int s_ok;
    const int tid = threadIdx.x;
    const int p = B.which[blockIdx.x];
    const IiProblem& P = B.problems[p];
    const IiMap M = ii_map(B, P);
    const double *bg3 = B.bg3 + 3 * (size_t)P.kf_off, *ba3 = B.ba3 + 3 * (size_t)P.kf_off;
    if (tid == 0) { for (int k = 0; k < 9; ++k) s_Rwg[k] = P.Rwg[k]; s_scale = P.scale; }
    __syncthreads();
    const double chi0 = ii_robust_chi2(M, bg3, ba3, s_Rwg, s_scale, s_red);
    int done = 0;
    for (int it = 0; it < P.iterations; ++it) {
        for (int k = 0; k < 12; ++k) s_acc[k][tid] = 0;
        for (int i = 1 + tid; i < M.N; i += kIiThreads) {
            if (!M.ok[i]) continue;
            double e[9], J[27], g[3] = {0, 0, 0}, h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, c = 0, r0, r1;
            ii_gs_edge<2>(M.pre[i], M.Rwb + 9 * (i - 1), M.twb + 3 * (i - 1), M.vel + 3 * (i - 1), M.Rwb + 9 * i, M.twb + 3 * i, M.vel + 3 * i, bg3 + 3 * (i - 1),
                          ba3 + 3 * (i - 1), s_Rwg, s_scale, e, J);
            const double* O = M.pre[i].info;
            // row r of Omega (e | J) and at once its terms of e' Omega e, J' Omega e and J' Omega J: the sums run over r in order, as the
            // host's do over its stored Omega e and Omega J.  e and J wait in LDS so that the rows are a loop: unrolled, the 81 loads of
            // Omega are all in flight at once and cost a hundred registers.
            for (int k = 0; k < 9; ++k) s_eJ[k][tid] = e[k];
            for (int k = 0; k < 27; ++k) s_eJ[9 + k][tid] = J[k];
#pragma unroll 1
            for (int r = 0; r < 9; ++r) {
                double t = 0, wq[3] = {0, 0, 0};
                for (int k = 0; k < 9; ++k) t += O[9 * r + k] * s_eJ[k][tid];
                for (int q = 0; q < 3; ++q) for (int k = 0; k < 9; ++k) wq[q] += O[9 * r + k] * s_eJ[9 + 3 * k + q][tid];
                c += s_eJ[r][tid] * t;
                for (int a = 0; a < 3; ++a) {
                    const double Jra = s_eJ[9 + 3 * r + a][tid];
                    g[a] += Jra * t;
                    for (int q = 0; q < 3; ++q) h[3 * a + q] += Jra * wq[q];
                }
            }
            ii_huber1(c, r0, r1);
            for (int a = 0; a < 3; ++a) {
                s_acc[9 + a][tid] -= r1 * g[a];
                for (int q = 0; q < 3; ++q) s_acc[3 * a + q][tid] += r1 * h[3 * a + q];
            }
        }
        for (int k = 0; k < 12; ++k) {
            const double t = ii_block_sum(s_acc[k][tid], s_red);
            if (tid == 0) { if (k < 9) s_H[k] = t; else s_b[k - 9] = t; }
        }
        __syncthreads();
        if (tid == 0) {
            double u[3];
            s_ok = ldlt_solve_small(s_H, 3, s_b, u, false) ? 1 : 0;
            if (s_ok) {
                const double wv[3] = {u[0], u[1], 0.0};
                double E[9], R[9];
                exp_so3(wv, E);
                r3_mul(s_Rwg, E, R);
                for (int k = 0; k < 9; ++k) s_Rwg[k] = R[k];
                s_scale *= exp(u[2]);
            }
        }
        __syncthreads();
        if (!s_ok) break;
        ++done;
    }
    const double chi1 = ii_robust_chi2(M, bg3, ba3, s_Rwg, s_scale, s_red);
    if (tid == 0) {
        IiResult& R = B.results[p];
        for (int k = 0; k < 9; ++k) R.Rwg[k] = s_Rwg[k];
        for (int k = 0; k < 3; ++k) { R.bg[k] = P.bg[k]; R.ba[k] = P.ba[k]; }
        R.scale = s_scale; R.chi2[0] = chi0; R.chi2[1] = chi1; R.lambda = 0; R.iterations = done; R.trials = done;
    }
}

void launch_inertial_init(const IiBatch& B, bool refine, hipStream_t st) {
    if (B.n <= 0) return;
    if (refine) TC2LI_LAUNCH(k_ii_refine, dim3(B.n), dim3(kIiThreads), 0, st, B);
    else TC2LI_LAUNCH(k_ii_optimize, dim3(B.n), dim3(kIiThreads), 0, st, B);
}

}  // namespace tc2li

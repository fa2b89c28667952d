// Optimizer::InertialOptimization, both overloads (SF/src/Optimizer.cc:2169-2356, 2359-2466), for many maps at once
// (tc2li_inertial_optimization_batch, include/tc2li_hip.h "IMU initialisation: the inertial optimisation, batched"): the tables the host
// entry and imu_init_kernels.hip share, and the arithmetic that is the same wherever it runs:
//   EdgeInertialGS::computeError / linearizeOplus            SF/src/G2oTypes.cc:603-724       ii_gs_edge_at
//   the block LDL' of the tridiagonal velocity part           ArrowSystem::solve (imu_init_host.cpp)  ii_arrow_pivot, ii_arrow_eliminate
// imu_init_host.cpp calls both (its results are the bits they were before the arithmetic moved here).  What differs between the sides is
// the pre-integration at the new bias that the edge is given: tc2li_imu_delta on the host, pi_delta (pose_inertial_device.hpp) in the kernels.
#pragma once
#include "pose_inertial_device.hpp"

namespace tc2li {
// a line in device code that neither the compiler's code motion nor its instruction scheduler moves work across (see ii_gs_edge_at)
#ifdef __HIP_DEVICE_COMPILE__
#define TC2LI_II_STAGE() do { asm volatile("" ::: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TC2LI_II_STAGE() ((void)0)
#endif

constexpr int kIiMaxKeyframes = 256;         // first overload: every frame a keyframe for 15 s at 10 Hz is 150
constexpr int kIiMaxRefineKeyframes = 4096;  // second overload: no per-keyframe solver state
constexpr int kIiMaxIterations = 200;        // the reference's 200 (first overload) and 10 (second); bounds every launch
constexpr int kIiThreads = 256;              // one workgroup per map
constexpr int kIiEdgeLanes = 16;             // lanes that share one edge while it is linearised: 15 Jacobian columns + Omega e
constexpr int kIiEdgesPerPass = kIiThreads / kIiEdgeLanes;
// Work table, doubles per keyframe row i (the link i joins keyframes i - 1 and i):
//   edge [6][16]  the rows of J' Omega J that belong to the velocities (V1 0..2, V2 3..5) over the 15 columns, then the gradient entry
//   Y [3][10], Z [3][10] = S^-1 Y, Sinv [9], t [3] (right-hand side of the back substitution), xv [3], backup of the velocity [3]
constexpr int kIiEdgeRow = 16, kIiEdge = 6 * kIiEdgeRow, kIiYw = 10;
constexpr int kIiOffY = kIiEdge, kIiOffZ = kIiOffY + 3 * kIiYw, kIiOffSinv = kIiOffZ + 3 * kIiYw, kIiOffT = kIiOffSinv + 9, kIiOffX = kIiOffT + 3,
              kIiOffBackup = kIiOffX + 3, kIiWorkPerKf = kIiOffBackup + 3;

// One map as the kernels see it.  Rows kf_off .. kf_off + n_kf of the keyframe tables; link i is row kf_off + i of the link tables.  Only
// the maps of the first form have rows in the work table, from work_off on.
struct IiProblem {
    int32_t kf_off, n_kf, mono, fixed_vel, iterations, work_off;
    double prior_g, prior_a;  // the floats, widened
    double Rwg[9], scale, bg[3], ba[3];
};
struct IiResult {
    double Rwg[9], scale, bg[3], ba[3], chi2[2], lambda;
    int32_t iterations, trials;
};
struct IiBatch {
    const IiProblem* problems;
    const int32_t* which;     // [n]: the problems of this launch
    const double* Rwb;        // [rows][9]
    const double* twb;        // [rows][3]
    double* vel;              // [rows][3]: in / out in the first form
    const double* bg3;        // [rows][3], [rows][3]: the refinement form's fixed biases
    const double* ba3;
    const PiPreint* pre;      // [rows]; row kf_off + 0 of a map is unused
    const uint8_t* link_ok;   // [rows]: 0 = no link (a NULL entry)
    double* work;             // [rows of the first form's maps][kIiWorkPerKf]
    IiResult* results;        // [all problems]
    int32_t n;
};

void launch_inertial_init(const IiBatch& B, bool refine, hipStream_t st);

// The shared unknowns [bg 3 | ba 3 |] gdir 2 [| scale 1] and the Jacobian column (V1 3 | bg 3 | ba 3 | V2 3 | gdir 2 | scale 1) of each
__host__ __device__ inline int ii_shared_count(bool mono, bool fixed_vel) { return (fixed_vel ? 2 : 8) + (mono ? 1 : 0); }
__host__ __device__ inline int ii_shared_column(int k, bool fixed_vel) { return fixed_vel ? 12 + k : (k < 6 ? 3 + k : 6 + k); }

// EdgeInertialGS between keyframes i - 1 and i, given the pre-integration at the current bias: dR, dV, dP = GetDelta*(b) widened, dbg = the
// float difference of the gyro biases, widened.  Pre: tc2li_preintegrated or PiPreint (dT and the float bias Jacobians).  MODE 0: the error.
// MODE 1: and J [9 x 15] (V1 3 | bg 3 | ba 3 | V2 3 | gdir 2 | scale 1).  MODE 2: and J [9 x 3], the gdir and scale columns alone.
// TC2LI_II_STAGE: on the device, a line the compiler does not move work across -- interleaved, the edge's independent chains of 3 x 3
// products are all live at once and the kernel runs out of registers.
template <int MODE, class Pre>
__host__ __device__ inline void ii_gs_edge_at(const Pre& pre, const double* dR, const double* dV, const double* dP, const double* dbg, const double* Rwb1,
                                              const double* twb1, const double* v1, const double* Rwb2, const double* twb2, const double* v2, const double* Rwg,
                                              double s, double err[9], double* J) {
    constexpr double kG = (double)9.81f;  // IMU::GRAVITY_VALUE is a float constant
    TC2LI_II_STAGE();
    double g[3], Rbw1[9], dRt[9], t1[9], eR[9], er[3], dv[3], dp[3], rv[3], rp[3];
    const double gI[3] = {0, 0, -kG}, dt = (double)pre.dT;
    r3_vec(Rwg, gI, g);
    pi_tr(Rwb1, Rbw1); pi_tr(dR, dRt);
    r3_mul(dRt, Rbw1, t1); r3_mul(t1, Rwb2, eR);
    pi_log_so3(eR, er);
    TC2LI_II_STAGE();
    for (int k = 0; k < 3; ++k) {
        dv[k] = s * (v2[k] - v1[k]) - g[k] * dt;
        dp[k] = s * (twb2[k] - twb1[k] - v1[k] * dt) - g[k] * dt * dt / 2;
    }
    r3_vec(Rbw1, dv, rv); r3_vec(Rbw1, dp, rp);
    for (int k = 0; k < 3; ++k) { err[k] = er[k]; err[3 + k] = rv[k] - dV[k]; err[6 + k] = rp[k] - dP[k]; }
    if (MODE == 0) return;
    TC2LI_II_STAGE();
    constexpr int W = MODE == 1 ? 15 : 3, G0 = MODE == 1 ? 12 : 0;  // row width, the first gdir column
    for (int k = 0; k < 9 * W; ++k) J[k] = 0;
#define TC2LI_II_PUT(r0, c0, m, f) for (int r_ = 0; r_ < 3; ++r_) for (int c_ = 0; c_ < 3; ++c_) J[W * ((r0) + r_) + (c0) + c_] = (f) * (double)(m)[3 * r_ + c_]
    if (MODE == 1) {
        TC2LI_II_PUT(3, 0, Rbw1, -s); TC2LI_II_PUT(6, 0, Rbw1, -s * dt);
        double invJr[9], JRg[9], Jd[3], RJ[9], eRt[9], a1[9], a2[9], a3[9];
        TC2LI_II_STAGE();
        pi_jr_so3(er, true, invJr);
        TC2LI_II_STAGE();
        for (int k = 0; k < 9; ++k) JRg[k] = pre.JRg[k];
        r3_vec(JRg, dbg, Jd);
        pi_jr_so3(Jd, false, RJ);
        TC2LI_II_STAGE();
        pi_tr(eR, eRt);
        r3_mul(invJr, eRt, a1); r3_mul(a1, RJ, a2); r3_mul(a2, JRg, a3);
        TC2LI_II_STAGE();
        TC2LI_II_PUT(0, 3, a3, -1.0); TC2LI_II_PUT(3, 3, pre.JVg, -1.0); TC2LI_II_PUT(6, 3, pre.JPg, -1.0);  // (the float Jacobians, widened)
        TC2LI_II_PUT(3, 6, pre.JVa, -1.0); TC2LI_II_PUT(6, 6, pre.JPa, -1.0);
        TC2LI_II_PUT(3, 9, Rbw1, s);
    }
    TC2LI_II_STAGE();
#undef TC2LI_II_PUT
    // dGdTheta = Rwg * [0 -G; G 0; 0 0]
    for (int r = 0; r < 3; ++r) {
        double c0 = 0, c1 = 0;
        for (int k = 0; k < 3; ++k) { c0 += Rbw1[3 * r + k] * (Rwg[3 * k + 1] * kG); c1 += Rbw1[3 * r + k] * (Rwg[3 * k] * -kG); }
        J[W * (3 + r) + G0] = -c0 * dt; J[W * (3 + r) + G0 + 1] = -c1 * dt;
        J[W * (6 + r) + G0] = -0.5 * c0 * dt * dt; J[W * (6 + r) + G0 + 1] = -0.5 * c1 * dt * dt;
    }
    double d1[3], d2[3], s1[3], s2[3];
    for (int k = 0; k < 3; ++k) { d1[k] = v2[k] - v1[k]; d2[k] = twb2[k] - twb1[k] - v1[k] * dt; }
    r3_vec(Rbw1, d1, s1); r3_vec(Rbw1, d2, s2);
    for (int r = 0; r < 3; ++r) { J[W * (3 + r) + G0 + 2] = s1[r]; J[W * (6 + r) + G0 + 2] = s2[r]; }
}

// The same with the device's pre-integration at the bias (bg, ba): pi_delta
template <int MODE>
__host__ __device__ inline void ii_gs_edge(const PiPreint& pre, const double* Rwb1, const double* twb1, const double* v1, const double* Rwb2,
                                           const double* twb2, const double* v2, const double* bg, const double* ba, const double* Rwg, double s,
                                           double err[9], double* J) {
    double dR[9], dV[3], dP[3];
    float dbgf[3];
    pi_delta(pre, bg, ba, dR, dV, dP, dbgf);
    const double dbg[3] = {(double)dbgf[0], (double)dbgf[1], (double)dbgf[2]};
    ii_gs_edge_at<MODE>(pre, dR, dV, dP, dbg, Rwb1, twb1, v1, Rwb2, twb2, v2, Rwg, s, err, J);
}

// ---- the arrow solver's chain, one keyframe per step -----------------------------------------------------------------------------------
__host__ __device__ inline bool ii_inv3(const double* a, double* o) {
    const double c0 = a[4] * a[8] - a[5] * a[7], c1 = a[5] * a[6] - a[3] * a[8], c2 = a[3] * a[7] - a[4] * a[6];
    const double det = a[0] * c0 + a[1] * c1 + a[2] * c2;
    if (!(fabs(det) > 0) || !(det - det == 0.0)) return false;  // zero, NaN or infinite
    const double id = 1.0 / det;
    o[0] = c0 * id; o[1] = (a[2] * a[7] - a[1] * a[8]) * id; o[2] = (a[1] * a[5] - a[2] * a[4]) * id;
    o[3] = c1 * id; o[4] = (a[0] * a[8] - a[2] * a[6]) * id; o[5] = (a[2] * a[3] - a[0] * a[5]) * id;
    o[6] = c2 * id; o[7] = (a[1] * a[6] - a[0] * a[7]) * id; o[8] = (a[0] * a[4] - a[1] * a[3]) * id;
    return true;
}
// S_i = D_i + lambda I - L_i S_{i-1}^-1 L_i' and its inverse; G = L_i S_{i-1}^-1 (first: no block above, G is not written).
// false: the pivot block is singular -- nothing may be read from Sinv then.
__host__ __device__ inline bool ii_arrow_pivot(const double* D, const double* L, const double* Sinv_prev, bool first, double lambda, double* G, double* Sinv) {
    double S[9];
    for (int k = 0; k < 9; ++k) S[k] = D[k];
    S[0] += lambda; S[4] += lambda; S[8] += lambda;
    if (!first) {
        r3_mul(L, Sinv_prev, G);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) { double t = 0; for (int k = 0; k < 3; ++k) t += G[3 * r + k] * L[3 * c + k]; S[3 * r + c] -= t; }
    }
    return ii_inv3(S, Sinv);
}
// one column of Y_i = (B_i | bv_i) - G Y_{i-1}
__host__ __device__ inline void ii_arrow_eliminate(const double* G, const double* y_prev, double* y) {
    for (int r = 0; r < 3; ++r) { double t = 0; for (int k = 0; k < 3; ++k) t += G[3 * r + k] * y_prev[k]; y[r] -= t; }
}

}  // namespace tc2li

// The inertial term of a local-BA window (EdgeInertial + EdgeGyroRW + EdgeAccRW per link, SF/src/G2oTypes.cc:499-601,
// SF/include/G2oTypes.h:645-714; the values of InertialTerm::cost, ba_internal.hpp) as tc2li_inertial_term_batch evaluates it: the tables
// the host entry and the kernels share, and the arithmetic of ONE link -- it_link() -- that inertial_term_kernels.hip runs on a wavefront
// and inertial_term_host.cpp on a thread.  Every value is formed by one lane with the same serial operations whatever the number of lanes,
// so the two sides differ by the compilers' contraction and libm only.
//
// Unknowns of a keyframe (15): pose 6 (the body-frame update of VertexPose: columns P1 / P2 of pi_inertial_edge) | velocity 3 | gyro bias 3 |
// acc bias 3.  For kf2 the inertial edge has pose and velocity columns only; its bias rows and columns get the random-walk edges alone.
#pragma once
#include "ba_math.hpp"
#include "pose_inertial_device.hpp"

namespace tc2li {

constexpr int kItMaxKeyframes = 256;  // per window: the reference's largest graph has 25 + 200 vertices
constexpr int kItMaxLinks = 256;      // per window; both only bound the serial walks of a window's and a keyframe's links
constexpr int kItU = 15;              // unknowns per keyframe
constexpr int kItBlock = kItU * kItU;
constexpr int kItSide = kItBlock + kItU;     // what a link gives one of its keyframes: the diagonal block, then the 15 gradient entries
constexpr int kItPerLink = 2 * kItSide;      // [kf1's side | kf2's side] in the work table
constexpr int kItLinkThreads = 256;          // k_it_link: one wavefront per link
constexpr int kItCostThreads = 64;           // k_it_cost: one lane per link

struct ItLink { int32_t kf1, kf2, robust, free_mask; };  // kf1 / kf2: rows of the batch's keyframe table; free_mask: 1 = kf1 free, 2 = kf2 free

// What one lane forms of a link before anything is spread: error, Omega e, the random-walk products and the costs
struct ItVals {
    double e[9], Oe[9], Og[3], Oa[3];
    double c2, rho0, rho1, rw_gyro, rw_acc;
};
__host__ __device__ inline double it_cost(const ItVals& v) { return (v.rho0 + v.rw_gyro) + v.rw_acc; }

// The batch as the kernels see it.  kf_off / kf_items: per keyframe the (link << 1 | side) of every link that has it as a FREE end, in link
// order.  blocks [n_links][kItPerLink], cost [n_links]: work tables.
struct ItBatch {
    const PiState* states;
    const PiPreint* pre;
    const ItLink* links;
    const int32_t* kf_off;
    const int32_t* kf_items;
    const int32_t* win_link_off;  // [n_windows + 1]
    double* chi2;                 // [n_windows]
    double* H_diag;               // [n_keyframes][15][15]
    double* H_link;               // [n_links][15][15]
    double* b;                    // [n_keyframes][15]
    double* blocks;
    double* cost;
    int32_t n_links, n_keyframes, n_windows;
    float huber_dsqr;
    double huber_d;               // (double)sqrtf(16.92f) and the float of its square, as InertialTerm::prepare
};

void launch_inertial_term(const ItBatch& B, bool linearize, hipStream_t st);

// ---- one lane: the edge, its cost ------------------------------------------------------------------------------------------------------
// J [9 x 24] or NULL
__host__ __device__ inline void it_link_values(const PiPreint& pre, const PiState& s1, const PiState& s2, bool robust, double huber_d, float huber_dsqr,
                                               ItVals& v, double* J) {
    pi_inertial_edge(pre, s1, s2, v.e, J);
    double c2 = 0;
    for (int r = 0; r < 9; ++r) {
        double s = 0;
        for (int k = 0; k < 9; ++k) s += pre.info[9 * r + k] * v.e[k];
        v.Oe[r] = s;
        c2 += v.e[r] * s;
    }
    double rho0 = c2, rho1 = 1.0;
    if (robust) huber(c2, huber_d, huber_dsqr, rho0, rho1);
    v.c2 = c2; v.rho0 = rho0; v.rho1 = rho1;
    double eg[3], ea[3], cg = 0, ca = 0;  // EdgeGyroRW / EdgeAccRW: error = kf2 - kf1, never robust
    for (int k = 0; k < 3; ++k) { eg[k] = s2.bg[k] - s1.bg[k]; ea[k] = s2.ba[k] - s1.ba[k]; }
    for (int r = 0; r < 3; ++r) {
        v.Og[r] = pre.infoG[3 * r] * eg[0] + pre.infoG[3 * r + 1] * eg[1] + pre.infoG[3 * r + 2] * eg[2];
        v.Oa[r] = pre.infoA[3 * r] * ea[0] + pre.infoA[3 * r + 1] * ea[1] + pre.infoA[3 * r + 2] * ea[2];
        cg += eg[r] * v.Og[r];
        ca += ea[r] * v.Oa[r];
    }
    v.rw_gyro = cg; v.rw_acc = ca;
}

// ---- spread over n_lanes: (rho' Omega) J, then the blocks ----------------------------------------------------------------------------------
// the column of J that unknown u of kf2 has, -1: none (unknown u of kf1 has column u)
__host__ __device__ inline int it_col2(int u) { return u < 9 ? 15 + u : -1; }
__host__ __device__ inline double it_jtj(const double* J, const double* T, int ci, int cj) {
    double h = 0;
    for (int k = 0; k < 9; ++k) h += J[24 * k + ci] * T[24 * k + cj];
    return h;
}
// the random-walk information between unknowns (r, c) of a keyframe: infoG on the gyro-bias block, infoA on the acc-bias block
__host__ __device__ inline double it_walk(const PiPreint& pre, int r, int c) {
    if (r >= 9 && r < 12 && c >= 9 && c < 12) return pre.infoG[3 * (r - 9) + (c - 9)];
    if (r >= 12 && c >= 12) return pre.infoA[3 * (r - 12) + (c - 12)];
    return 0.0;
}
// -J^T (rho' Omega e) of the column, then the random-walk edge's share: +Omega e for kf1 (J = -I), -Omega e for kf2 (J = +I)
__host__ __device__ inline double it_gradient(const double* J, const ItVals& v, int u, int col, double sign) {
    double s = 0;
    if (col >= 0) for (int k = 0; k < 9; ++k) s += J[24 * k + col] * (v.rho1 * v.Oe[k]);
    double g = 0.0 - s;
    if (u >= 9 && u < 12) g += sign * v.Og[u - 9];
    if (u >= 12) g += sign * v.Oa[u - 12];
    return g;
}

// The link's blocks from J and the values: T = (rho' Omega) J [9 x 24] (work), side1 / side2 [kItSide] = the diagonal block and the gradient of
// kf1 / kf2 (written only for a free end: a fixed end gets nothing), L12 [15 x 15] = rows kf1's unknowns, columns kf2's (zero unless both
// ends are free).  sync(): what makes the lanes' writes to T visible to each other.
template <class Sync>
__host__ __device__ inline void it_link_blocks(const PiPreint& pre, const ItVals& v, const double* J, double* T, bool free1, bool free2, double* side1,
                                               double* side2, double* L12, int lane, int n_lanes, Sync sync) {
    for (int i = lane; i < 9 * 24; i += n_lanes) {
        const int r = i / 24, c = i % 24;
        double t = 0;
        for (int k = 0; k < 9; ++k) t += v.rho1 * pre.info[9 * r + k] * J[24 * k + c];
        T[i] = t;
    }
    sync();
    for (int i = lane; i < 2 * kItSide + kItBlock; i += n_lanes) {
        const int part = i < kItSide ? 0 : i < 2 * kItSide ? 1 : 2, k = i - part * kItSide;
        if (part == 2) {
            const int r = k / kItU, c = k % kItU, cc = it_col2(c);
            L12[k] = !(free1 && free2) ? 0.0 : cc >= 0 ? it_jtj(J, T, r, cc) : 0.0 - it_walk(pre, r, c);
            continue;
        }
        if (!(part == 0 ? free1 : free2)) continue;
        double* out = part == 0 ? side1 : side2;
        if (k >= kItBlock) {
            const int u = k - kItBlock;
            out[k] = it_gradient(J, v, u, part == 0 ? u : it_col2(u), part == 0 ? 1.0 : -1.0);
            continue;
        }
        const int r = k / kItU, c = k % kItU, cr = part == 0 ? r : it_col2(r), cc = part == 0 ? c : it_col2(c);
        const double h = (cr >= 0 && cc >= 0) ? it_jtj(J, T, cr, cc) : 0.0;
        out[k] = h + it_walk(pre, r, c);
    }
}

struct ItNoSync {  // one lane: nothing to wait for
    __host__ __device__ void operator()() const {}
};

// One link, by n_lanes lanes that share v, J and T: lane 0 forms the edge, then everybody the blocks when `linearize`.
template <class Sync>
__host__ __device__ inline void it_link(const PiPreint& pre, const PiState& s1, const PiState& s2, const ItLink& lk, double huber_d, float huber_dsqr,
                                        bool linearize, ItVals& v, double* J, double* T, double* side1, double* side2, double* L12, int lane, int n_lanes,
                                        Sync sync) {
    if (lane == 0) it_link_values(pre, s1, s2, lk.robust != 0, huber_d, huber_dsqr, v, linearize ? J : nullptr);
    if (!linearize) return;
    sync();
    it_link_blocks(pre, v, J, T, (lk.free_mask & 1) != 0, (lk.free_mask & 2) != 0, side1, side2, L12, lane, n_lanes, sync);
}

// ---- the sums, in link order -----------------------------------------------------------------------------------------------------------
// entry e of [H_diag block | b] of a keyframe with the items kf_items[i0 .. i1)
__host__ __device__ inline double it_keyframe_entry(const int32_t* kf_items, int i0, int i1, const double* blocks, int e) {
    double s = 0.0;
    for (int i = i0; i < i1; ++i) s += blocks[(size_t)(kf_items[i] >> 1) * kItPerLink + (size_t)(kf_items[i] & 1) * kItSide + e];
    return s;
}
__host__ __device__ inline double it_window_chi2(const double* cost, int l0, int l1) {
    double s = 0.0;
    for (int l = l0; l < l1; ++l) s += cost[l];
    return s;
}

}  // namespace tc2li

// tc2li_inertial_term_batch on the device (inertial_term_device.hpp has the arithmetic of a link and the tables).
//   k_it_link      one wavefront per link, four links per workgroup.  The link's record and its two states are staged in LDS; lane 0 forms the
//                  edge -- error, the 9 x 24 Jacobian, Omega e, Huber, the random-walk products: one serial chain -- with J in LDS; the 64
//                  lanes then form (rho' Omega) J into LDS and the 705 entries of the link's blocks from the two (J^T Omega J: 9 products
//                  per entry).  The link block goes to H_link, the two keyframes' shares and the link's cost to work tables.
//   k_it_assemble  one workgroup per keyframe: entry e of [H_diag | b] by thread e, summed over the keyframe's links in link order from the
//                  CSR table the host built; a keyframe without a free end of a link gets zeros.  The workgroups behind the keyframes'
//                  sum every window's costs in link order, one thread per window.
//   k_it_cost      linearize == 0: one lane per link, no Jacobian (the edge's error is a serial chain: more lanes per link would idle),
//   k_it_chi2      then the windows' sums as above.
// No atomics, no value that depends on where a link or a keyframe sits in the grid: a link's values come from one wavefront's fixed
// sequence, a sum from one thread's.  Every output entry is written by exactly one thread.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "inertial_term_device.hpp"

namespace tc2li {

// LDS writes of this wavefront's lanes become visible to its other lanes (as pi_ldlt_solve_wave, pose_inertial_kernel.hip)
struct ItWaveSync {
    __device__ __forceinline__ void operator()() const {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    }
};

template <class T>
__device__ __forceinline__ void it_stage(T* dst, const T* src, int lane) {
    static_assert(sizeof(T) % 4 == 0, "copied as dwords");
    for (int k = lane; k < (int)(sizeof(T) / 4); k += 64) reinterpret_cast<uint32_t*>(dst)[k] = reinterpret_cast<const uint32_t*>(src)[k];
}

__global__ __launch_bounds__(kItLinkThreads) void k_it_link(ItBatch B) {
    constexpr int kWaves = kItLinkThreads / 64;
    __shared__ PiPreint s_pre[kWaves];
    __shared__ PiState s_state[kWaves][2];
    __shared__ ItVals s_vals[kWaves];
    __shared__ double s_J[kWaves][216], s_T[kWaves][216];
    const int wave = wave_in_block(), lane = threadIdx.x & 63;
    const int l = blockIdx.x * kWaves + wave;
    if (l >= B.n_links) return;  // (no workgroup barrier below: the wavefronts are independent)
    const ItLink lk = B.links[l];
    it_stage(&s_pre[wave], &B.pre[l], lane);
    it_stage(&s_state[wave][0], &B.states[lk.kf1], lane);
    it_stage(&s_state[wave][1], &B.states[lk.kf2], lane);
    ItWaveSync sync;
    sync();
    double* const side1 = B.blocks + (size_t)l * kItPerLink;
    it_link(s_pre[wave], s_state[wave][0], s_state[wave][1], lk, B.huber_d, B.huber_dsqr, true, s_vals[wave], s_J[wave], s_T[wave], side1, side1 + kItSide,
            B.H_link + (size_t)l * kItBlock, lane, 64, sync);
    if (lane == 0) B.cost[l] = it_cost(s_vals[wave]);
}

__device__ __forceinline__ void it_windows_chi2(const ItBatch& B, int w) {
    if (w < B.n_windows) B.chi2[w] = it_window_chi2(B.cost, B.win_link_off[w], B.win_link_off[w + 1]);
}

__global__ __launch_bounds__(256) void k_it_assemble(ItBatch B) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x >= B.n_keyframes) {
        it_windows_chi2(B, ((int)blockIdx.x - B.n_keyframes) * 256 + tid);
        return;
    }
    const int kf = blockIdx.x;
    if (tid >= kItSide) return;
    const double s = it_keyframe_entry(B.kf_items, B.kf_off[kf], B.kf_off[kf + 1], B.blocks, tid);
    if (tid < kItBlock) B.H_diag[(size_t)kf * kItBlock + tid] = s;
    else B.b[(size_t)kf * kItU + (tid - kItBlock)] = s;
}

__global__ __launch_bounds__(kItCostThreads) void k_it_cost(ItBatch B) {
    const int l = blockIdx.x * kItCostThreads + threadIdx.x;
    if (l >= B.n_links) return;
    const ItLink lk = B.links[l];
    ItVals v;
    it_link(B.pre[l], B.states[lk.kf1], B.states[lk.kf2], lk, B.huber_d, B.huber_dsqr, false, v, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1, ItNoSync());
    B.cost[l] = it_cost(v);
}

__global__ __launch_bounds__(256) void k_it_chi2(ItBatch B) { it_windows_chi2(B, blockIdx.x * 256 + threadIdx.x); }

void launch_inertial_term(const ItBatch& B, bool linearize, hipStream_t st) {
    const int window_blocks = (B.n_windows + 255) / 256;
    if (linearize) {
        if (B.n_links > 0) TC2LI_LAUNCH(k_it_link, dim3((B.n_links + kItLinkThreads / 64 - 1) / (kItLinkThreads / 64)), dim3(kItLinkThreads), 0, st, B);
        if (B.n_keyframes + window_blocks > 0) TC2LI_LAUNCH(k_it_assemble, dim3(B.n_keyframes + window_blocks), dim3(256), 0, st, B);
    } else {
        if (B.n_links > 0) TC2LI_LAUNCH(k_it_cost, dim3((B.n_links + kItCostThreads - 1) / kItCostThreads), dim3(kItCostThreads), 0, st, B);
        if (window_blocks > 0) TC2LI_LAUNCH(k_it_chi2, dim3(window_blocks), dim3(256), 0, st, B);
    }
}

}  // namespace tc2li

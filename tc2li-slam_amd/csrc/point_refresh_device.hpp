// What the kernels of LocalMapping::SearchInNeighbors (neighbors_kernels.hip) and LocalMapping::ProcessNewKeyFrame
// (process_keyframe_kernels.hip) do to one map point, in one copy: MapPoint::IsInKeyFrame on a row that ascends by keyframe,
// MapPoint::ComputeDistinctiveDescriptors by one wavefront, and MapPoint::UpdateNormalAndDepth by one lane.  A kernel hands in how it
// keeps its observation rows (a pool that is edited in place there, a CSR here) as small functions; the arithmetic and its order are here.
// Include after `#pragma clang fp contract(off)`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fuse_search.hpp"

namespace tc2li {
namespace refresh {

constexpr int kDescStride = 9;  // words per descriptor row in LDS: 8 + 1, so that lanes reading their own rows meet no bank twice

__device__ __forceinline__ void wave_sync_lds() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int lane_rank(unsigned long long mask) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}

// MapPoint::IsInKeyFrame (SF/src/MapPoint.cc:429-433): kf_at(k) is the keyframe of entry k of a row of len entries that ascends by
// keyframe.  -> the first entry whose keyframe is not below kf (len: none); the point is in kf when that entry's keyframe is kf.
template <class KfAt>
__device__ __forceinline__ int lower_bound_kf(int len, KfAt kf_at, int kf) {
    int lo = 0, hi = len;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (kf_at(mid) < kf) lo = mid + 1; else hi = mid; }
    return lo;
}
template <class KfAt>
__device__ __forceinline__ bool in_kf(int len, KfAt kf_at, int kf) {
    const int lo = lower_bound_kf(len, kf_at, kf);
    return lo < len && kf_at(lo) == kf;
}

// MapPoint::ComputeDistinctiveDescriptors (SF/src/MapPoint.cc:338-412) of a point with len observations, by the calling wavefront.
// kf_at(o): the keyframe of observation o; bad_kf(kf): isBad() (:361); desc_of(o): the 8 words of observation o's descriptor.  desc: the
// wavefront's len x kDescStride words of LDS, rows: which observation each row is.  -> the observation that wins (the first row with
// the least median, :397-401), -1: no descriptor to take (:352, :374); its words are desc[row * kDescStride ...] of the returned *row
// until the caller's next wave_sync_lds().  At most 256 observations (rows are bytes).
template <class KfAt, class BadKf, class DescOf>
__device__ __forceinline__ int describe_rows(int len, KfAt kf_at, BadKf bad_kf, DescOf desc_of, uint32_t* desc, uint8_t* rows, int lane, int* row) {
    int N = 0;
    for (int o0 = 0; o0 < len; o0 += 64) {
        const int o = o0 + lane;
        bool ok = false;
        if (o < len) ok = !bad_kf(kf_at(o));
        const unsigned long long mask = __ballot(ok);
        if (ok) {
            const int r = N + lane_rank(mask);
            rows[r] = (uint8_t)o;
            const uint32_t* d = desc_of(o);
#pragma unroll
            for (int k = 0; k < 8; ++k) desc[r * kDescStride + k] = d[k];
        }
        N += __popcll(mask);
    }
    if (N == 0) return -1;
    wave_sync_lds();
    int best_median = 0x7fffffff, best_row = 0x7fffffff;
    for (int i = lane; i < N; i += 64) {
        const int m = row_median(desc, kDescStride, N, i);
        if (m < best_median) { best_median = m; best_row = i; }  // rows of a lane ascend: the first minimum is kept
    }
    for (int o = 32; o >= 1; o >>= 1) {
        const int m = __shfl_xor(best_median, o, 64), r = __shfl_xor(best_row, o, 64);
        if (m < best_median || (m == best_median && r < best_row)) { best_median = m; best_row = r; }
    }
    *row = best_row;
    return rows[best_row];
}

// MapPoint::UpdateNormalAndDepth (SF/src/MapPoint.cc:435-503) of a point at X with N > 0 observations, by one lane, in the order of
// k_map_points_refresh: the order of the sum is the result.  centre_at(o): the camera centre of observation o's keyframe, bad ones
// included (:456-475); R: the centre of mpRefKF.
template <class CentreAt>
__device__ __forceinline__ void normal_and_depth(const float* X, int N, CentreAt centre_at, const float* R, float ref_scale, float last_level_scale,
                                                 float* normal3, float* min_dist, float* max_dist) {
    const float px = X[0], py = X[1], pz = X[2];
    float nx = 0, ny = 0, nz = 0;
    for (int o = 0; o < N; ++o) {
        const float* C = centre_at(o);
        const float vx = px - C[0], vy = py - C[1], vz = pz - C[2];
        const float nr = sqrtf(vx * vx + vy * vy + vz * vz);
        nx = nx + vx / nr; ny = ny + vy / nr; nz = nz + vz / nr;
    }
    const float rx = px - R[0], ry = py - R[1], rz = pz - R[2];
    const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
    const float mx = dist * ref_scale;                                       // :499
    *max_dist = mx;
    *min_dist = mx / last_level_scale;                                       // :500
    normal3[0] = nx / (float)N; normal3[1] = ny / (float)N; normal3[2] = nz / (float)N;   // :501
}

}  // namespace refresh
}  // namespace tc2li

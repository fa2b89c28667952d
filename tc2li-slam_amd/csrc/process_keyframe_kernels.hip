// LocalMapping::ProcessNewKeyFrame (SF/src/LocalMapping.cc:312-352) on gfx950: the association loop :326-345 of many keyframes at once
// (include/tc2li_hip.h "tc2li_process_new_keyframe_batch" states the rules).  The connection kernels (connections_kernels.hip) follow on
// the observation rows written here.
//   k_pkf_associate  one workgroup per problem.  Every slot of the current keyframe's row, one lane each: NULL and bad are skipped, the
//                    point's entry row is searched for the current keyframe (it ascends by keyframe: a bisection); a point that is not in
//                    takes the integer minimum of the slots that hold it -- the one fact of the loop that depends on its order.  The
//                    slot that is that minimum associates, every other slot of a point that is not bad pushes to the recent list; both
//                    lists are compacted in slot order with block_scan_excl.  Then the end-state rows: a point gains at most one
//                    observation, so their offsets are an exclusive sum over (entry length + associated), and each point's row is
//                    copied with the new pair put in at its place, by one lane.  The marks are words in global memory: no limit on
//                    the points of a problem.
//   k_pkf_refresh    one wavefront per associated point over the whole batch: ComputeDistinctiveDescriptors with the descriptor rows
//                    staged in LDS (9-word stride), UpdateNormalAndDepth as one lane's sequential float sum.  The grid is sized on the host
//                    by the occupied slots, the most points there can be; a wavefront past its problem's count leaves at once.
// A point that would pass kPkMaxObs observations ends the problem with status ON_HOST (its rows are still written, so the connection
// kernels read valid rows; the host twin computes the problem).  Every loop is bounded by a count fixed at launch, every output entry has
// one writer, no floating-point atomics.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "point_refresh_device.hpp"
#include "process_keyframe_device.hpp"

namespace tc2li {

__global__ __launch_bounds__(kPkThreads) void k_pkf_associate(PkBatch B) {
    __shared__ int scan[kPkThreads / 64];
    __shared__ int s_over;
    const int tid = threadIdx.x;
    const PkProblemDev P = B.problems[blockIdx.x];
    const int32_t* slot_point = B.slot_point + P.slot_off;
    const uint8_t* point_bad = B.point_bad + P.point_off;
    const int32_t* obs_offsets = B.obs_offsets + P.point_row_off;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int32_t* obs_index = B.obs_index + P.obs_off;
    int32_t* first_slot = B.first_slot + P.point_off;
    const int cur = P.current, n_slots = P.n_slots, n_points = P.n_points;

    if (tid == 0) s_over = 0;
    for (int p = tid; p < n_points; p += kPkThreads) {
        const size_t g = (size_t)P.point_off + p;
        first_slot[p] = kPkNoSlot;
        B.desc_kf[g] = -1; B.desc_index[g] = -1; B.refreshed[g] = 0;
        B.min_dist[g] = 0; B.max_dist[g] = 0;
        B.normals[3 * g] = 0; B.normals[3 * g + 1] = 0; B.normals[3 * g + 2] = 0;
    }
    __syncthreads();
    // ---- :326-333: which slots hold a point that is not in the current keyframe; the lowest such slot of every point ----
    for (int i = tid; i < n_slots; i += kPkThreads) {
        const int p = slot_point[i];
        if (p < 0 || point_bad[p]) continue;                                         // :329, :331
        const int32_t* row = obs_kf + obs_offsets[p];
        if (!refresh::in_kf(obs_offsets[p + 1] - obs_offsets[p], [=](int k) { return row[k]; }, cur)) atomicMin(&first_slot[p], i);   // :333
    }
    __syncthreads();
    // ---- the two lists in slot order (:335, :341) ----
    int32_t* associated_slot = B.associated_slot + P.list_off;
    int32_t* associated_point = B.associated_point + P.list_off;
    int32_t* recent = B.recent + P.list_off;
    int n_associated = 0, n_recent = 0;
    for (int base = 0; base < n_slots; base += kPkThreads) {
        const int i = base + tid;
        const int p = i < n_slots ? slot_point[i] : -1;
        int kind = 0;                                                                // 1 associates, 2 pushes
        if (p >= 0 && !point_bad[p]) kind = __hip_atomic_load(&first_slot[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == i ? 1 : 2;
        int tot;
        const int at = block_scan_excl<kPkThreads>((kind == 1 ? 1 : 0) | (kind == 2 ? 1 << 16 : 0), scan, &tot);   // at most 256 of each
        if (kind == 1) { const int a = n_associated + (at & 0xffff); associated_slot[a] = i; associated_point[a] = p; }
        if (kind == 2) recent[n_recent + (at >> 16)] = p;
        n_associated += tot & 0xffff;
        n_recent += tot >> 16;
    }
    // ---- the end state: AddObservation (MapPoint.cc:150-175) as one more entry at its place in the row ----
    int32_t* offsets_out = B.obs_offsets_out + P.point_row_off;
    int32_t* kf_out = B.obs_kf_out + P.obs_out_off;
    int32_t* index_out = B.obs_index_out + P.obs_out_off;
    int run = 0;
    for (int base = 0; base < n_points; base += kPkThreads) {
        const int p = base + tid;
        int len = 0, slot = kPkNoSlot, b = 0;
        if (p < n_points) {
            b = obs_offsets[p]; len = obs_offsets[p + 1] - b;
            slot = __hip_atomic_load(&first_slot[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        const int add = slot != kPkNoSlot ? 1 : 0;
        int tot;
        const int at = run + block_scan_excl<kPkThreads>(len + add, scan, &tot);
        if (p < n_points) {
            offsets_out[p] = at;
            int k = 0;
            if (add) {
                for (; k < len && obs_kf[b + k] < cur; ++k) { kf_out[at + k] = obs_kf[b + k]; index_out[at + k] = obs_index[b + k]; }
                kf_out[at + k] = cur; index_out[at + k] = slot;
                if (len + 1 > kPkMaxObs) s_over = 1;                                 // every writer stores the same value
            }
            for (; k < len; ++k) { kf_out[at + add + k] = obs_kf[b + k]; index_out[at + add + k] = obs_index[b + k]; }
            B.nobs_out[P.point_off + p] = B.nobs[P.point_off + p] + (add ? (P.u_right[slot] >= 0 ? 2 : 1) : 0);   // :171-174
        }
        run += tot;
    }
    __syncthreads();
    if (tid == 0) {
        offsets_out[n_points] = run;
        int32_t* counts = B.counts + kPkCounts * (size_t)blockIdx.x;
        counts[kPkStatus] = s_over ? TC2LI_PROCESS_KEYFRAME_ON_HOST : TC2LI_PROCESS_KEYFRAME_ON_DEVICE;
        counts[kPkAssociated] = n_associated; counts[kPkRecent] = n_recent; counts[kPkObs] = run;
    }
}

__global__ __launch_bounds__(64 * kPkRefreshWaves) void k_pkf_refresh(PkBatch B) {
    __shared__ uint32_t s_desc[kPkRefreshWaves][kPkMaxObs * refresh::kDescStride];
    __shared__ uint8_t s_rows[kPkRefreshWaves][kPkMaxObs];
    const int lane = threadIdx.x & 63, wave = wave_in_block();
    const int item = blockIdx.x * kPkRefreshWaves + wave;
    if (item >= B.n_items) return;                                                   // the whole wavefront: there is no barrier below
    int lo = 0, hi = B.n_problems - 1;                                               // the last problem whose first item is not past this one
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (B.problems[mid].item_off <= item) lo = mid; else hi = mid - 1; }
    const PkProblemDev& P = B.problems[lo];
    const int32_t* counts = B.counts + kPkCounts * (size_t)lo;
    const int k = item - P.item_off;
    if (counts[kPkStatus] != TC2LI_PROCESS_KEYFRAME_ON_DEVICE || k >= counts[kPkAssociated]) return;
    const int p = B.associated_point[P.list_off + k];
    const size_t g = (size_t)P.point_off + p;
    const int32_t* offsets = B.obs_offsets_out + P.point_row_off;
    const int at = offsets[p], len = offsets[p + 1] - at;                            // 1 .. kPkMaxObs: the point was associated
    const int32_t* row_kf = B.obs_kf_out + P.obs_out_off + at;
    const int32_t* row_index = B.obs_index_out + P.obs_out_off + at;
    const PkKf* kfs = B.kfs + P.kf_off;
    const uint8_t* kf_flags = B.kf_flags + P.kf_off;
    if (lane == 0) {                                                                 // :336
        refresh::normal_and_depth(B.positions + 3 * g, len, [=](int o) { return kfs[row_kf[o]].centre; }, kfs[B.ref_kf[g]].centre, B.ref_scale[g],
                                  P.last_level_scale, B.normals + 3 * g, B.min_dist + g, B.max_dist + g);
        B.refreshed[g] = 1;
    }
    int best_row;                                                                    // :337
    const int best = refresh::describe_rows(
        len, [=](int o) { return row_kf[o]; }, [=](int kf) { return (kf_flags[kf] & 1) != 0; },
        [=](int o) { return reinterpret_cast<const uint32_t*>(kfs[row_kf[o]].desc) + 8 * (size_t)row_index[o]; }, s_desc[wave], s_rows[wave], lane, &best_row);
    if (best >= 0 && lane == 0) { B.desc_kf[g] = row_kf[best]; B.desc_index[g] = row_index[best]; }
}

void launch_process_keyframe(const PkBatch& B, hipStream_t st) {
    if (B.n_problems <= 0) return;
    TC2LI_LAUNCH(k_pkf_associate, dim3(B.n_problems), dim3(kPkThreads), 0, st, B);
    if (B.n_items > 0) TC2LI_LAUNCH(k_pkf_refresh, dim3((B.n_items + kPkRefreshWaves - 1) / kPkRefreshWaves), dim3(64 * kPkRefreshWaves), 0, st, B);
}

}  // namespace tc2li

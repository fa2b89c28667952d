// An edit log applied to the resident map graph on gfx950 (include/tc2li_hip.h "the map graph resident on the device"; the edits stand
// for KeyFrame::SetPose / SetBadFlag / AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch, SF/src/KeyFrame.cc:121, :585, :309-340,
// and MapPoint::AddObservation / EraseObservation / SetBadFlag / SetWorldPos, SF/src/MapPoint.cc:150-210, :225).  Integer work and
// copies.  map_graph_host.cpp has checked every edit against the resident sizes before the launch: no index read here is unchecked.
//   k_mg_apply   one workgroup per sequence, the log in steps of 256 edits in log order:
//                appends        ADD_KEYFRAME / ADD_POINT: the new row is the old count + the appends before the edit, a block prefix sum per
//                               step; the new keyframes' slot rows are one stretch at the end of slot_point, filled with -1.
//                overwrites     flags, poses, positions, slots.  They run after the appends (the host refuses a row named before its
//                               append, so log order is kept).  Last writer wins: inside a step an edit yields when a later edit of the
//                               step names the same cell (the cells of the step are in LDS), and a barrier parts the steps.
//                observations   every edit does atomicMin / atomicMax of its number on its point: the touched rows and the stretch of the
//                               log that holds their edits.  The touched rows are compacted (block prefix sum); a wavefront per touched
//                               row copies the old row -- into LDS up to kMgLdsRow entries (old + the row's ADD edits), into the staging
//                               table in global memory beyond -- and applies the row's edits in log order: the place by a count over the
//                               lanes, the shift by the lanes in steps of 64 from the far end.  The merged row goes to the staging table.
//                offsets        a block prefix sum over the new lengths gives the other generation's obs_offsets.
//   k_mg_write   kMgWriteBlocks workgroups per sequence, a thread per entry of the new CSR: its row by bisection of the new offsets, the
//                entry from the old CSR (an untouched row: neighbours read and write neighbours) or from the staging table.
// Two launches whatever the edits and sequences.  Every loop runs to a bound the host checked; no workgroup waits for another.
#include "launch.hpp"
#include "map_graph_device.hpp"

namespace tc2li {
namespace {

constexpr int kMgUntouched = 0x7fffffff;

__device__ __forceinline__ bool mg_is_obs(int op) {
    return op == TC2LI_MAP_GRAPH_ADD_OBSERVATION || op == TC2LI_MAP_GRAPH_ERASE_OBSERVATION || op == TC2LI_MAP_GRAPH_CLEAR_OBSERVATIONS;
}

// A row under merge in LDS: the wavefront's own stretch, plain accesses.  settle() parts two edits: what one lane wrote another reads.
struct MgRowLds {
    int *kf, *index;
    __device__ __forceinline__ int ld_kf(int j) const { return kf[j]; }
    __device__ __forceinline__ int ld_index(int j) const { return index[j]; }
    __device__ __forceinline__ void st(int j, int k, int i) const { kf[j] = k; index[j] = i; }
    __device__ __forceinline__ void st_index(int j, int i) const { index[j] = i; }
    __device__ __forceinline__ void settle() const { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
};
// The same in the staging table: loads and stores that pass by the L1, and a wait for the stores before the next edit's loads.
struct MgRowGlobal {
    int *kf, *index;
    __device__ __forceinline__ int ld_kf(int j) const { return __hip_atomic_load(kf + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int ld_index(int j) const { return __hip_atomic_load(index + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void st(int j, int k, int i) const {
        __hip_atomic_store(kf + j, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(index + j, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __device__ __forceinline__ void st_index(int j, int i) const { __hip_atomic_store(index + j, i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ void settle() const { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
};

// The edits e0 .. e1 of the log that name point p, applied in order to the row of `len` entries in R by one wavefront, all 64 lanes
// arriving.  Returns the new length.  The row has room for len + the ADD edits among them.
template <class Row>
__device__ __forceinline__ int mg_merge_row(const Row& R, int len, const tc2li_map_graph_edit* edits, int e0, int e1, int p) {
    const int lane = threadIdx.x & 63;
    for (int e = e0; e <= e1; ++e) {
        const int op = __builtin_amdgcn_readfirstlane(edits[e].op), a = __builtin_amdgcn_readfirstlane(edits[e].a);
        if (!mg_is_obs(op) || a != p) continue;
        if (op == TC2LI_MAP_GRAPH_CLEAR_OBSERVATIONS) { len = 0; continue; }              // mObservations.clear()
        const int k = __builtin_amdgcn_readfirstlane(edits[e].b), idx = __builtin_amdgcn_readfirstlane(edits[e].c);
        int less = 0, equal = 0;
        for (int j = lane; j < len; j += 64) {
            const int v = R.ld_kf(j);
            less += v < k ? 1 : 0;
            equal += v == k ? 1 : 0;
        }
        const int at = wave_sum_i32(less);                                               // the rows ascend strictly: the pair's place
        const bool present = wave_sum_i32(equal) != 0;
        if (op == TC2LI_MAP_GRAPH_ADD_OBSERVATION) {
            if (present) {                                                               // mObservations[pKF] = indexes (MapPoint.cc:155-169)
                if (lane == 0) R.st_index(at, idx);
            } else {
                // [at, len) one to the right, 64 entries at a time from the far end: a step reads all its entries before it writes any
                // (the stores carry what the loads returned), and the next step reads only below what this one wrote
                for (int hi = len; hi > at; hi -= 64) {
                    const int j = hi - 1 - lane;
                    int tk = 0, ti = 0;
                    if (j >= at) { tk = R.ld_kf(j); ti = R.ld_index(j); }
                    R.settle();
                    if (j >= at) R.st(j + 1, tk, ti);
                }
                R.settle();
                if (lane == 0) R.st(at, k, idx);
                ++len;
            }
        } else if (present) {                                                            // EraseObservation; absent: a no-op (MapPoint.cc:182)
            for (int lo = at + 1; lo < len; lo += 64) {
                const int j = lo + lane;
                int tk = 0, ti = 0;
                if (j < len) { tk = R.ld_kf(j); ti = R.ld_index(j); }
                R.settle();
                if (j < len) R.st(j - 1, tk, ti);
            }
            --len;
        }
        R.settle();
    }
    return len;
}

__global__ __launch_bounds__(kMgThreads) void k_mg_apply(MgApplyBatch B) {
    __shared__ int scan[kMgThreads / 64];
    __shared__ int cell_kind[kMgThreads], cell_row[kMgThreads], cell_sub[kMgThreads];
    __shared__ int row_kf[kMgThreads / 64][kMgLdsRow], row_index[kMgThreads / 64][kMgLdsRow];
    __shared__ int staged;
    const MgApplyDev& D = B.deltas[blockIdx.x];
    const MgTables& T = B.T;
    const int tid = threadIdx.x, lane = tid & 63, w = wave_in_block();
    const size_t seq = (size_t)D.sequence;
    const tc2li_map_graph_edit* edits = B.edits + D.edit_off;
    const double* values = B.values + D.value_off;
    const int n_edits = D.n_edits;
    int32_t* kf_slot = T.kf_slot + seq * T.cap_kf;
    int64_t* kf_id = T.kf_id + seq * T.cap_kf;
    uint8_t* kf_flags = T.kf_flags + seq * T.cap_kf;
    double* poses7 = T.poses7 + seq * T.cap_kf * 7;
    int32_t* slot_offsets = T.slot_offsets + seq * ((size_t)T.cap_kf + 1);
    int32_t* slot_point = T.slot_point + seq * T.cap_slot;
    uint8_t* point_flags = T.point_flags + seq * T.cap_pt;
    double* positions = T.positions + seq * T.cap_pt * 3;
    const size_t g_old = seq * 2 + (size_t)D.generation, g_new = seq * 2 + (size_t)(D.generation ^ 1);
    const int32_t* old_off = T.obs_offsets + g_old * ((size_t)T.cap_pt + 1);
    const int32_t* old_kf = T.obs_kf + g_old * T.cap_obs;
    const int32_t* old_index = T.obs_index + g_old * T.cap_obs;
    int32_t* new_off = T.obs_offsets + g_new * ((size_t)T.cap_pt + 1);
    int32_t* head = T.pt_head + seq * T.cap_pt;
    int32_t* last = T.pt_last + seq * T.cap_pt;
    int32_t* new_len = T.pt_len + seq * T.cap_pt;
    int32_t* stage_at = T.pt_stage + seq * T.cap_pt;
    int32_t* touched = T.touched + seq * T.cap_pt;
    int32_t* stage_kf = T.stage_kf + seq * T.cap_obs;
    int32_t* stage_index = T.stage_index + seq * T.cap_obs;
    const int n_points = D.n_points_new;

    for (int p = tid; p < n_points; p += kMgThreads) { head[p] = kMgUntouched; last[p] = -1; stage_at[p] = 0; }
    if (tid == 0) staged = 0;

    // appends
    int n_kf = D.n_kf, n_pt = D.n_points, n_slot = D.n_slot;
    for (int base = 0; base < n_edits; base += kMgThreads) {
        const int e = base + tid;
        tc2li_map_graph_edit ed{-1, 0, 0, 0};
        if (e < n_edits) ed = edits[e];
        const bool keyframe = ed.op == TC2LI_MAP_GRAPH_ADD_KEYFRAME, point = ed.op == TC2LI_MAP_GRAPH_ADD_POINT;
        int tot, tot_slots;
        const int at = block_scan_excl<kMgThreads>((keyframe ? 1 : 0) | (point ? 1 << 16 : 0), scan, &tot);   // at most 256 of each
        const int at_slots = block_scan_excl<kMgThreads>(keyframe ? ed.b : 0, scan, &tot_slots);
        if (keyframe) {                                                                  // new KeyFrame (Tracking.cc:3078)
            const int row = n_kf + (at & 0xffff);
            const double* v = values + ed.c;
            kf_slot[row] = ed.a;
            kf_id[row] = (int64_t)v[0];
            kf_flags[row] = (uint8_t)(int)v[1];
#pragma unroll
            for (int c = 0; c < 7; ++c) poses7[(size_t)row * 7 + c] = v[2 + c];
            slot_offsets[row + 1] = n_slot + at_slots + ed.b;
        }
        if (point) {                                                                     // new MapPoint
            const int row = n_pt + (at >> 16);
            point_flags[row] = (uint8_t)ed.a;
#pragma unroll
            for (int c = 0; c < 3; ++c) positions[(size_t)row * 3 + c] = values[ed.b + c];
        }
        n_kf += tot & 0xffff; n_pt += tot >> 16; n_slot += tot_slots;
    }
    for (int s = D.n_slot + tid; s < n_slot; s += kMgThreads) slot_point[s] = -1;
    __syncthreads();

    // overwrites, the last writer of a cell winning
    for (int base = 0; base < n_edits; base += kMgThreads) {
        const int e = base + tid;
        tc2li_map_graph_edit ed{-1, 0, 0, 0};
        if (e < n_edits) ed = edits[e];
        const bool cell = ed.op == TC2LI_MAP_GRAPH_SET_KEYFRAME_FLAGS || ed.op == TC2LI_MAP_GRAPH_SET_POSE || ed.op == TC2LI_MAP_GRAPH_SET_POINT_FLAGS ||
                          ed.op == TC2LI_MAP_GRAPH_SET_POSITION || ed.op == TC2LI_MAP_GRAPH_SET_SLOT;
        const int kind = cell ? ed.op : -1, sub = ed.op == TC2LI_MAP_GRAPH_SET_SLOT ? ed.b : 0;
        cell_kind[tid] = kind; cell_row[tid] = ed.a; cell_sub[tid] = sub;
        __syncthreads();
        bool wins = cell;
        for (int j = tid + 1; j < kMgThreads && wins; ++j) wins = !(cell_kind[j] == kind && cell_row[j] == ed.a && cell_sub[j] == sub);
        if (wins) {
            switch (ed.op) {
                case TC2LI_MAP_GRAPH_SET_KEYFRAME_FLAGS: kf_flags[ed.a] = (uint8_t)ed.b; break;      // KeyFrame::SetBadFlag (KeyFrame.cc:585)
                case TC2LI_MAP_GRAPH_SET_POSE:                                                       // KeyFrame::SetPose (KeyFrame.cc:121)
                    for (int c = 0; c < 7; ++c) poses7[(size_t)ed.a * 7 + c] = values[ed.b + c];
                    break;
                case TC2LI_MAP_GRAPH_SET_POINT_FLAGS: point_flags[ed.a] = (uint8_t)ed.b; break;      // MapPoint::SetBadFlag (MapPoint.cc:225)
                case TC2LI_MAP_GRAPH_SET_POSITION:                                                   // MapPoint::SetWorldPos
                    for (int c = 0; c < 3; ++c) positions[(size_t)ed.a * 3 + c] = values[ed.b + c];
                    break;
                default: slot_point[slot_offsets[ed.a] + ed.b] = ed.c; break;                        // KeyFrame.cc:309-340
            }
        }
        __syncthreads();
    }

    // the observation rows the log touches, and where in the log
    for (int e = tid; e < n_edits; e += kMgThreads) {
        const int op = edits[e].op, p = edits[e].a;
        if (!mg_is_obs(op)) continue;
        atomicMin(&head[p], e);
        atomicMax(&last[p], e);
        if (op == TC2LI_MAP_GRAPH_ADD_OBSERVATION) atomicAdd(&stage_at[p], 1);
    }
    __syncthreads();
    int n_touched = 0;
    for (int base = 0; base < n_points; base += kMgThreads) {
        const int p = base + tid;
        const bool is_touched = p < n_points && head[p] != kMgUntouched;
        int tot;
        const int at = block_scan_excl<kMgThreads>(is_touched ? 1 : 0, scan, &tot);
        if (is_touched) touched[n_touched + at] = p;
        else if (p < n_points) new_len[p] = p < D.n_points ? old_off[p + 1] - old_off[p] : 0;
        n_touched += tot;
    }
    __syncthreads();

    // a wavefront per touched row
    for (int i = w; i < n_touched; i += kMgThreads / 64) {
        const int p = __builtin_amdgcn_readfirstlane(touched[i]);
        const int o0 = p < D.n_points ? __builtin_amdgcn_readfirstlane(old_off[p]) : 0;
        const int len0 = p < D.n_points ? __builtin_amdgcn_readfirstlane(old_off[p + 1]) - o0 : 0;
        const int room = len0 + __builtin_amdgcn_readfirstlane(stage_at[p]);             // the host: the sum of these is within cap_obs
        int at = 0;
        if (lane == 0) at = atomicAdd(&staged, room);
        at = __builtin_amdgcn_readfirstlane(at);
        const int e0 = __builtin_amdgcn_readfirstlane(head[p]), e1 = __builtin_amdgcn_readfirstlane(last[p]);
        int len;
        if (room <= kMgLdsRow) {
            const MgRowLds R{row_kf[w], row_index[w]};
            for (int j = lane; j < len0; j += 64) R.st(j, old_kf[o0 + j], old_index[o0 + j]);
            R.settle();
            len = mg_merge_row(R, len0, edits, e0, e1, p);
            for (int j = lane; j < len; j += 64) { stage_kf[at + j] = R.ld_kf(j); stage_index[at + j] = R.ld_index(j); }
            R.settle();
        } else {
            const MgRowGlobal R{stage_kf + at, stage_index + at};
            for (int j = lane; j < len0; j += 64) R.st(j, old_kf[o0 + j], old_index[o0 + j]);
            R.settle();
            len = mg_merge_row(R, len0, edits, e0, e1, p);
        }
        if (lane == 0) { new_len[p] = len; stage_at[p] = at; }
    }
    __syncthreads();

    // the new offsets
    int total = 0;
    for (int base = 0; base < n_points; base += kMgThreads) {
        const int p = base + tid;
        int tot;
        const int at = block_scan_excl<kMgThreads>(p < n_points ? new_len[p] : 0, scan, &tot);
        if (p < n_points) new_off[p] = total + at;
        total += tot;
    }
    if (tid == 0) { new_off[n_points] = total; B.totals[blockIdx.x] = total; }
}

__global__ __launch_bounds__(kMgThreads) void k_mg_write(MgApplyBatch B) {
    const MgApplyDev& D = B.deltas[blockIdx.x];
    const MgTables& T = B.T;
    const size_t seq = (size_t)D.sequence;
    const size_t g_old = seq * 2 + (size_t)D.generation, g_new = seq * 2 + (size_t)(D.generation ^ 1);
    const int32_t* old_off = T.obs_offsets + g_old * ((size_t)T.cap_pt + 1);
    const int32_t* old_kf = T.obs_kf + g_old * T.cap_obs;
    const int32_t* old_index = T.obs_index + g_old * T.cap_obs;
    const int32_t* new_off = T.obs_offsets + g_new * ((size_t)T.cap_pt + 1);
    int32_t* new_kf = T.obs_kf + g_new * T.cap_obs;
    int32_t* new_index = T.obs_index + g_new * T.cap_obs;
    const int32_t* head = T.pt_head + seq * T.cap_pt;
    const int32_t* stage_at = T.pt_stage + seq * T.cap_pt;
    const int32_t* stage_kf = T.stage_kf + seq * T.cap_obs;
    const int32_t* stage_index = T.stage_index + seq * T.cap_obs;
    const int n_points = D.n_points_new;
    const int total = new_off[n_points];
    for (int j = blockIdx.y * kMgThreads + threadIdx.x; j < total; j += kMgWriteBlocks * kMgThreads) {
        int lo = 0, hi = n_points;                                                       // the last row whose offset is <= j: at most 31 steps
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (new_off[mid] <= j) lo = mid; else hi = mid;
        }
        const int r = j - new_off[lo];
        if (head[lo] != kMgUntouched) { new_kf[j] = stage_kf[stage_at[lo] + r]; new_index[j] = stage_index[stage_at[lo] + r]; }
        else { new_kf[j] = old_kf[old_off[lo] + r]; new_index[j] = old_index[old_off[lo] + r]; }
    }
}

}  // namespace

void launch_map_graph_apply(const MgApplyBatch& B, hipStream_t st) {
    if (B.n <= 0) return;
    TC2LI_LAUNCH(k_mg_apply, dim3(B.n), dim3(kMgThreads), 0, st, B);
    TC2LI_LAUNCH(k_mg_write, dim3(B.n, kMgWriteBlocks), dim3(kMgThreads), 0, st, B);
}

}  // namespace tc2li

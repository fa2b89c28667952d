// KeyFrame::UpdateConnections / AddConnection / UpdateBestCovisibles of local mapping on gfx950 (SF/src/KeyFrame.cc:391-486, :201-238).
// Integer work over the flat graph: votes into a histogram, a threshold, and lists ordered by a 64-bit key; no float, no MFMA.
//   k_conn_vote        one workgroup per problem.  Groups of 16 lanes take one slot each and walk the point's observation row together
//                      (rows are 10-20 entries: one or two 64-byte reads); every vote is an integer atomic add on the keyframe's counter,
//                      in LDS up to kConnLdsKeyframes keyframes and in global memory beyond.  Integer sums do not depend on their order.
//                      The counters are then compacted in row order (KFcounter = the new weight map; those with at least 15 votes, or the
//                      maximum alone, are the touched keyframes), the current keyframe's lists are ordered by ranking, and every touched
//                      keyframe's row is looked through by one wavefront: does it hold (current, weight) already, and how long is its
//                      new list.  A prefix sum over those lengths is the CSR of the changed neighbours.
//   k_conn_neighbours  one wavefront per (problem, touched keyframe) with changed = 1: its row with the entry of the current keyframe
//                      overwritten or added, bad keyframes dropped, ordered by ranking.
//   k_best_covisibles  one wavefront per row: the same ordering for tc2li_update_best_covisibles_batch.
// Ranking (rank_emit): an entry's place is the number of entries with a greater (weight, row) key -- std::sort's result read from the
// back, because the keys are distinct.  The keys of 64 entries are loaded once, one per lane, and then read lane by lane as scalars
// (readlane: no LDS, no bank conflicts), so a list of n entries costs n / 64 loads and n compares per lane and group of 64 places.
// The wavefront's number is taken as a scalar (wave_in_block) where loop bounds derive from it: all 64 lanes must be active at a readlane.
#include "connections_device.hpp"
#include "launch.hpp"

namespace tc2li {

// Orders n entries: entry i has the key key_of(i) (0: not in the list) and goes to the place that is the number of greater keys.
// wave / n_waves: the wavefronts that share the work, each takes whole groups of 64 places.  Every lane of the wavefront must call it.
template <class KeyOf>
__device__ __forceinline__ void rank_emit(int n, KeyOf key_of, int32_t* out_kf, int32_t* out_weight, int wave, int n_waves) {
    const int lane = threadIdx.x & 63;
    for (int ib = wave * 64; ib < n; ib += 64 * n_waves) {
        const int i = ib + lane;
        const uint64_t ki = i < n ? key_of(i) : 0;
        int r = 0;
        for (int jb = 0; jb < n; jb += 64) {
            const int j = jb + lane;
            const uint64_t kj = j < n ? key_of(j) : 0;
            const int lo = (int)(uint32_t)kj, hi = (int)(uint32_t)(kj >> 32);
#pragma unroll
            for (int t = 0; t < 64; ++t) {
                const uint64_t s = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane(hi, t) << 32) | (uint32_t)__builtin_amdgcn_readlane(lo, t);
                r += s > ki;
            }
        }
        if (ki) { out_kf[r] = conn::key_kf(ki); out_weight[r] = conn::key_weight(ki); }
    }
}

// KeyFrame::UpdateBestCovisibles (:216-238) by one wavefront: the row's entries, with the weight of keyframe `cur` replaced by cur_weight
// and -- append -- that entry added at the end; keyframes whose flag has a bit of bad_mask are left out (:229).
__device__ __forceinline__ void best_covisibles(const int32_t* row_kf, const int32_t* row_weight, int n_row, const uint8_t* flags, int bad_mask,
                                                int cur, int cur_weight, bool append, int32_t* out_kf, int32_t* out_weight) {
    auto key_of = [=](int j) -> uint64_t {
        const int kf = j < n_row ? row_kf[j] : cur;
        if (flags[kf] & bad_mask) return 0;
        return conn::key(kf == cur ? cur_weight : row_weight[j], kf);
    };
    rank_emit(n_row + (append ? 1 : 0), key_of, out_kf, out_weight, 0, 1);
}

// hist: the problem's counters, LDS or global (the address space is known after inlining)
__device__ __forceinline__ void conn_problem(const ConnBatch& B, const ConnProblemDev& P, int* hist, int* scan, unsigned long long* best) {
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int32_t* slot_point = B.slot_point + P.slot_off;
    const uint8_t* point_bad = B.point_bad + P.point_off;
    const int32_t* obs_row = B.obs_offsets + P.obs_row_off;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int cur = P.current;
    int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_CONNECTIONS_COUNTS;
    for (int k = tid; k < P.n_kf; k += kConnThreads) hist[k] = 0;
    if (tid == 0) *best = 0;
    __syncthreads();
    // votes (:404-423)
    const int sub = tid & 15;
    for (int s = tid >> 4; s < P.n_slots; s += kConnThreads / 16) {
        const int p = slot_point[s];
        if (p < 0 || point_bad[p]) continue;                                         // :408, :411
        const int o1 = obs_row[p + 1];
        for (int o = obs_row[p] + sub; o < o1; o += 16) {
            const int kf = obs_kf[o];
            if (kf != cur && !(flags[kf] & 3)) atomicAdd(&hist[kf], 1);              // :418-420
        }
    }
    __syncthreads();
    // KFcounter in map order, vPairs of :448-452 (= the touched keyframes), the maximum of :443-447
    int32_t* counter_kf = B.counter_kf + P.counter_off;
    int32_t* counter_weight = B.counter_weight + P.counter_off;
    int32_t* touched_kf = B.touched_kf + P.ordered_off;
    int32_t* touched_weight = B.touched_weight + P.ordered_off;
    int n_counter = 0, n_pairs = 0;
    unsigned long long mine = 0;
    for (int base = 0; base < P.n_kf; base += kConnThreads) {
        const int k = base + tid;
        const int c = k < P.n_kf ? hist[k] : 0;
        int tot;
        const int at = block_scan_excl<kConnThreads>((c > 0 ? 1 : 0) | (c >= TC2LI_CONNECTIONS_TH ? 1 << 16 : 0), scan, &tot);   // at most 256 of each
        const int a = n_counter + (at & 0xffff), b = n_pairs + (at >> 16);
        if (c > 0 && a < P.counter_cap) { counter_kf[a] = k; counter_weight[a] = c; }
        if (c >= TC2LI_CONNECTIONS_TH && b < P.ordered_cap) { touched_kf[b] = k; touched_weight[b] = c; }
        n_counter += tot & 0xffff;
        n_pairs += tot >> 16;
        if (c > 0) {                                                                 // most votes, the lowest row among equals
            const unsigned long long m = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0x7fffffff - k);
            mine = m > mine ? m : mine;
        }
    }
    if (n_counter == 0) {                                                            // :426-427
        if (tid < TC2LI_CONNECTIONS_COUNTS) counts[tid] = tid == TC2LI_CONNECTIONS_PARENT ? -1 : 0;
        return;
    }
    if (n_pairs == 0) {                                                              // :455-459
        if (mine) atomicMax(best, mine);
        __syncthreads();
        const unsigned long long m = *best;
        n_pairs = 1;
        if (tid == 0 && P.ordered_cap > 0) { touched_kf[0] = 0x7fffffff - (int)(uint32_t)m; touched_weight[0] = (int)(m >> 32); }
    }
    if (n_counter > P.counter_cap || n_pairs > P.ordered_cap) {                      // the host answers TC2LI_ERR_CAPACITY from these sizes
        if (tid < TC2LI_CONNECTIONS_COUNTS)
            counts[tid] = tid == TC2LI_CONNECTIONS_STATUS ? TC2LI_CONNECTIONS_UPDATED : tid == TC2LI_CONNECTIONS_N_COUNTER ? n_counter
                        : tid == TC2LI_CONNECTIONS_N_ORDERED ? n_pairs : tid == TC2LI_CONNECTIONS_PARENT ? -1 : 0;
        return;
    }
    __syncthreads();   // touched_* are read by other lanes from here on
    // own lists (:461-475)
    int32_t* ordered_kf = B.ordered_kf + P.ordered_off;
    rank_emit(n_pairs, [=](int j) { return conn::key(touched_weight[j], touched_kf[j]); }, ordered_kf, B.ordered_weight + P.ordered_off,
              wave, kConnThreads / 64);
    // AddConnection in every touched keyframe (:201-211): is the entry there with this weight, and how many entries will its list have
    const int32_t* conn_row = B.conn_offsets + P.conn_row_off;
    const int32_t* conn_kf = B.conn_kf + P.conn_off;
    const int32_t* conn_weight = B.conn_weight + P.conn_off;
    uint8_t* touched_changed = B.touched_changed + P.ordered_off;
    int32_t* item_off = B.item_off + P.ordered_off;
    uint8_t* item_found = B.item_found + P.ordered_off;
    const int cur_alive = (flags[cur] & 1) ? 0 : 1;
    for (int i = wave; i < n_pairs; i += kConnThreads / 64) {
        const int k = touched_kf[i], w = touched_weight[i];
        const int r1 = conn_row[k + 1];
        int alive = 0, found = 0, held = 0;
        for (int j = conn_row[k] + lane; j < r1; j += 64) {
            const int kk = conn_kf[j];
            if (kk == cur) { found = 1; held = conn_weight[j]; }
            else alive += (flags[kk] & 1) ? 0 : 1;
        }
        alive = wave_sum_i32(alive);
        held = wave_sum_i32(found ? held : 0);                                       // at most one lane found it: the rows ascend strictly
        found = wave_sum_i32(found);
        const bool changed = !(found && held == w);                                  // :205-210
        if (lane == 0) { touched_changed[i] = changed; item_found[i] = found; item_off[i] = changed ? alive + cur_alive : 0; }
    }
    __syncthreads();
    // the CSR over the changed ones
    int32_t* changed_offsets = B.changed_offsets + P.ordered_off + blockIdx.x;
    int n_changed = 0, n_entries = 0;
    for (int base = 0; base < n_pairs; base += kConnThreads) {
        const int i = base + tid;
        const int changed = i < n_pairs ? touched_changed[i] : 0;
        const int len = i < n_pairs ? item_off[i] : 0;
        int tot_c, tot_l;
        const int c = n_changed + block_scan_excl<kConnThreads>(changed, scan, &tot_c);
        const int o = n_entries + block_scan_excl<kConnThreads>(len, scan, &tot_l);
        if (i < n_pairs) item_off[i] = changed ? o : -1;
        if (changed) changed_offsets[c] = o;
        n_changed += tot_c;
        n_entries += tot_l;
    }
    if (tid == 0) {
        changed_offsets[n_changed] = n_entries;
        counts[TC2LI_CONNECTIONS_STATUS] = TC2LI_CONNECTIONS_UPDATED;
        counts[TC2LI_CONNECTIONS_N_COUNTER] = n_counter;
        counts[TC2LI_CONNECTIONS_N_ORDERED] = n_pairs;
        counts[TC2LI_CONNECTIONS_N_CHANGED] = n_changed;
        counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] = n_entries;
        counts[TC2LI_CONNECTIONS_PARENT] = (P.flags & 3) == 1 ? ordered_kf[0] : -1;  // :478-483; ordered_kf: before the barrier above
        counts[6] = 0;
        counts[7] = 0;
    }
}

__global__ __launch_bounds__(kConnThreads) void k_conn_vote(ConnBatch B) {
    __shared__ int hist[kConnLdsKeyframes];
    __shared__ int scan[kConnThreads / 64];
    __shared__ unsigned long long best;
    const ConnProblemDev& P = B.problems[blockIdx.x];
    if (P.hist_off < 0) conn_problem(B, P, hist, scan, &best);
    else conn_problem(B, P, B.hist + P.hist_off, scan, &best);
}

__global__ __launch_bounds__(kConnRankLanes) void k_conn_neighbours(ConnBatch B) {
    const int e = blockIdx.x;
    const int p = B.problem_of_item[e];
    const ConnProblemDev& P = B.problems[p];
    const int32_t* counts = B.counts + (size_t)p * TC2LI_CONNECTIONS_COUNTS;
    const int i = e - P.ordered_off;
    // the whole wavefront leaves together: nothing to do, or a list of the problem did not fit
    if (counts[TC2LI_CONNECTIONS_N_COUNTER] > P.counter_cap || counts[TC2LI_CONNECTIONS_N_ORDERED] > P.ordered_cap ||
        counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] > P.changed_cap || i >= counts[TC2LI_CONNECTIONS_N_ORDERED])
        return;
    const int off = B.item_off[e];
    if (off < 0) return;
    const int k = B.touched_kf[e];
    const int32_t* conn_row = B.conn_offsets + P.conn_row_off;
    const int r0 = conn_row[k], r1 = conn_row[k + 1];
    best_covisibles(B.conn_kf + P.conn_off + r0, B.conn_weight + P.conn_off + r0, r1 - r0, B.kf_flags + P.kf_off, 1, P.current, B.touched_weight[e],
                    !B.item_found[e], B.changed_kf + P.changed_off + off, B.changed_weight + P.changed_off + off);
}

__global__ __launch_bounds__(256) void k_best_covisibles(CovisBatch B) {
    const int row = blockIdx.x * 4 + wave_in_block();
    if (row >= B.n_rows) return;
    const int lane = threadIdx.x & 63;
    const int r0 = B.row_offsets[row], r1 = B.row_offsets[row + 1];
    int alive = 0;
    for (int j = r0 + lane; j < r1; j += 64) alive += B.bad[B.row_kf[j]] ? 0 : 1;
    alive = wave_sum_i32(alive);
    if (lane == 0) B.out_count[row] = alive;
    best_covisibles(B.row_kf + r0, B.row_weight + r0, r1 - r0, B.bad, 0xff, -1, 0, false, B.out_kf + r0, B.out_weight + r0);
}

void launch_update_connections(const ConnBatch& B, hipStream_t st) {
    if (B.n_problems > 0) TC2LI_LAUNCH(k_conn_vote, dim3(B.n_problems), dim3(kConnThreads), 0, st, B);
    if (B.n_items > 0) TC2LI_LAUNCH(k_conn_neighbours, dim3(B.n_items), dim3(kConnRankLanes), 0, st, B);
}

void launch_update_best_covisibles(const CovisBatch& B, hipStream_t st) {
    if (B.n_rows > 0) TC2LI_LAUNCH(k_best_covisibles, dim3((B.n_rows + 3) / 4), dim3(256), 0, st, B);
}

}  // namespace tc2li

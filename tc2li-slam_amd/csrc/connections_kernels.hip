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
#include "map_graph_device.hpp"

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

// The CSR over the touched keyframes with changed = 1: item_off holds every touched keyframe's new list length (0: unchanged) and gets
// where its list starts (-1: unchanged).  Every thread of the workgroup must call it.
__device__ __forceinline__ void changed_csr(const uint8_t* touched_changed, int32_t* item_off, int32_t* changed_offsets, int n_pairs, int* scan,
                                            int* n_changed_out, int* n_entries_out) {
    const int tid = threadIdx.x;
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
    if (tid == 0) changed_offsets[n_changed] = n_entries;
    *n_changed_out = n_changed;
    *n_entries_out = n_entries;
}

// hist: the problem's counters, LDS or global (the address space is known after inlining).  kPointBad: the bits of point_bad that mean
// isBad() -- any for the host's arrays, bit 0 for the point_flags of the resident graph.
template <int kPointBad>
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
        if (p < 0 || (point_bad[p] & kPointBad)) continue;                           // :408, :411
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
    int n_changed, n_entries;
    changed_csr(touched_changed, item_off, changed_offsets, n_pairs, scan, &n_changed, &n_entries);
    if (tid == 0) {
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
    if (P.hist_off < 0) conn_problem<0xff>(B, P, hist, scan, &best);
    else conn_problem<0xff>(B, P, B.hist + P.hist_off, scan, &best);
}

// item e of problem p, by one wavefront
__device__ __forceinline__ void conn_neighbour(const ConnBatch& B, int p, int e) {
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

__global__ __launch_bounds__(kConnRankLanes) void k_conn_neighbours(ConnBatch B) {
    conn_neighbour(B, B.problem_of_item[blockIdx.x], blockIdx.x);
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

// ---- the same calls on the resident map graph (map_graph_device.hpp "the covisibility graph of the resident map"; tc2li_hip.h
// tc2li_map_graph_update_connections_batch / tc2li_map_graph_erase_connections_batch) ----------------------------------------------------
//   k_mgc_vote         one workgroup per sequence.  Builds the sequence's ConnProblemDev from its 64-byte record -- the tables are the
//                      resident ones, the outputs a scratch that can hold the largest lists -- and runs conn_problem on it: the vote, the
//                      threshold and the ordering are the code of tc2li_update_connections_batch.  For an erase (KeyFrame::SetBadFlag,
//                      :600-603, :617-618) the touched keyframes are the row's neighbours and changed = the neighbour held the row.
//   k_mgc_neighbours   one wavefront per (sequence, touched keyframe): conn_neighbour, or for an erase the neighbour's row without the
//                      erased keyframe and without bad ones, ranked.
//   k_mgc_rebuild      one workgroup per sequence writes the other generation of both CSRs: new row lengths, a scan for the offsets,
//                      then one wavefront per row copies it, merges (current, weight) into it at its place in row order, drops the
//                      erased keyframe from it or takes the new list from the scratch.  A sequence whose new CSR would pass the reserve
//                      writes its offsets and its status word only.
// All loops are bounded by the keyframe rows and the entries of the reserve, which the host knows.

__device__ __forceinline__ ConnProblemDev mgc_problem(const MgConnBatch& M, const MgConnDev& R, int b) {
    const int s = R.sequence, cw = 2 * s + R.conn_generation, ob = 2 * s + R.obs_generation;
    ConnProblemDev P;
    P.kf_off = s * M.T.cap_kf; P.n_kf = R.n_kf;
    P.conn_row_off = cw * (M.T.cap_kf + 1); P.conn_off = cw * M.C.cap_e;
    P.slot_off = s * M.T.cap_slot + R.slot_begin; P.n_slots = R.n_slots;
    P.point_off = s * M.T.cap_pt; P.obs_row_off = ob * (M.T.cap_pt + 1); P.obs_off = ob * M.T.cap_obs;
    P.current = R.current;
    P.flags = (R.first_connection ? 1 : 0) | (M.T.kf_id[(size_t)P.kf_off + R.current] == R.init_kf_id ? 2 : 0);
    P.hist_off = R.n_kf > kConnLdsKeyframes ? b * M.T.cap_kf : -1;
    P.counter_off = b * M.T.cap_kf; P.counter_cap = M.T.cap_kf;
    P.ordered_off = b * M.T.cap_kf; P.ordered_cap = M.T.cap_kf;
    P.changed_off = b * (M.C.cap_e + M.T.cap_kf); P.changed_cap = M.C.cap_e + M.T.cap_kf;   // every touched row and one entry more each
    return P;
}

// KeyFrame::SetBadFlag's EraseConnection in every neighbour (:600-603): which neighbours hold the row, and how long their new lists are
__device__ __forceinline__ void mgc_erase_prepare(const ConnBatch& B, const ConnProblemDev& P, int* scan) {
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int32_t* conn_row = B.conn_offsets + P.conn_row_off;
    const int32_t* conn_kf = B.conn_kf + P.conn_off;
    const int cur = P.current;
    int32_t* touched_kf = B.touched_kf + P.ordered_off;
    uint8_t* touched_changed = B.touched_changed + P.ordered_off;
    int32_t* item_off = B.item_off + P.ordered_off;
    const int r0 = conn_row[cur], n_row = min(conn_row[cur + 1] - r0, P.ordered_cap);   // a row names no keyframe twice and not its own
    for (int i = wave; i < n_row; i += kConnThreads / 64) {
        const int k = conn_kf[r0 + i];
        const int k1 = conn_row[k + 1];
        int alive = 0, found = 0;
        for (int j = conn_row[k] + lane; j < k1; j += 64) {
            const int kk = conn_kf[j];
            if (kk == cur) found = 1;
            else alive += (flags[kk] & 1) ? 0 : 1;                                  // :229, with the flags as they are at the call
        }
        alive = wave_sum_i32(alive);
        found = wave_sum_i32(found);
        if (lane == 0) { touched_kf[i] = k; touched_changed[i] = found ? 1 : 0; item_off[i] = found ? alive : 0; }
    }
    __syncthreads();
    int n_changed, n_entries;
    changed_csr(touched_changed, item_off, B.changed_offsets + P.ordered_off + blockIdx.x, n_row, scan, &n_changed, &n_entries);
    if (tid < TC2LI_CONNECTIONS_COUNTS) {
        int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_CONNECTIONS_COUNTS;
        counts[tid] = tid == TC2LI_CONNECTIONS_STATUS ? TC2LI_CONNECTIONS_UPDATED : tid == TC2LI_CONNECTIONS_N_ORDERED ? n_row
                    : tid == TC2LI_CONNECTIONS_N_CHANGED ? n_changed : tid == TC2LI_CONNECTIONS_N_CHANGED_ENTRIES ? n_entries
                    : tid == TC2LI_CONNECTIONS_PARENT ? -1 : 0;
    }
}

__global__ __launch_bounds__(kConnThreads) void k_mgc_vote(MgConnBatch M) {
    __shared__ int hist[kConnLdsKeyframes];
    __shared__ int scan[kConnThreads / 64];
    __shared__ unsigned long long best;
    const MgConnDev R = M.records[blockIdx.x];
    const ConnProblemDev P = mgc_problem(M, R, blockIdx.x);
    if (threadIdx.x == 0) M.problems[blockIdx.x] = P;
    if (R.conn_rows < R.n_kf) {   // the rows ADD_KEYFRAME appended since the offsets were written: empty, in both CSRs
        int32_t* wo = M.C.conn_offsets + P.conn_row_off;
        int32_t* oo = M.C.ord_offsets + P.conn_row_off;
        const int tw = R.conn_rows ? wo[R.conn_rows] : 0, to = R.conn_rows ? oo[R.conn_rows] : 0;
        for (int k = R.conn_rows + threadIdx.x; k <= R.n_kf; k += kConnThreads) { wo[k] = tw; oo[k] = to; }   // [conn_rows] gets what it holds
        __syncthreads();
    }
    if (R.mode == kMgcErase) mgc_erase_prepare(M.B, P, scan);
    else if (P.hist_off < 0) conn_problem<1>(M.B, P, hist, scan, &best);
    else conn_problem<1>(M.B, P, M.B.hist + P.hist_off, scan, &best);
}

__global__ __launch_bounds__(kConnRankLanes) void k_mgc_neighbours(MgConnBatch M) {
    const int p = blockIdx.y, i = blockIdx.x;
    const ConnBatch& B = M.B;
    const ConnProblemDev& P = M.problems[p];
    if (i >= P.n_kf) return;
    const int e = P.ordered_off + i;
    if (M.records[p].mode != kMgcErase) { conn_neighbour(B, p, e); return; }
    const int32_t* counts = B.counts + (size_t)p * TC2LI_CONNECTIONS_COUNTS;
    if (i >= counts[TC2LI_CONNECTIONS_N_ORDERED]) return;
    const int off = B.item_off[e];
    if (off < 0) return;
    const int k = B.touched_kf[e], cur = P.current;
    const int32_t* conn_row = B.conn_offsets + P.conn_row_off;
    const int r0 = conn_row[k], r1 = conn_row[k + 1];
    const int32_t* row_kf = B.conn_kf + P.conn_off + r0;
    const int32_t* row_weight = B.conn_weight + P.conn_off + r0;
    const uint8_t* flags = B.kf_flags + P.kf_off;
    // KeyFrame::EraseConnection (:699-713): the entry goes, then UpdateBestCovisibles (:216-238) on what is left
    rank_emit(r1 - r0, [=](int j) -> uint64_t {
        const int kf = row_kf[j];
        return kf == cur || (flags[kf] & 1) ? 0 : conn::key(row_weight[j], kf);
    }, B.changed_kf + P.changed_off + off, B.changed_weight + P.changed_off + off, 0, 1);
}

__global__ __launch_bounds__(kConnThreads) void k_mgc_rebuild(MgConnBatch M) {
    __shared__ int scan[kConnThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    const MgConnDev R = M.records[b];
    const ConnProblemDev P = M.problems[b];
    const ConnBatch& B = M.B;
    const int32_t* counts = B.counts + (size_t)b * TC2LI_CONNECTIONS_COUNTS;
    int32_t* status = M.status + (size_t)b * kMgcStatusWords;
    const int K = R.n_kf, cur = R.current, E = M.C.cap_e, rows = M.T.cap_kf + 1;
    const bool update = R.mode != kMgcErase;
    const size_t g_old = (size_t)(2 * R.sequence + R.conn_generation), g_new = g_old ^ 1;
    const int32_t *wo = M.C.conn_offsets + g_old * rows, *oo = M.C.ord_offsets + g_old * rows;
    int32_t *wn = M.C.conn_offsets + g_new * rows, *on = M.C.ord_offsets + g_new * rows;
    if (counts[TC2LI_CONNECTIONS_STATUS] == TC2LI_CONNECTIONS_UNCHANGED) {           // :426-427: nothing is written
        if (tid == 0) { status[0] = 1; status[1] = wo[K]; status[2] = oo[K]; status[3] = 0; }
        return;
    }
    const int n_touched = counts[TC2LI_CONNECTIONS_N_ORDERED], n_counter = counts[TC2LI_CONNECTIONS_N_COUNTER];
    const int32_t* touched_kf = B.touched_kf + P.ordered_off;
    const int32_t* touched_weight = B.touched_weight + P.ordered_off;
    const uint8_t* touched_changed = B.touched_changed + P.ordered_off;
    const uint8_t* item_found = B.item_found + P.ordered_off;
    const int32_t* item_off = B.item_off + P.ordered_off;
    const int32_t* changed_offsets = B.changed_offsets + P.ordered_off + b;
    int32_t* row_of = M.row_of + (size_t)b * 2 * M.T.cap_kf;
    int32_t* list_len = row_of + M.T.cap_kf;
    for (int k = tid; k < K; k += kConnThreads) row_of[k] = -1;
    __syncthreads();
    int n_changed = 0;
    for (int base = 0; base < n_touched; base += kConnThreads) {
        const int i = base + tid;
        const int changed = i < n_touched ? touched_changed[i] : 0;
        int tot;
        const int c = n_changed + block_scan_excl<kConnThreads>(changed, scan, &tot);
        if (changed) { row_of[touched_kf[i]] = i; list_len[i] = changed_offsets[c + 1] - changed_offsets[c]; }
        n_changed += tot;
    }
    __syncthreads();
    // the new offsets of both CSRs
    int n_w = 0, n_o = 0;
    for (int base = 0; base < K; base += kConnThreads) {
        const int k = base + tid;
        int lw = 0, lo = 0;
        if (k < K) {
            lw = wo[k + 1] - wo[k]; lo = oo[k + 1] - oo[k];
            const int i = row_of[k];
            if (k == cur) { lw = update ? n_counter : 0; lo = update ? n_touched : 0; }                     // :473-475; mConnectedKeyFrameWeights.clear() (:617-618)
            else if (i >= 0) { lw += update ? (item_found[i] ? 0 : 1) : -1; lo = list_len[i]; }             // :205-213; :703-711
        }
        int tot_w, tot_o;
        const int aw = n_w + block_scan_excl<kConnThreads>(lw, scan, &tot_w);
        const int ao = n_o + block_scan_excl<kConnThreads>(lo, scan, &tot_o);
        if (k < K) { wn[k] = aw; on[k] = ao; }
        n_w += tot_w;
        n_o += tot_o;
    }
    const bool fits = n_w <= E && n_o <= E;
    if (tid == 0) { wn[K] = n_w; on[K] = n_o; status[0] = fits; status[1] = n_w; status[2] = n_o; status[3] = 0; }
    if (!fits) return;                                                               // the whole workgroup: the host keeps the generation
    __syncthreads();
    const int32_t *okf = M.C.conn_kf + g_old * E, *owt = M.C.conn_weight + g_old * E, *ook = M.C.ord_kf + g_old * E, *oow = M.C.ord_weight + g_old * E;
    int32_t *nkf = M.C.conn_kf + g_new * E, *nwt = M.C.conn_weight + g_new * E, *nok = M.C.ord_kf + g_new * E, *now = M.C.ord_weight + g_new * E;
    for (int k = wave; k < K; k += kConnThreads / 64) {
        const int i = k == cur ? -1 : row_of[k];
        {   // the weight row
            const int o0 = wo[k], n_old = wo[k + 1] - o0;
            int32_t *dk = nkf + wn[k], *dw = nwt + wn[k];
            if (k == cur) {
                if (update)
                    for (int j = lane; j < n_counter; j += 64) { dk[j] = B.counter_kf[P.counter_off + j]; dw[j] = B.counter_weight[P.counter_off + j]; }
            } else if (i < 0) {
                for (int j = lane; j < n_old; j += 64) { dk[j] = okf[o0 + j]; dw[j] = owt[o0 + j]; }
            } else if (update) {                                                     // mConnectedKeyFrameWeights[pKF] = weight at its place in map order
                const int w = touched_weight[i];
                const bool insert = !item_found[i];
                if (insert && lane == 0 && (n_old == 0 || okf[o0] > cur)) { dk[0] = cur; dw[0] = w; }
                for (int j = lane; j < n_old; j += 64) {
                    const int kk = okf[o0 + j];
                    const int d = j + (insert && kk > cur ? 1 : 0);
                    dk[d] = kk; dw[d] = kk == cur ? w : owt[o0 + j];
                    if (insert && kk < cur && (j + 1 == n_old || okf[o0 + j + 1] > cur)) { dk[j + 1] = cur; dw[j + 1] = w; }
                }
            } else {                                                                 // mConnectedKeyFrameWeights.erase(pKF) (:703-707)
                for (int j = lane; j < n_old; j += 64) {
                    const int kk = okf[o0 + j];
                    if (kk != cur) { const int d = j - (kk > cur ? 1 : 0); dk[d] = kk; dw[d] = owt[o0 + j]; }
                }
            }
        }
        {   // the ordered row
            int32_t *dk = nok + on[k], *dw = now + on[k];
            if (k == cur) {
                if (update)
                    for (int j = lane; j < n_touched; j += 64) { dk[j] = B.ordered_kf[P.ordered_off + j]; dw[j] = B.ordered_weight[P.ordered_off + j]; }
            } else if (i < 0) {                                                      // :209-210 too: a stale list stays stale
                const int o0 = oo[k], n_old = oo[k + 1] - o0;
                for (int j = lane; j < n_old; j += 64) { dk[j] = ook[o0 + j]; dw[j] = oow[o0 + j]; }
            } else {
                const int32_t *sk = B.changed_kf + P.changed_off + item_off[i], *sw = B.changed_weight + P.changed_off + item_off[i];
                for (int j = lane; j < list_len[i]; j += 64) { dk[j] = sk[j]; dw[j] = sw[j]; }
            }
        }
    }
}

void launch_map_graph_connections(const MgConnBatch& M, hipStream_t st) {
    if (M.n <= 0) return;
    TC2LI_LAUNCH(k_mgc_vote, dim3(M.n), dim3(kConnThreads), 0, st, M);
    if (M.max_kf > 0) TC2LI_LAUNCH(k_mgc_neighbours, dim3(M.max_kf, M.n), dim3(kConnRankLanes), 0, st, M);
    TC2LI_LAUNCH(k_mgc_rebuild, dim3(M.n), dim3(kConnThreads), 0, st, M);
}

}  // namespace tc2li

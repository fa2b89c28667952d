// Projection-guided matching of the tracking thread on gfx950 -- the loop bodies shared by
// ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono) (SF/src/ORBmatcher.cc:1685-1896) and
// ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th, ...) (:52-222), with Frame::GetFeaturesInArea
// (SF/src/Frame.cc:687-753) on the 64x48 feature grid (AssignFeaturesToGrid / PosInGrid, :412-443,755-765).
//
// The reference loop is sequential: a keypoint matched by an earlier map point is skipped by later ones.  One
// workgroup per frame reproduces exactly that result by fixed-point iteration: in every round all queries are
// evaluated in parallel against "keypoints claimed in the previous round by a query with a smaller index"; query q's
// answer depends only on the answers of queries < q, so after round k the first k queries are final and the
// iteration stops at the first round that changes nothing (unique fixed point = the sequential result).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "matcher_device.hpp"

namespace tc2li {

constexpr int kGridCols = 64, kGridRows = 48, kCells = kGridCols * kGridRows;
constexpr int kThreads = 512;

__global__ __launch_bounds__(kThreads) void k_match_by_projection(const MatchFrameDev* __restrict__ frames, int mode, float nn_ratio, int max_dist,
                                                                 int32_t* __restrict__ match_of_query, int32_t* __restrict__ prev_claim,
                                                                 int32_t* __restrict__ rounds_out) {
    __shared__ int s_cell_start[kCells + 1];
    __shared__ uint16_t s_items[kMaxMatchKeys];
    __shared__ float s_x[kMaxMatchKeys], s_y[kMaxMatchKeys], s_ur[kMaxMatchKeys];
    __shared__ uint8_t s_oct[kMaxMatchKeys], s_occ[kMaxMatchKeys];
    __shared__ int s_claim[2][kMaxMatchKeys];
    __shared__ int s_tmp[64];
    const MatchFrameDev fr = global_record(frames[blockIdx.x]);
    const int tid = threadIdx.x, N = fr.n_keys, M = fr.n_queries;
    const float invW = (float)kGridCols / (fr.max_x - fr.min_x), invH = (float)kGridRows / (fr.max_y - fr.min_y);
    int32_t* out = match_of_query + fr.query_off;
    int32_t* prev = prev_claim + fr.query_off;

    // ---- feature grid ----
    for (int c = tid; c <= kCells; c += kThreads) s_cell_start[c] = 0;
    __syncthreads();
    int* cell_of = s_claim[1];  // scratch until the matching rounds start
    for (int i = tid; i < N; i += kThreads) {
        const MatchKey k = fr.keys[i];
        s_x[i] = k.x; s_y[i] = k.y; s_oct[i] = (uint8_t)k.octave;
        s_ur[i] = fr.u_right[i];
        s_occ[i] = fr.occupied ? fr.occupied[i] : 0;
        const int px = (int)roundf((k.x - fr.min_x) * invW), py = (int)roundf((k.y - fr.min_y) * invH);
        const bool in = !(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows);
        const int c = in ? px * kGridRows + py : -1;
        cell_of[i] = c;
        if (in) atomicAdd(&s_cell_start[c + 1], 1);
    }
    __syncthreads();
    // exclusive scan over the cell counts (one wavefront, 48 cells per lane)
    if (tid < 64) {
        constexpr int per = kCells / 64;
        int sum = 0;
        for (int k = 0; k < per; ++k) sum += s_cell_start[1 + tid * per + k];
        int incl = sum;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
        int run = incl - sum;
        for (int k = 0; k < per; ++k) { const int c = s_cell_start[1 + tid * per + k]; s_cell_start[1 + tid * per + k] = run + c; run += c; }
    }
    __syncthreads();
    // fill (cursor = claim[0] scratch), then restore ascending keypoint order inside each cell
    int* cursor = s_claim[0];
    for (int c = tid; c < kCells; c += kThreads) cursor[c] = s_cell_start[c];
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) {
        const int c = cell_of[i];
        if (c >= 0) s_items[atomicAdd(&cursor[c], 1)] = (uint16_t)i;
    }
    __syncthreads();
    for (int c = tid; c < kCells; c += kThreads) {
        const int b = s_cell_start[c], e = s_cell_start[c + 1];
        for (int a = b + 1; a < e; ++a) {
            const uint16_t key = s_items[a];
            int k = a - 1;
            while (k >= b && s_items[k] > key) { s_items[k + 1] = s_items[k]; --k; }
            s_items[k + 1] = key;
        }
    }
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) { s_claim[0][i] = 0x7fffffff; s_claim[1][i] = 0x7fffffff; }
    for (int q = tid; q < M; q += kThreads) prev[q] = -2;
    __syncthreads();

    const uint32_t* D = reinterpret_cast<const uint32_t*>(fr.desc);
    int cur = 0, round = 0;
    for (;;) {
        int* claim_prev = s_claim[cur];
        int* claim_new = s_claim[cur ^ 1];
        int changed = 0;
        for (int q = tid; q < M; q += kThreads) {
            const MatchQuery Q = fr.queries[q];
            int claim = -1;
            if (Q.valid) {
                // Frame::GetFeaturesInArea(u, v, r, minLevel, maxLevel)
                const float r = Q.radius;
                const int minCX = max(0, (int)floorf((Q.u - fr.min_x - r) * invW));
                const int maxCX = min(kGridCols - 1, (int)ceilf((Q.u - fr.min_x + r) * invW));
                const int minCY = max(0, (int)floorf((Q.v - fr.min_y - r) * invH));
                const int maxCY = min(kGridRows - 1, (int)ceilf((Q.v - fr.min_y + r) * invH));
                const bool any = !(minCX >= kGridCols || maxCX < 0 || minCY >= kGridRows || maxCY < 0);
                const bool check_levels = (Q.min_level > 0) || (Q.max_level >= 0);
                const uint32_t* qd = reinterpret_cast<const uint32_t*>(Q.desc);
                int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
                if (any)
                    for (int ix = minCX; ix <= maxCX; ++ix)
                        for (int iy = minCY; iy <= maxCY; ++iy) {
                            const int c = ix * kGridRows + iy;
                            for (int k = s_cell_start[c]; k < s_cell_start[c + 1]; ++k) {
                                const int idx = s_items[k];
                                const int oct = s_oct[idx];
                                if (check_levels) {
                                    if (oct < Q.min_level) continue;
                                    if (Q.max_level >= 0 && oct > Q.max_level) continue;
                                }
                                if (!(fabsf(s_x[idx] - Q.u) < r && fabsf(s_y[idx] - Q.v) < r)) continue;
                                if (s_occ[idx] || claim_prev[idx] < q) continue;  // already matched by an earlier point
                                if (s_ur[idx] > 0) {
                                    if (fabsf(Q.u_right - s_ur[idx]) > r) continue;
                                }
                                const uint32_t* kd = D + (size_t)idx * 8;
                                int dist = 0;
#pragma unroll
                                for (int w = 0; w < 8; ++w) dist += __popc(qd[w] ^ kd[w]);
                                if (mode == 0) {
                                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                                } else if (dist < bestDist) {
                                    bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = oct; bestIdx = idx;
                                } else if (dist < bestDist2) {
                                    bestLevel2 = oct; bestDist2 = dist;
                                }
                            }
                        }
                if (bestDist <= max_dist) {  // TH_HIGH (100), or the ORBdist of the keyframe overload
                    bool ok = true;
                    if (mode != 0) {
                        if (bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) ok = false;
                    }
                    if (ok) claim = bestIdx;
                }
            }
            if (claim >= 0 && Q.has_observations) atomicMin(&claim_new[claim], q);
            if (prev[q] != claim) { changed = 1; prev[q] = claim; }
            out[q] = claim;
        }
        const int any_changed = __syncthreads_or(changed);
        ++round;
        if (!any_changed || round > M + 1) break;
        for (int i = tid; i < N; i += kThreads) claim_prev[i] = 0x7fffffff;  // becomes the next round's "new"
        cur ^= 1;
        __syncthreads();
    }
    if (tid == 0) rounds_out[blockIdx.x] = round;
    (void)s_tmp;
}

// ---- the same result in three launches -----------------------------------------------------------------------------------
// k_match_by_projection recomputes every Hamming distance in every round with one workgroup per frame.  Everything except
// "claimed by an earlier query" is independent of the rounds, so:
//   k_match_grid        one workgroup per frame: the 64x48 feature grid (cell starts, keypoint indices ascending per cell) in HBM
//                       (the frames of an extractor handle: once per extraction, frame_grids of projection_search.hpp)
//   k_match_candidates  a sub-group of lanes per query over the whole batch: the candidates that pass the static tests of the loop
//                       body, in scan order, with their descriptor distance (idx | dist << 12 | octave << 21), into a pool
//   k_match_resolve     one workgroup per frame: the fixed-point rounds walk the short candidate lists only

__global__ __launch_bounds__(kThreads) void k_match_grid(const MatchFrameDev* __restrict__ frames, MatchLists L) {
    __shared__ int s_cell_start[kCells + 1];
    __shared__ int s_cursor[kCells];
    __shared__ int s_cell_of[kMaxMatchKeys];
    __shared__ uint16_t s_items[kMaxMatchKeys];
    const MatchFrameDev fr = global_record(frames[blockIdx.x]);
    const int tid = threadIdx.x, N = fr.n_keys;
    const float invW = (float)kGridCols / (fr.max_x - fr.min_x), invH = (float)kGridRows / (fr.max_y - fr.min_y);
    for (int c = tid; c <= kCells; c += kThreads) s_cell_start[c] = 0;
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) {
        const MatchKey k = fr.keys[i];
        const int px = (int)roundf((k.x - fr.min_x) * invW), py = (int)roundf((k.y - fr.min_y) * invH);
        const bool in = !(px < 0 || px >= kGridCols || py < 0 || py >= kGridRows);
        const int c = in ? px * kGridRows + py : -1;
        s_cell_of[i] = c;
        if (in) atomicAdd(&s_cell_start[c + 1], 1);
    }
    __syncthreads();
    if (tid < 64) {
        constexpr int per = kCells / 64;
        int sum = 0;
        for (int k = 0; k < per; ++k) sum += s_cell_start[1 + tid * per + k];
        int incl = sum;
        for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (tid >= o) incl += t; }
        int run = incl - sum;
        for (int k = 0; k < per; ++k) { const int c = s_cell_start[1 + tid * per + k]; s_cell_start[1 + tid * per + k] = run + c; run += c; }
    }
    __syncthreads();
    for (int c = tid; c < kCells; c += kThreads) s_cursor[c] = s_cell_start[c];
    __syncthreads();
    for (int i = tid; i < N; i += kThreads) {
        const int c = s_cell_of[i];
        if (c >= 0) s_items[atomicAdd(&s_cursor[c], 1)] = (uint16_t)i;
    }
    __syncthreads();
    for (int c = tid; c < kCells; c += kThreads) {  // ascending keypoint order inside each cell (the order the reference's grid has)
        const int b = s_cell_start[c], e = s_cell_start[c + 1];
        for (int a = b + 1; a < e; ++a) {
            const uint16_t key = s_items[a];
            int k = a - 1;
            while (k >= b && s_items[k] > key) { s_items[k + 1] = s_items[k]; --k; }
            s_items[k + 1] = key;
        }
    }
    __syncthreads();
    int32_t* cs = L.cell_start + (size_t)(L.cell_row ? L.cell_row[blockIdx.x] : (int)blockIdx.x) * (kCells + 1);
    uint16_t* it = L.items + L.key_base[blockIdx.x];
    for (int c = tid; c <= kCells; c += kThreads) cs[c] = s_cell_start[c];
    const int n_in = s_cell_start[kCells];
    for (int i = tid; i < n_in; i += kThreads) it[i] = s_items[i];
}

// what a lane needs of its query for the static tests
struct QueryWindow {
    float u, v, r, u_right;
    int min_level, max_level;
    bool check_levels;
};

// the static part of the loop body for one candidate: level window, search window, occupancy, stereo coordinate
__device__ __forceinline__ bool candidate_ok(const MatchFrameDev& fr, const QueryWindow& Q, int idx, int& oct) {
    const MatchKey k = fr.keys[idx];
    oct = k.octave;
    if (Q.check_levels) {
        if (oct < Q.min_level) return false;
        if (Q.max_level >= 0 && oct > Q.max_level) return false;
    }
    const float r = Q.r;
    if (!(fabsf(k.x - Q.u) < r && fabsf(k.y - Q.v) < r)) return false;
    if (fr.occupied && fr.occupied[idx]) return false;
    const float ur = fr.u_right[idx];
    if (ur > 0) {
        if (fabsf(Q.u_right - ur) > r) return false;
    }
    return true;
}

constexpr int kCandThreads = 256;
// candidates a sub-group keeps in LDS until the pool space is reserved (the pool's default: 32 per query); narrow sub-groups are many per
// workgroup and keep half as many
constexpr int cand_stage(int lanes) { return lanes >= 8 ? 32 : 16; }

// LDS written by some lanes of a wavefront and read by others of the same wavefront
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the ballot of the W lanes of the caller's sub-group (every lane of a sub-group runs the same loops, so they are active together)
template <int W>
__device__ __forceinline__ uint32_t sub_ballot(bool p) {
    const unsigned long long m = __ballot(p);
    return (uint32_t)(m >> ((threadIdx.x & 63) / W * W)) & (W == 32 ? 0xffffffffu : (1u << (W & 31)) - 1u);
}

// One walk over a query's window in the reference's order: ix outer, iy inner, key index ascending.  The cells iy = minCY .. maxCY of a
// column are neighbours in cell_start, so a column is ONE run of items.  The W lanes of the sub-group take a run W keys at a time -- the
// gathers of a round (item, key, occupied, u_right, descriptor) are independent of each other -- and a ballot gives every passing key its
// place in the list.  kStage > 0: the count is not known yet, the first kStage entries go to the sub-group's LDS stage `out`; 0: `out` is
// the query's pool space.  Returns the number of candidates.
template <int W, int kStage>
__device__ __forceinline__ int walk_window(const MatchFrameDev& fr, const QueryWindow& Q, const uint4 qd0, const uint4 qd1, const int32_t* cs,
                                           const uint16_t* items, int minCX, int maxCX, int minCY, int maxCY, int sl, uint32_t* out) {
    const uint4* D = reinterpret_cast<const uint4*>(fr.desc);
    const int span = maxCY - minCY + 1;
    int c0 = minCX * kGridRows + minCY;
    int b = cs[c0], e = cs[c0 + span];
    int cnt = 0;
    for (int ix = minCX; ix <= maxCX; ++ix) {
        c0 += kGridRows;
        int nb = 0, ne = 0;
        if (ix < maxCX) { nb = cs[c0]; ne = cs[c0 + span]; }  // the next column's run: in flight under this column's keys
        for (int k0 = b; k0 < e; k0 += W) {
            const int k = k0 + sl;
            bool ok = false;
            uint32_t entry = 0;
            if (k < e) {
                const int idx = items[k];
                int oct;
                ok = candidate_ok(fr, Q, idx, oct);
                if (ok) {
                    const uint4 d0 = D[2 * (size_t)idx], d1 = D[2 * (size_t)idx + 1];
                    const int dist = __popc(qd0.x ^ d0.x) + __popc(qd0.y ^ d0.y) + __popc(qd0.z ^ d0.z) + __popc(qd0.w ^ d0.w) +
                                     __popc(qd1.x ^ d1.x) + __popc(qd1.y ^ d1.y) + __popc(qd1.z ^ d1.z) + __popc(qd1.w ^ d1.w);
                    entry = (uint32_t)idx | ((uint32_t)dist << 12) | ((uint32_t)oct << 21);
                }
            }
            const uint32_t m = sub_ballot<W>(ok);
            if (ok) {
                const int at = cnt + __popc(m & ((1u << sl) - 1u));
                if (kStage == 0 || at < kStage) out[at] = entry;
            }
            cnt += __popc(m);
        }
        b = nb; e = ne;
    }
    return cnt;
}

// W lanes per query, kCandThreads / W queries per block of queries.  The queries of a pass come frame by frame, and the hardware deals
// consecutive workgroups to the eight XCDs in turn, each with its own L2: XCD k takes the k-th contiguous eighth of the query blocks (as
// k_fast_cells does with its cells), so a frame's keys, descriptors, u_right, occupied and grid are fetched into ONE L2, not into eight.
// A workgroup takes `run` consecutive blocks of its XCD's share.  Every candidate is tested once: the walk keeps the entries in LDS, one
// atomic per wavefront reserves the pool space of its queries, and the stage is copied out; only a list longer than the stage is walked a
// second time.
template <int W>
__global__ __launch_bounds__(kCandThreads) void k_match_candidates(const MatchFrameDev* __restrict__ frames, int nframes,
                                                                   const int32_t* __restrict__ query_frame, int total_q, MatchLists L, int run) {
    static_assert(W >= 2 && W <= 32 && (W & (W - 1)) == 0, "a sub-group lies inside half a wavefront");
    constexpr int kSub = kCandThreads / W, kCandStage = cand_stage(W);
    __shared__ uint4 s_query[kSub][4];
    __shared__ uint32_t s_stage[kSub][kCandStage];
    const int tid = threadIdx.x, sub = tid / W, sl = tid % W, lane = tid & 63, lead = lane / W * W;
    const int nblk = (total_q + kSub - 1) / kSub, per_xcd = (nblk + 7) / 8;
    for (int rep = 0; rep < run; ++rep) {
        const int in_xcd = ((int)blockIdx.x >> 3) * run + rep;
        const int logical = ((int)blockIdx.x & 7) * per_xcd + in_xcd;
        if (in_xcd >= per_xcd || logical >= nblk) break;  // whole workgroup
        const int g = logical * kSub + sub;
        const int f = g < total_q ? query_frame[g] : -1;
        MatchFrameDev fr{};
        QueryWindow Q{};
        uint4 qd0 = make_uint4(0, 0, 0, 0), qd1 = qd0;
        const int32_t* cs = nullptr;
        const uint16_t* items = nullptr;
        int minCX = 0, maxCX = -1, minCY = 0, maxCY = -1, cnt = 0, flags = 0;
        if (f >= 0) {
            fr = global_record(frames[f]);
            // the query's record once per sub-group, in 16-byte pieces through LDS
            for (int i = sl; i < 4; i += W) s_query[sub][i] = reinterpret_cast<const uint4*>(fr.queries + (g - fr.query_off))[i];
            wave_lds_sync();
            const uint4 q0 = s_query[sub][0], q1 = s_query[sub][1];
            qd0 = s_query[sub][2]; qd1 = s_query[sub][3];
            Q.u = __uint_as_float(q0.x); Q.v = __uint_as_float(q0.y); Q.r = __uint_as_float(q0.z); Q.u_right = __uint_as_float(q0.w);
            Q.min_level = (int)q1.x; Q.max_level = (int)q1.y;
            Q.check_levels = (Q.min_level > 0) || (Q.max_level >= 0);
            const bool valid = (q1.w & 0xffffu) != 0, has_observations = (q1.w >> 16) != 0;  // MatchQuery: int16_t valid, has_observations
            flags = has_observations ? (1 << 30) : 0;
            if (valid && fr.n_keys > 0) {
                const float invW = (float)kGridCols / (fr.max_x - fr.min_x), invH = (float)kGridRows / (fr.max_y - fr.min_y);
                const float r = Q.r;
                minCX = max(0, (int)floorf((Q.u - fr.min_x - r) * invW));
                maxCX = min(kGridCols - 1, (int)ceilf((Q.u - fr.min_x + r) * invW));
                minCY = max(0, (int)floorf((Q.v - fr.min_y - r) * invH));
                maxCY = min(kGridRows - 1, (int)ceilf((Q.v - fr.min_y + r) * invH));
                const bool any = !(minCX >= kGridCols || maxCX < 0 || minCY >= kGridRows || maxCY < 0);
                if (any) {
                    cs = L.cell_start + (size_t)(L.cell_row ? L.cell_row[f] : f) * (kCells + 1);
                    items = L.items + L.key_base[f];
                    cnt = walk_window<W, kCandStage>(fr, Q, qd0, qd1, cs, items, minCX, maxCX, minCY, maxCY, sl, s_stage[sub]);
                }
            }
        }
        wave_lds_sync();
        // ---- pool space: one atomic per wavefront (every lane of the wavefront is here) ----
        const int mine = sl == 0 ? cnt : 0;
        int incl = mine;
        for (int o = W; o < 64; o <<= 1) { const int t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        const int total = __shfl(incl, 64 - W, 64);
        int base = 0;
        if (lane == 0 && total > 0) base = atomicAdd(L.pool_top, total);
        base = __shfl(base, 0, 64);
        int off = __shfl(base + incl - mine, lead, 64);
        // a list the pool cannot hold is dropped whole and reported: projection_search then runs the one-kernel form
        if (cnt > 0 && off + cnt > L.pool_cap) { if (sl == 0) L.pool_top[1] = 1; cnt = 0; }
        if (cnt == 0) off = 0;
        if (sl == 0 && g < total_q) { L.cand_off[g] = off; L.cand_cnt[g] = cnt | flags; }
        if (cnt > 0) {
            uint32_t* out = L.pool + off;
            if (cnt <= kCandStage) for (int i = sl; i < cnt; i += W) out[i] = s_stage[sub][i];
            else walk_window<W, 0>(fr, Q, qd0, qd1, cs, items, minCX, maxCX, minCY, maxCY, sl, out);
        }
        wave_lds_sync();  // the next block of queries rewrites the sub-group's LDS
    }
}

__global__ __launch_bounds__(kThreads) void k_match_resolve(const MatchFrameDev* __restrict__ frames, int mode, float nn_ratio, int max_dist, MatchLists L,
                                                           int32_t* __restrict__ match_of_query, int32_t* __restrict__ prev_claim,
                                                           int32_t* __restrict__ rounds_out) {
    __shared__ int s_claim[2][kMaxMatchKeys];
    const MatchFrameDev fr = global_record(frames[blockIdx.x]);
    const int tid = threadIdx.x, N = fr.n_keys, M = fr.n_queries;
    int32_t* out = match_of_query + fr.query_off;
    int32_t* prev = prev_claim + fr.query_off;
    const int32_t* coff = L.cand_off + fr.query_off;
    const int32_t* ccnt = L.cand_cnt + fr.query_off;
    for (int i = tid; i < N; i += kThreads) { s_claim[0][i] = 0x7fffffff; s_claim[1][i] = 0x7fffffff; }
    for (int q = tid; q < M; q += kThreads) prev[q] = -2;
    __syncthreads();
    int cur = 0, round = 0;
    for (;;) {
        int* claim_prev = s_claim[cur];
        int* claim_new = s_claim[cur ^ 1];
        int changed = 0;
        for (int q = tid; q < M; q += kThreads) {
            const int cc = ccnt[q], cnt = cc & 0x3fffffff;
            const uint32_t* e = L.pool + coff[q];
            int bestDist = 256, bestLevel = -1, bestDist2 = 256, bestLevel2 = -1, bestIdx = -1;
            for (int k = 0; k < cnt; ++k) {
                const uint32_t v = e[k];
                const int idx = v & 0xfff, dist = (v >> 12) & 0x1ff, oct = (v >> 21) & 0xf;
                if (claim_prev[idx] < q) continue;  // already matched by an earlier point
                if (mode == 0) {
                    if (dist < bestDist) { bestDist = dist; bestIdx = idx; }
                } else if (dist < bestDist) {
                    bestDist2 = bestDist; bestDist = dist; bestLevel2 = bestLevel; bestLevel = oct; bestIdx = idx;
                } else if (dist < bestDist2) {
                    bestLevel2 = oct; bestDist2 = dist;
                }
            }
            int claim = -1;
            if (bestDist <= max_dist) {  // TH_HIGH (100), or the ORBdist of the keyframe overload
                bool ok = true;
                if (mode != 0) {
                    if (bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) ok = false;
                }
                if (ok) claim = bestIdx;
            }
            if (claim >= 0 && (cc & (1 << 30))) atomicMin(&claim_new[claim], q);
            if (prev[q] != claim) { changed = 1; prev[q] = claim; }
            out[q] = claim;
        }
        const int any_changed = __syncthreads_or(changed);
        ++round;
        if (!any_changed || round > M + 1) break;
        for (int i = tid; i < N; i += kThreads) claim_prev[i] = 0x7fffffff;  // becomes the next round's "new"
        cur ^= 1;
        __syncthreads();
    }
    if (tid == 0) rounds_out[blockIdx.x] = round;
}

void launch_match_grid(const MatchFrameDev* frames, int nframes, const MatchLists& L, hipStream_t st) {
    if (nframes > 0) TC2LI_LAUNCH(k_match_grid, dim3(nframes), dim3(kThreads), 0, st, frames, L);
}

template <int W>
static void launch_match_candidates_w(const MatchFrameDev* frames, int nframes, const int32_t* query_frame, int total_q, const MatchLists& L,
                                      hipStream_t st) {
    constexpr int kSub = kCandThreads / W;
    const int nblk = (total_q + kSub - 1) / kSub, per_xcd = (nblk + 7) / 8;
    // a workgroup covers up to W blocks of 256 / W queries, fewer when that would leave an XCD's 32 CUs short of two workgroups each
    const int run = std::min(W, std::max(1, per_xcd / 64));
    TC2LI_LAUNCH(k_match_candidates<W>, dim3(((per_xcd + run - 1) / run) * 8), dim3(kCandThreads), 0, st, frames, nframes, query_frame, total_q, L, run);
}

static void launch_match_candidates(const MatchFrameDev* frames, int nframes, const int32_t* query_frame, int total_q, const MatchLists& L,
                                    hipStream_t st) {
    if (total_q <= 0) return;
    // Lanes per query, read per call: 2 (default), 4, 8, 16 or 32.  The loop's windows hold a handful of keys, so wide sub-groups are mostly
    // idle lanes and the kernel's time follows its wavefront count (in the loop, per launch of 512 frames: 0.62 ms with 2 lanes, 0.84 with
    // 4, 1.17 with 8, 1.79 with 16, 2.42 with 32; one lane per query that walks twice, the form before: 0.96 - 1.10 ms).
    const char* lanes_env = getenv("TC2LI_MATCH_LANES");
    const int lanes = lanes_env ? atoi(lanes_env) : 2;
    if (lanes == 4) launch_match_candidates_w<4>(frames, nframes, query_frame, total_q, L, st);
    else if (lanes == 8) launch_match_candidates_w<8>(frames, nframes, query_frame, total_q, L, st);
    else if (lanes == 16) launch_match_candidates_w<16>(frames, nframes, query_frame, total_q, L, st);
    else if (lanes == 32) launch_match_candidates_w<32>(frames, nframes, query_frame, total_q, L, st);
    else launch_match_candidates_w<2>(frames, nframes, query_frame, total_q, L, st);
}

void launch_match_lists(const MatchFrameDev* frames, int nframes, const int32_t* query_frame, int total_q, const MatchLists& L, int mode,
                        float nn_ratio, int32_t* match_of_query, int32_t* prev_claim, int32_t* rounds_out, hipStream_t st, int max_dist) {
    if (nframes <= 0) return;
    (void)hipMemsetAsync(L.pool_top, 0, 2 * sizeof(int32_t), st);
    if (!L.grid_ready) TC2LI_LAUNCH(k_match_grid, dim3(nframes), dim3(kThreads), 0, st, frames, L);
    launch_match_candidates(frames, nframes, query_frame, total_q, L, st);
    TC2LI_LAUNCH(k_match_resolve, dim3(nframes), dim3(kThreads), 0, st, frames, mode, nn_ratio, max_dist, L, match_of_query, prev_claim, rounds_out);
}

void launch_match_by_projection(const MatchFrameDev* frames, int nframes, int mode, float nn_ratio, int32_t* match_of_query,
                                int32_t* prev_claim, int32_t* rounds_out, hipStream_t st, int max_dist) {
    if (nframes > 0)
        TC2LI_LAUNCH(k_match_by_projection, dim3(nframes), dim3(kThreads), 0, st, frames, mode, nn_ratio, max_dist, match_of_query, prev_claim,
                           rounds_out);
}

}  // namespace tc2li

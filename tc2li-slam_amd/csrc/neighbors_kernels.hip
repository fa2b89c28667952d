// LocalMapping::SearchInNeighbors (SF/src/LocalMapping.cc:728-837) in the reference's order: one workgroup owns one problem from the
// target selection to the refresh (include/tc2li_hip.h "tc2li_search_in_neighbors_batch" states the rules this file follows).
//
// Per target (and per piece of kNbMaxKeys entries of the stage-2 list):
//   search    all list entries side by side, one lane per entry, on the store's grid (fuse_search_one); an entry's search reads only the
//             state its point had when the target started -- whatever an earlier entry of the same target does to a point makes it skipped
//             (the header's three sentences)
//   compact   the hits, in list order, with wavefront ballots (wavefront 0)
//   apply     thread 0 walks the hits in list order: "bad now" / "in the keyframe now" again, the slot's live occupant, AddObservation or
//             Replace on the flat graph; a winner is flagged
//   describe  every flagged winner that survived: ComputeDistinctiveDescriptors, one wavefront per point
// State: the per-point flags (bad, candidate mark, flagged, to refresh) and the keyframe flags (bad, target mark) are bytes in LDS; the
// slot rows, nObs, found, visible and the point records are the problem's tables in global memory; an observation list lives in the
// problem's pool (global), first where the upload put it, and moves to a fresh piece of the pool when it outgrows its room (a bump
// pointer that only thread 0 moves).  A point that would pass kNbMaxObs observations, a pool that runs out, or a Replace whose winner
// stays outside the keyframe with an entry ahead in the list (possible only where a slot holds a point without the matching
// observation) ends the problem with status ON_HOST: the host twin computes it.  No workgroup waits for another; every loop is bounded by a count fixed at launch.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "fuse_search.hpp"
#include "neighbors_device.hpp"
#include "point_refresh_device.hpp"

namespace tc2li {

namespace {

constexpr int F_BAD = 1, F_MARK = 2, F_DIRTY = 4, F_REFRESH = 8;
using refresh::kDescStride;
using refresh::lane_rank;
using refresh::wave_sync_lds;
enum { S_STATUS = 0, S_NTARGETS, S_NHITS, S_POOL, S_NOPS, S_NCAND, S_FUSED1, S_FUSED2, S_NREFRESHED, S_FUSED, S_COUNT };

struct Ctx {  // the tables of this workgroup's problem
    NbProblemDev P;
    const NbKf* kfs;
    const int32_t* slot_offsets;
    int32_t* slot;
    uint8_t* points;
    int32_t *nobs, *found, *visible, *replaced;
    NbObs* pool;
    int32_t *p_start, *p_len, *p_cap;
    int32_t* ops;
    uint8_t *pflag, *kflag;  // LDS
    int32_t* s;              // LDS scalars
};

// MapPoint::IsInKeyFrame: the row ascends by keyframe
__device__ __forceinline__ bool in_kf(const Ctx& c, int p, int kf) {
    const NbObs* o = c.pool + c.p_start[p];
    return refresh::in_kf(c.p_len[p], [=](int k) { return o[k].kf; }, kf);
}

// room for `need` observations of point w: a list that outgrows its room moves to a fresh piece of the pool, half as long again as
// needed; false: the pool has run out (status set)
__device__ bool reserve_obs(Ctx& c, int w, int need) {
    if (need <= c.p_cap[w]) return true;
    int cap = need + (need >> 1);
    cap = cap < 4 ? 4 : (cap > kNbMaxObs ? kNbMaxObs : cap);
    const int at = c.s[S_POOL], len = c.p_len[w];
    if (at + cap > c.P.pool_size) { c.s[S_STATUS] = 1; return false; }
    c.s[S_POOL] = at + cap;
    const NbObs* from = c.pool + c.p_start[w];
    for (int k = 0; k < len; ++k) c.pool[at + k] = from[k];
    c.p_start[w] = at; c.p_cap[w] = cap;
    return true;
}

// MapPoint::AddObservation (MapPoint.cc:150-175) of a keyframe the point is not in; false: a limit was met (status set)
__device__ bool add_obs(Ctx& c, int w, int kf, int idx) {
    const int len = c.p_len[w];
    if (len + 1 > kNbMaxObs) { c.s[S_STATUS] = 1; return false; }
    if (!reserve_obs(c, w, len + 1)) return false;
    NbObs* o = c.pool + c.p_start[w];
    int k = len;
    while (k > 0 && o[k - 1].kf > kf) { o[k] = o[k - 1]; --k; }
    o[k] = NbObs{kf, idx};
    c.p_len[w] = len + 1;
    c.nobs[w] += c.kfs[kf].u_right[idx] >= 0 ? 2 : 1;
    return true;
}

// x.Replace(w), x != w (MapPoint.cc:257-309) without the descriptor, which the describe step computes
__device__ bool replace_point(Ctx& c, int x, int w) {
    const int sx = c.p_start[x], lx = c.p_len[x];
    if (!reserve_obs(c, w, min(c.p_len[w] + lx, kNbMaxObs))) return false;   // one move for the whole merge (x's own piece stays where it is)
    for (int o = 0; o < lx; ++o) {
        const NbObs ob = c.pool[sx + o];
        int32_t* slot = c.slot + c.slot_offsets[ob.kf] + ob.idx;
        if (!in_kf(c, w, ob.kf)) {
            *slot = w;
            if (!add_obs(c, w, ob.kf, ob.idx)) return false;
        } else {
            *slot = -1;
        }
    }
    c.pflag[x] |= F_BAD;
    c.p_len[x] = 0;
    c.replaced[x] = w;
    c.found[w] += c.found[x];
    c.visible[w] += c.visible[x];
    c.pflag[w] |= F_DIRTY;
    return true;
}

__device__ __forceinline__ void put_op(Ctx& c, int kind, int stage_target, int point, int occupant, int winner, int kf, int idx) {
    const int n = c.s[S_NOPS];
    if (n < c.P.op_room) {
        int32_t* r = c.ops + 8 * (size_t)n;
        r[0] = kind; r[1] = stage_target; r[2] = point; r[3] = occupant; r[4] = winner; r[5] = kf; r[6] = idx; r[7] = 0;
    }
    c.s[S_NOPS] = n + 1;
}

__device__ __forceinline__ FuseDev fuse_of(const NbKf& k, const NbConsts& cc) {
    FuseDev f{};
    f.keys = k.keys; f.desc = k.desc; f.u_right = k.u_right; f.cell_start = k.cell_start; f.items = k.items;
    f.n_keys = k.n; f.n_levels = cc.n_levels;
#pragma unroll
    for (int a = 0; a < 4; ++a) f.q[a] = k.q[a];
#pragma unroll
    for (int a = 0; a < 3; ++a) { f.t[a] = k.t[a]; f.Ow[a] = k.Ow[a]; }
    f.fx = cc.fx; f.fy = cc.fy; f.cx = cc.cx; f.cy = cc.cy; f.bf = cc.bf; f.th = 3.0f; f.log_scale_factor = cc.log_scale_factor;
    f.min_x = k.bounds[0]; f.max_x = k.bounds[1]; f.min_y = k.bounds[2]; f.max_y = k.bounds[3];
    f.scale_factors = cc.scale_factors; f.inv_level_sigma2 = cc.inv_level_sigma2;
    return f;
}

// MapPoint::ComputeDistinctiveDescriptors of point w by the calling wavefront; desc: its kNbMaxObs x kDescStride words, rows: which
// observation each row is.  A bad point or one without a descriptor to take is left as it is.
__device__ void describe_point(const Ctx& c, int w, uint32_t* desc, uint8_t* rows, int32_t* desc_kf, int32_t* desc_index, int lane) {
    const int len = c.p_len[w];
    const NbObs* obs = c.pool + c.p_start[w];
    int best_row;
    const int best = refresh::describe_rows(
        len, [=](int o) { return obs[o].kf; }, [&](int kf) { return (c.kflag[kf] & 1) != 0; },
        [&](int o) { return reinterpret_cast<const uint32_t*>(c.kfs[obs[o].kf].desc) + 8 * (size_t)obs[o].idx; }, desc, rows, lane, &best_row);
    if (best < 0) return;
    if (lane < 8) reinterpret_cast<uint32_t*>(c.points + 68 * (size_t)w + 36)[lane] = desc[best_row * kDescStride + lane];
    if (lane == 0) {
        const NbObs ob = obs[best];
        desc_kf[w] = ob.kf; desc_index[w] = ob.idx;
    }
    wave_sync_lds();  // the rows are free for the wavefront's next point
}

}  // namespace

__global__ __launch_bounds__(kNbThreads) void k_search_in_neighbors(NbBatch B) {
    __shared__ uint8_t s_pflag[kNbMaxPoints];
    __shared__ uint8_t s_kflag[kNbMaxKeyframes];
    __shared__ int16_t s_best[kNbMaxKeys];
    __shared__ uint16_t s_hits[kNbMaxKeys];
    __shared__ uint32_t s_desc[kNbThreads / 64][kNbMaxObs * kDescStride];
    __shared__ uint8_t s_rows[kNbThreads / 64][kNbMaxObs];
    __shared__ int32_t s_targets[kNbMaxTargets];
    __shared__ int32_t s_s[S_COUNT];
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    Ctx c;
    c.P = B.problems[blockIdx.x];
    const NbProblemDev& P = c.P;
    c.kfs = B.kfs + P.kf_off;
    c.slot_offsets = B.slot_offsets + P.kf_row_off;
    c.slot = B.slot_point + P.slot_off;
    c.points = B.points + 68 * (size_t)P.point_off;
    c.nobs = B.nobs + P.point_off; c.found = B.found + P.point_off; c.visible = B.visible + P.point_off;
    c.replaced = B.replaced + P.point_off;
    c.pool = B.pool + P.pool_off;
    c.p_start = B.p_start + P.point_off; c.p_len = B.p_len + P.point_off; c.p_cap = B.p_cap + P.point_off;
    c.ops = B.ops + 8 * (size_t)P.op_off;
    c.pflag = s_pflag; c.kflag = s_kflag; c.s = s_s;
    const uint8_t* kf_flags = B.kf_flags + P.kf_off;
    const int32_t* prev_kf = B.prev_kf + P.kf_off;
    const int32_t* covis_offsets = B.covis_offsets + P.kf_row_off;
    const int32_t* covis = B.covis + P.covis_off;
    const int32_t* obs_offsets = B.obs_offsets + P.point_row_off;
    int32_t* counts = B.counts + kNbCounts * (size_t)blockIdx.x;
    int32_t* targets_out = B.targets + kNbMaxTargets * (size_t)blockIdx.x;
    int32_t* target_fused = B.target_fused + kNbMaxTargets * (size_t)blockIdx.x;
    int32_t* candidates = B.candidates + P.point_off;
    int32_t* desc_kf = B.desc_kf + P.point_off;
    int32_t* desc_index = B.desc_index + P.point_off;
    int32_t* snap = B.snap + P.snap_off;
    const int n_points = P.n_points, n_kf = P.n_kf, cur = P.current;
    const bool inertial = P.flags & 1, abort_ba = P.flags & 2;

    // ---- the state as it is on entry ----
    if (tid < S_COUNT) s_s[tid] = tid == S_POOL ? P.n_obs : 0;
    for (int k = tid; k < n_kf; k += kNbThreads) s_kflag[k] = kf_flags[k] & 3;
    for (int p = tid; p < n_points; p += kNbThreads) {
        s_pflag[p] = B.point_flags[P.point_off + p] & 3;
        const int b = obs_offsets[p], n = obs_offsets[p + 1] - b;
        c.p_start[p] = b; c.p_len[p] = n; c.p_cap[p] = n;
        c.replaced[p] = -1; desc_kf[p] = -1; desc_index[p] = -1;
        const size_t g = (size_t)P.point_off + p;
        B.refreshed[g] = 0; B.min_dist[g] = 0; B.max_dist[g] = 0;
        B.normals[3 * g] = 0; B.normals[3 * g + 1] = 0; B.normals[3 * g + 2] = 0;
    }
    for (int o = tid; o < P.n_obs; o += kNbThreads) c.pool[o] = NbObs{B.obs_kf[P.obs_off + o], B.obs_index[P.obs_off + o]};
    const int cur_b = c.slot_offsets[cur], cur_n = c.slot_offsets[cur + 1] - cur_b;
    for (int i = tid; i < cur_n; i += kNbThreads) snap[i] = c.slot[cur_b + i];  // vpMapPointMatches: the row before stage 1 (:781)
    __syncthreads();

    // ---- rule 1: the targets (:731-777) ----
    if (tid == 0) {
        int nt = 0;
        const int b0 = covis_offsets[cur], n0 = min(10, covis_offsets[cur + 1] - b0);
        for (int k = 0; k < n0; ++k) {
            const int kf = covis[b0 + k];
            if (s_kflag[kf] & 3) continue;
            s_targets[nt++] = kf; s_kflag[kf] |= 2;
        }
        const int imax = nt;
        for (int i = 0; i < imax; ++i) {
            const int t = s_targets[i];
            const int b = covis_offsets[t], n = min(20, covis_offsets[t + 1] - b);
            for (int k = 0; k < n; ++k) {
                const int kf = covis[b + k];
                if ((s_kflag[kf] & 3) || kf == cur) continue;
                s_targets[nt++] = kf; s_kflag[kf] |= 2;
            }
            if (abort_ba) break;
        }
        if (inertial) {
            int kf = prev_kf[cur];
            for (int step = 0; step < n_kf && nt < 20 && kf >= 0; ++step) {  // the host refused a chain that returns to itself
                if (!(s_kflag[kf] & 3)) { s_targets[nt++] = kf; s_kflag[kf] |= 2; }
                kf = prev_kf[kf];
            }
        }
        s_s[S_NTARGETS] = nt;
    }
    __syncthreads();
    const int n_targets = s_s[S_NTARGETS];
    for (int k = tid; k < n_targets; k += kNbThreads) targets_out[k] = s_targets[k];

    // ---- ORBmatcher::Fuse of one keyframe over a list, in pieces of kNbMaxKeys entries ----
    auto fuse_list = [&](int T, const int32_t* list, int len, int ordinal) {
        const FuseDev f = fuse_of(c.kfs[T], B.c);
        const int32_t* t_slot = c.slot + c.slot_offsets[T];
        if (tid == 0) s_s[S_FUSED] = 0;
        for (int c0 = 0; c0 < len; c0 += kNbMaxKeys) {
            const int m = min(kNbMaxKeys, len - c0);
            for (int i = tid; i < m; i += kNbThreads) {  // search
                const int p = list[c0 + i];
                int bi = -1, bd = 256;
                if (p >= 0 && !(s_pflag[p] & F_BAD) && !in_kf(c, p, T))
                    fuse_search_one(f, reinterpret_cast<const float*>(c.points + 68 * (size_t)p), &bi, &bd);
                s_best[i] = (int16_t)bi;
            }
            __syncthreads();
            if (wave == 0) {  // compact
                int run = 0;
                for (int base = 0; base < m; base += 64) {
                    const int i = base + lane;
                    const bool hit = i < m && s_best[i] >= 0;
                    const unsigned long long mask = __ballot(hit);
                    if (hit) s_hits[run + lane_rank(mask)] = (uint16_t)i;
                    run += __popcll(mask);
                }
                if (lane == 0) s_s[S_NHITS] = run;
            }
            __syncthreads();
            if (tid == 0 && s_s[S_STATUS] == 0) {  // apply, in list order (ORBmatcher.cc:1321-1340)
                const int nh = s_s[S_NHITS];
                int fused = s_s[S_FUSED];
                for (int h = 0; h < nh; ++h) {
                    const int i = s_hits[h], p = list[c0 + i], b = s_best[i];
                    if ((s_pflag[p] & F_BAD) || in_kf(c, p, T)) continue;
                    const int q = t_slot[b];
                    if (q < 0) {
                        if (!add_obs(c, p, T, b)) break;
                        c.slot[c.slot_offsets[T] + b] = p;
                        put_op(c, TC2LI_NEIGHBORS_ADD_OBSERVATION, ordinal, p, -1, -1, T, b);
                    } else if (!(s_pflag[q] & F_BAD) && q != p) {
                        const bool q_wins = c.nobs[q] > c.nobs[p];
                        if (!(q_wins ? replace_point(c, p, q) : replace_point(c, q, p))) break;
                        put_op(c, TC2LI_NEIGHBORS_REPLACE, ordinal, p, q, q_wins ? q : p, T, b);
                        // A winner holds the keyframe's row afterwards when every slot's point has the matching observation.  Where a
                        // slot held a point without one, the winner may still be outside the keyframe with an entry ahead in this
                        // piece, and the reference searches that entry with the winner's new state: the host twin takes the problem.
                        const int w = q_wins ? q : p;
                        if (!in_kf(c, w, T)) {
                            for (int j = i + 1; j < m; ++j)
                                if (list[c0 + j] == w) { s_s[S_STATUS] = 1; break; }
                            if (s_s[S_STATUS] != 0) break;
                        }
                    }
                    ++fused;
                }
                s_s[S_FUSED] = fused;
            }
            __syncthreads();
            if (s_s[S_STATUS] != 0) return;
            for (int base = wave * 64; base < n_points; base += kNbThreads) {  // describe the winners
                const int p = base + lane;
                unsigned long long mask = __ballot(p < n_points && (s_pflag[p] & (F_DIRTY | F_BAD)) == F_DIRTY);
                if (p < n_points) s_pflag[p] &= ~F_DIRTY;
                while (mask) {
                    const int k = __ffsll((long long)mask) - 1;
                    mask &= mask - 1;
                    describe_point(c, base + k, s_desc[wave], s_rows[wave], desc_kf, desc_index, lane);
                }
            }
            __syncthreads();
        }
    };

    // ---- rule 2: stage 1 (:781-788) ----
    for (int ti = 0; ti < n_targets; ++ti) {
        fuse_list(s_targets[ti], snap, cur_n, ti);
        if (s_s[S_STATUS] != 0) break;
        if (tid == 0) { target_fused[ti] = s_s[S_FUSED]; s_s[S_FUSED1] += s_s[S_FUSED]; }
        __syncthreads();
    }
    if (s_s[S_STATUS] != 0) {  // uniform: read after a barrier
        if (tid == 0) counts[kNbStatus] = TC2LI_NEIGHBORS_ON_HOST;
        return;
    }

    if (!abort_ba) {  // rule 5
        // ---- rule 6: the candidates (:795-814), wavefront 0: 64 slots at a time, duplicates inside the 64 settled by the lower lane ----
        if (wave == 0) {
            int nc = 0;
            for (int ti = 0; ti < n_targets; ++ti) {
                const int T = s_targets[ti];
                const int b = c.slot_offsets[T], n = c.slot_offsets[T + 1] - b;
                for (int base = 0; base < n; base += 64) {
                    const int i = base + lane;
                    const int p = i < n ? c.slot[b + i] : -1;
                    bool take = p >= 0 && !(s_pflag[p] & (F_BAD | F_MARK));
                    if (__ballot(take)) {
                        for (int l = 0; l < 63; ++l) {
                            const int pl = __shfl(p, l, 64);
                            const int tl = __shfl((int)take, l, 64);
                            if (l < lane && tl && pl == p) take = false;
                        }
                    }
                    const unsigned long long mask = __ballot(take);
                    if (take) { candidates[nc + lane_rank(mask)] = p; s_pflag[p] |= F_MARK; }
                    nc += __popcll(mask);
                    wave_sync_lds();
                }
            }
            if (lane == 0) s_s[S_NCAND] = nc;
        }
        __syncthreads();
        fuse_list(cur, candidates, s_s[S_NCAND], n_targets);  // :816
        if (s_s[S_STATUS] != 0) {
            if (tid == 0) counts[kNbStatus] = TC2LI_NEIGHBORS_ON_HOST;
            return;
        }
        if (tid == 0) s_s[S_FUSED2] = s_s[S_FUSED];
        // ---- rule 7: the refresh (:821-833) ----
        for (int i = tid; i < cur_n; i += kNbThreads) {
            const int p = c.slot[cur_b + i];
            if (p >= 0 && !(s_pflag[p] & F_BAD)) s_pflag[p] |= F_REFRESH;  // two slots with one point store the same byte
        }
        __syncthreads();
        for (int base = wave * 64; base < n_points; base += kNbThreads) {
            const int p0 = base + lane;
            unsigned long long mask = __ballot(p0 < n_points && (s_pflag[p0] & F_REFRESH));
            while (mask) {
                const int k = __ffsll((long long)mask) - 1;
                mask &= mask - 1;
                const int p = base + k;
                describe_point(c, p, s_desc[wave], s_rows[wave], desc_kf, desc_index, lane);
                const int N = c.p_len[p];
                if (lane == 0 && N > 0) {  // MapPoint::UpdateNormalAndDepth in the order of k_map_points_refresh
                    const float* X = reinterpret_cast<const float*>(c.points + 68 * (size_t)p);
                    const NbObs* ob = c.pool + c.p_start[p];
                    const size_t g = (size_t)P.point_off + p;
                    refresh::normal_and_depth(X, N, [&](int o) { return c.kfs[ob[o].kf].Ow; }, c.kfs[B.ref_kf[g]].Ow, B.ref_scale[g], P.last_level_scale,
                                              B.normals + 3 * g, B.min_dist + g, B.max_dist + g);
                    B.refreshed[g] = 1;
                    atomicAdd(&s_s[S_NREFRESHED], 1);
                }
            }
        }
        __syncthreads();
    }

    // ---- the end state ----
    int32_t* off_out = B.obs_offsets_out + P.point_row_off;
    if (tid == 0) {
        int run = 0;
        for (int p = 0; p < n_points; ++p) { off_out[p] = run; run += c.p_len[p]; }
        off_out[n_points] = run;
        counts[kNbStatus] = TC2LI_NEIGHBORS_ON_DEVICE; counts[kNbTargets] = n_targets; counts[kNbCandidates] = s_s[S_NCAND];
        counts[kNbOps] = s_s[S_NOPS]; counts[kNbObs] = run; counts[kNbRefreshed] = s_s[S_NREFRESHED];
        counts[kNbFused1] = s_s[S_FUSED1]; counts[kNbFused2] = s_s[S_FUSED2];
    }
    __syncthreads();
    const bool obs_fit = off_out[n_points] <= P.obs_out_room;
    for (int p = tid; p < n_points; p += kNbThreads) {
        const bool bad = s_pflag[p] & F_BAD;
        B.bad[P.point_off + p] = bad ? 1 : 0;
        if (bad) { desc_kf[p] = -1; desc_index[p] = -1; }
        if (obs_fit) {
            const NbObs* ob = c.pool + c.p_start[p];
            const int n = c.p_len[p], at = P.obs_out_off + off_out[p];
            for (int o = 0; o < n; ++o) { B.obs_kf_out[at + o] = ob[o].kf; B.obs_index_out[at + o] = ob[o].idx; }
        }
    }
}

void launch_search_in_neighbors(const NbBatch& B, int n_problems, hipStream_t st) {
    if (n_problems > 0) TC2LI_LAUNCH(k_search_in_neighbors, dim3(n_problems), dim3(kNbThreads), 0, st, B);
}

}  // namespace tc2li

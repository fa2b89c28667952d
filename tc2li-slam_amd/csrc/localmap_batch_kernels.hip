// Tracking::UpdateLocalMap (SF/src/Tracking.cc:3286-3476) for a batch of sequences: the loops of localmap_kernels.hip, one problem per
// workgroup (keyframe phase) or per kLmbPointGroups workgroups (point phase), so that a call's launches do not grow with the batch.
//   k_lmb_keyframes  one workgroup per problem: the votes of the frame's points (integer atomics in LDS, or in the work buffer above
//                    kLmbLdsKeyframes keyframes), the voted keyframes in index order (ballot compaction), the first keyframe with the most
//                    votes (packed 64-bit max), then one lane walks the dependent chain -- at most 81 visits of three tests each and 20
//                    temporal rounds -- and the workgroup lays out the reversed concatenation of the local keyframes' match lists
//   k_lmb_first      a problem's reversed concatenation cut into kLmbPointGroups contiguous slices, one workgroup each: the first position
//                    at which a point occurs (atomicMax of 0x7fffffff - position on keys that start at 0)
//   k_lmb_count      kept entries (first occurrences) per slice
//   k_lmb_scan       one workgroup: local points per problem, where every problem's lists and every slice's entries start
//   k_lmb_scatter    ordered compaction of the first occurrences = mvpLocalMapPoints in the reference's order, behind the problem's local
//                    keyframes in one list without gaps: the host downloads exactly what was found
// A phase that needs another's result across workgroups starts at a kernel boundary; nothing else passes between workgroups.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#include <stdint.h>

#include "../../include/tc2li_hip.h"
#include "localmap_batch_device.hpp"

namespace tc2li {
namespace {

constexpr int kWaves = kLmbThreads / 64;

// exclusive position of every kept lane in thread order, *total = the workgroup's kept lanes; two barriers: ALL threads arrive
__device__ __forceinline__ int ballot_rank(int keep, int* s_cnt, int* total) {
    const unsigned long long bal = __ballot(keep);
    const int lane = threadIdx.x & 63, wave = wave_in_block();
    if (lane == 0) s_cnt[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) {
        const int c = s_cnt[w];
        if (w < wave) base += c;
        tot += c;
    }
    __syncthreads();
    *total = tot;
    return base + __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
}

// the counters are written by atomics only; a read that cannot be served from a line the vector cache held before them
__device__ __forceinline__ int vote_of(const int* votes, int kf) { return __hip_atomic_load(votes + kf, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct LmbShared {
    int cnt[kWaves];
    unsigned long long best;
    int n_cleared, n_list;
};

// votes / marked: [n_keyframes], zero on entry
__device__ __forceinline__ void keyframes_of_problem(const LmbBatch& B, const LmbProblem& pr, int problem, int* votes, uint8_t* marked, LmbShared& s) {
    const LocalMapDev& m = pr.map;
    const int K = m.n_keyframes, tid = threadIdx.x;
    int32_t* kf_list = B.kf_list + pr.list_off;
    int32_t* rev_base = B.rev_base + pr.list_off + problem;
    // ---- :3329-3347 the votes of the frame's points; bad points are reported ----
    int n_cleared = 0;
    for (int i = tid; i < pr.n_fp; i += kLmbThreads) {
        const int p = B.frame_points[pr.fp_off + i];
        uint8_t c = 0;
        if (p >= 0) {
            if (!m.point_bad[p]) {
                for (int k = m.obs_off[p]; k < m.obs_off[p + 1]; ++k) atomicAdd(votes + m.obs_kf[k], 1);
            } else {
                c = 1;
            }
        }
        B.cleared[pr.fp_off + i] = c;
        n_cleared += c;
    }
    if (n_cleared) atomicAdd(&s.n_cleared, n_cleared);
    __threadfence_block();
    __syncthreads();
    // ---- :3382-3397 the voted, not-bad keyframes in index order; the first one with the most votes ----
    int n_list = 0;
    for (int chunk = 0; chunk < K; chunk += kLmbThreads) {
        const int kf = chunk + tid;
        const int v = kf < K ? vote_of(votes, kf) : 0;
        const int keep = v > 0 && !m.kf_bad[kf];
        int tot;
        const int at = ballot_rank(keep, s.cnt, &tot);
        if (keep) {
            kf_list[n_list + at] = kf;
            marked[kf] = 1;
            // more votes win; among equal votes the lower index (the reference's `>` keeps the first it meets)
            atomicMax(&s.best, ((unsigned long long)(unsigned)v << 32) | (unsigned)(0x7fffffff - kf));
        }
        n_list += tot;
    }
    __threadfence_block();
    __syncthreads();
    const int n_voted = n_list;
    if (tid == 0) {
        // ---- :3400-3451 extensions: a chain of dependent steps over the voted keyframes only ----
        for (int j = 0; j < n_voted; ++j) {
            if (n_list > 80) break;
            const int kf = kf_list[j];
            const int ce = min(m.covis_off[kf + 1], m.covis_off[kf] + 10);  // GetBestCovisibilityKeyFrames(10)
            for (int k = m.covis_off[kf]; k < ce; ++k) {
                const int n = m.covis[k];
                if (!m.kf_bad[n] && !marked[n]) { kf_list[n_list++] = n; marked[n] = 1; break; }
            }
            for (int k = m.child_off[kf]; k < m.child_off[kf + 1]; ++k) {
                const int c = m.children[k];
                if (!m.kf_bad[c] && !marked[c]) { kf_list[n_list++] = c; marked[c] = 1; break; }
            }
            const int par = m.parent[kf];
            if (par >= 0 && !marked[par]) { kf_list[n_list++] = par; marked[par] = 1; break; }  // the reference's break leaves the keyframe loop
        }
        // ---- :3453-3469 the temporal block: 20 rounds, a step along prev_kf only after a push ----
        if (pr.temporal_last_kf >= 0 && n_list < 80) {
            int t = pr.temporal_last_kf;
            for (int i = 0; i < 20 && t >= 0; ++i)
                if (!marked[t]) { kf_list[n_list++] = t; marked[t] = 1; t = m.prev_kf[t]; }
        }
        s.n_list = n_list;
    }
    __threadfence_block();
    __syncthreads();
    n_list = s.n_list;
    // ---- UpdateLocalPoints walks the local keyframes backwards: where their match lists start in that concatenation ----
    int run = 0;
    for (int chunk = 0; chunk < n_list; chunk += kLmbThreads) {
        const int jr = chunk + tid;
        int len = 0;
        if (jr < n_list) {
            const int kf = kf_list[n_list - 1 - jr];
            len = m.match_off[kf + 1] - m.match_off[kf];
        }
        int tot;
        const int at = block_scan_excl<kLmbThreads>(len, s.cnt, &tot);
        if (jr < n_list) rev_base[jr] = run + at;
        run += tot;
    }
    if (tid == 0) {
        rev_base[n_list] = run;
        B.info[2 * problem] = n_list;
        B.info[2 * problem + 1] = run;
        int32_t* c = B.counts + (size_t)problem * TC2LI_LOCAL_MAP_COUNTS;
        c[TC2LI_LOCAL_MAP_N_KEYFRAMES] = n_list;
        c[TC2LI_LOCAL_MAP_N_VOTED] = n_voted;
        c[TC2LI_LOCAL_MAP_REFERENCE_KF] = s.best ? 0x7fffffff - (int)(unsigned)(s.best & 0xffffffffull) : -1;
        c[TC2LI_LOCAL_MAP_N_POINTS] = 0;  // k_lmb_scan
        c[TC2LI_LOCAL_MAP_N_CLEARED] = s.n_cleared;
        for (int i = TC2LI_LOCAL_MAP_N_CLEARED + 1; i < TC2LI_LOCAL_MAP_COUNTS; ++i) c[i] = 0;
    }
}

}  // namespace

__global__ __launch_bounds__(kLmbThreads) void k_lmb_keyframes(LmbBatch B) {
    __shared__ int s_votes[kLmbLdsKeyframes];
    __shared__ uint8_t s_marked[kLmbLdsKeyframes];
    __shared__ LmbShared s;
    const int problem = blockIdx.x;
    const LmbProblem& pr = B.problems[problem];
    if (threadIdx.x == 0) { s.best = 0ull; s.n_cleared = 0; s.n_list = 0; }
    if (pr.vote_off < 0) {   // the same in the whole workgroup
        for (int k = threadIdx.x; k < pr.map.n_keyframes; k += kLmbThreads) { s_votes[k] = 0; s_marked[k] = 0; }
        __syncthreads();
        keyframes_of_problem(B, pr, problem, s_votes, s_marked, s);
    } else {
        __syncthreads();
        keyframes_of_problem(B, pr, problem, B.votes + pr.vote_off, B.marks + pr.vote_off, s);
    }
}

namespace {

// entry `pos` of the problem's reversed concatenation -> the map point there, or -1 (empty slot / bad point)
__device__ __forceinline__ int entry_point(const LocalMapDev& m, const int32_t* kf_list, const int32_t* rev_base, int n_local, int pos) {
    int lo = 0, hi = n_local;  // rev_base[lo] <= pos < rev_base[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (rev_base[mid] <= pos) lo = mid; else hi = mid;
    }
    const int kf = kf_list[n_local - 1 - lo];
    const int p = m.matches[m.match_off[kf] + (pos - rev_base[lo])];
    return p >= 0 && !m.point_bad[p] ? p : -1;
}

// the slice [*lo, *hi) of the problem's reversed concatenation that workgroup `group` of the problem takes
__device__ __forceinline__ void slice_of(int total, int group, int* lo, int* hi) {
    const int per = (total + kLmbPointGroups - 1) / kLmbPointGroups;
    *lo = min(group * per, total);
    *hi = min(*lo + per, total);
}

constexpr int kFirstKey = 0x7fffffff;

}  // namespace

__global__ __launch_bounds__(kLmbThreads) void k_lmb_first(LmbBatch B) {
    const int problem = blockIdx.x / kLmbPointGroups, group = blockIdx.x % kLmbPointGroups;
    const LmbProblem& pr = B.problems[problem];
    const int n_local = B.info[2 * problem];
    int lo, hi;
    slice_of(B.info[2 * problem + 1], group, &lo, &hi);
    for (int pos = lo + (int)threadIdx.x; pos < hi; pos += kLmbThreads) {
        const int p = entry_point(pr.map, B.kf_list + pr.list_off, B.rev_base + pr.list_off + problem, n_local, pos);
        if (p >= 0) atomicMax(B.keys + pr.key_off + p, kFirstKey - pos);
    }
}

__global__ __launch_bounds__(kLmbThreads) void k_lmb_count(LmbBatch B) {
    __shared__ int s_cnt[kWaves];
    const int problem = blockIdx.x / kLmbPointGroups, group = blockIdx.x % kLmbPointGroups;
    const LmbProblem& pr = B.problems[problem];
    const int n_local = B.info[2 * problem];
    int lo, hi;
    slice_of(B.info[2 * problem + 1], group, &lo, &hi);
    int kept = 0;
    for (int pos = lo + (int)threadIdx.x; pos < hi; pos += kLmbThreads) {
        const int p = entry_point(pr.map, B.kf_list + pr.list_off, B.rev_base + pr.list_off + problem, n_local, pos);
        kept += p >= 0 && B.keys[pr.key_off + p] == kFirstKey - pos;
    }
    kept = wave_sum_i32(kept);
    if ((threadIdx.x & 63) == 0) s_cnt[wave_in_block()] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
        for (int w = 0; w < kWaves; ++w) sum += s_cnt[w];
        B.block_counts[blockIdx.x] = sum;
    }
}

__global__ __launch_bounds__(kLmbThreads) void k_lmb_scan(LmbBatch B) {
    __shared__ int s_cnt[kWaves];
    int run = 0;
    for (int chunk = 0; chunk < B.n_problems; chunk += kLmbThreads) {
        const int problem = chunk + (int)threadIdx.x;
        int n_kf = 0, n_pts = 0;
        if (problem < B.n_problems) {
            n_kf = B.info[2 * problem];
            for (int g = 0; g < kLmbPointGroups; ++g) n_pts += B.block_counts[problem * kLmbPointGroups + g];
        }
        int tot;
        const int at = run + block_scan_excl<kLmbThreads>(n_kf + n_pts, s_cnt, &tot);
        if (problem < B.n_problems) {
            B.seg[problem] = at;
            B.counts[(size_t)problem * TC2LI_LOCAL_MAP_COUNTS + TC2LI_LOCAL_MAP_N_POINTS] = n_pts;
            int base = at + n_kf;
            for (int g = 0; g < kLmbPointGroups; ++g) {
                B.block_base[problem * kLmbPointGroups + g] = base;
                base += B.block_counts[problem * kLmbPointGroups + g];
            }
        }
        run += tot;
    }
    if (threadIdx.x == 0) B.seg[B.n_problems] = run;
}

__global__ __launch_bounds__(kLmbThreads) void k_lmb_scatter(LmbBatch B) {
    __shared__ int s_cnt[kWaves];
    const int problem = blockIdx.x / kLmbPointGroups, group = blockIdx.x % kLmbPointGroups;
    const LmbProblem& pr = B.problems[problem];
    const int n_local = B.info[2 * problem];
    const int32_t* kf_list = B.kf_list + pr.list_off;
    // the local keyframes in front of the points
    for (int j = group * kLmbThreads + (int)threadIdx.x; j < n_local; j += kLmbPointGroups * kLmbThreads) B.lists[B.seg[problem] + j] = kf_list[j];
    int lo, hi;
    slice_of(B.info[2 * problem + 1], group, &lo, &hi);
    int at = B.block_base[blockIdx.x];
    for (int tile = lo; tile < hi; tile += kLmbThreads) {   // the same bounds in all threads: ballot_rank has barriers
        const int pos = tile + (int)threadIdx.x;
        int keep = 0, p = -1;
        if (pos < hi) {
            p = entry_point(pr.map, kf_list, B.rev_base + pr.list_off + problem, n_local, pos);
            keep = p >= 0 && B.keys[pr.key_off + p] == kFirstKey - pos;
        }
        int tot;
        const int rank = ballot_rank(keep, s_cnt, &tot);
        if (keep) B.lists[at + rank] = p;
        at += tot;
    }
}

void launch_local_map_batch(const LmbBatch& B, hipStream_t st) {
    const dim3 per_problem(B.n_problems), per_slice(B.n_problems * kLmbPointGroups), threads(kLmbThreads);
    TC2LI_LAUNCH(k_lmb_keyframes, per_problem, threads, 0, st, B);
    TC2LI_LAUNCH(k_lmb_first, per_slice, threads, 0, st, B);
    TC2LI_LAUNCH(k_lmb_count, per_slice, threads, 0, st, B);
    TC2LI_LAUNCH(k_lmb_scan, dim3(1), threads, 0, st, B);
    TC2LI_LAUNCH(k_lmb_scatter, per_slice, threads, 0, st, B);
}

}  // namespace tc2li

// Relocalisation on the device (reloc_host.cpp sequences it):
//   * score_wave / k_bow_score: TemplatedVocabulary::score (SF/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311) -- one wavefront per pair of
//     BowVectors.  The lanes take 64 consecutive entries of one vector and binary-search the other (both ascending: the
//     reference's lower_bound walk visits exactly the common words, in ascending order); a ballot marks the common words, and their
//     terms are added one at a time in lane order -- ascending word order -- into one double, each broadcast from its lane by a readlane.
//     The chain of dependent f64 adds is what the reference computes; a tree sum would change the bits.
//   * k_reloc_rows: the same for one (query, keyframe row) per wavefront of KeyFrameDatabase::DetectRelocalizationCandidates
//     (SF/src/KeyFrameDatabase.cc:742-854): mnRelocWords, the smallest shared word (the ordering key) and si.  The keyframe's row is
//     the vector walked (streamed once, coalesced), the frame's words are searched in LDS.
//   * k_reloc_select: the rest of the query, one workgroup per query: the word gate (:771-796), lKFsSharingWords order by a bitonic sort of
//     (smallest shared word, pool row) in LDS, the covisibility accumulation (:805-830), the 0.75 gate, the map filter and the
//     first-occurrence rule (:833-851).
//   * k_reloc_ladder_*: the bookkeeping of the refinement ladder after a PnP pose (SF/src/Tracking.cc:3562-3631) around the
//     pose-optimisation kernel and the keyframe overload of SearchByProjection, every branch decided on the device.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <limits.h>
#include <stdint.h>

#include "reloc_device.hpp"

namespace tc2li {

namespace {

enum { kL1 = 0, kL2 = 1, kChi = 2, kKL = 3, kBhat = 4, kDot = 5 };

__device__ __forceinline__ double lane_value(double v, int src) {  // v of lane src (wave-uniform), in every lane
    const int s = __builtin_amdgcn_readfirstlane(src);
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), s), __builtin_amdgcn_readlane(__double2loint(v), s));
}

// The closed score of two BowVectors: the lanes walk 64 consecutive entries of one vector (ws, ns) and binary-search the other (wl, nl;
// global memory or LDS); walk_is_v1 says which of the two is score()'s first argument, whose value is vi.  All 64 lanes of the wavefront
// must call it with the same arguments.  common: number of common words; first: the smallest of them, -1 without one.
__device__ __forceinline__ double score_wave(const int32_t* __restrict__ ws, const double* __restrict__ vs, int ns, const int32_t* wl,
                                             const double* __restrict__ vl, int nl, bool walk_is_v1, int scoring, int& common, int& first) {
    const int lane = threadIdx.x & 63;
    double score = 0.0;
    common = 0;
    first = -1;
    for (int base = 0; base < ns; base += 64) {
        const int i = base + lane;
        const bool valid = i < ns;
        const int word = valid ? ws[i] : 0;
        int lo = 0, hi = valid ? nl : 0;
        while (lo < hi) {  // lower_bound
            const int mid = (lo + hi) >> 1;
            if (wl[mid] < word) lo = mid + 1; else hi = mid;
        }
        const bool hit = valid && lo < nl && wl[lo] == word;
        bool use = hit;
        double term = 0.0;
        if (hit) {
            const double a = vs[i], b = vl[lo];
            const double vi = walk_is_v1 ? a : b, wi = walk_is_v1 ? b : a;
            switch (scoring) {
                case kL1: term = fabs(vi - wi) - fabs(vi) - fabs(wi); break;
                case kChi:
                    if (vi + wi != 0.0) term = vi * wi / (vi + wi); else use = false;
                    break;
                case kBhat: term = sqrt(vi * wi); break;
                default: term = vi * wi; break;  // L2_NORM, DOT_PRODUCT
            }
        }
        const unsigned long long hits = __ballot(hit);
        unsigned long long terms = __ballot(use);
        if (hits != 0 && first < 0) first = __builtin_amdgcn_readlane(word, __builtin_amdgcn_readfirstlane(__ffsll((long long)hits) - 1));
        common += __popcll(hits);
        while (terms != 0) {
            score += lane_value(term, __ffsll((long long)terms) - 1);
            terms &= terms - 1;
        }
    }
    switch (scoring) {
        case kL1: score = -score / 2.0; break;
        case kL2: score = score >= 1 ? 1.0 : 1.0 - sqrt(1.0 - score); break;
        case kChi: score = 2. * score; break;
        default: break;
    }
    return score;
}

__global__ __launch_bounds__(256) void k_bow_score(const RelocPairDev* __restrict__ pairs, int n_pairs, const int32_t* __restrict__ word,
                                                   const double* __restrict__ value, int scoring, double* __restrict__ out) {
    const int p = blockIdx.x * 4 + wave_in_block();
    if (p >= n_pairs) return;
    const RelocPairDev P = pairs[p];
    int common, first;
    const bool walk1 = P.n1 <= P.n2;  // walk the shorter vector, search the longer one
    const int a = walk1 ? P.off1 : P.off2, na = walk1 ? P.n1 : P.n2, b = walk1 ? P.off2 : P.off1, nb = walk1 ? P.n2 : P.n1;
    const double s = score_wave(word + a, value + a, na, word + b, value + b, nb, walk1, scoring, common, first);
    if ((threadIdx.x & 63) == 0) out[p] = s;
}

// One wavefront per (query, keyframe row); the four rows of a workgroup belong to one query, whose words are staged in LDS once: every
// wavefront streams its row (coalesced) and searches the frame's words there.
__global__ __launch_bounds__(256) void k_reloc_rows(RelocArgs A) {
    __shared__ int32_t s_fword[kRelocMaxWords];
    const int q = blockIdx.y;
    const int r = blockIdx.x * 4 + wave_in_block();
    const RelocQueryDev Q = A.queries[q];
    if (blockIdx.x * 4 >= Q.n_rows) return;  // the whole workgroup
    for (int i = threadIdx.x; i < Q.f_n; i += 256) s_fword[i] = A.f_word[Q.f_off + i];
    __syncthreads();
    if (r >= Q.n_rows) return;
    const RelocRowDev* row = Q.rows + r;
    int common = 0, first = -1;
    double s = 0.0;
    if (row->live) {
        const int off = row->off;
        s = score_wave(Q.kf_word + off, Q.kf_value + off, row->n, s_fword, A.f_value + Q.f_off, Q.f_n, false, A.scoring, common, first);
    }
    if ((threadIdx.x & 63) == 0) {
        A.common[Q.row_off + r] = common;
        A.first_word[Q.row_off + r] = first;
        A.si[Q.row_off + r] = (float)s;
    }
}

constexpr int kSelThreads = 1024;

__global__ __launch_bounds__(kSelThreads) void k_reloc_select(RelocArgs A) {
    // the sort keys, and after the sort's last use the first list position of every best keyframe (ints over the same bytes)
    __shared__ unsigned long long s_key[kRelocMaxLive];
    __shared__ int s_scan[kSelThreads];
    __shared__ int s_max_words, s_gated;
    __shared__ unsigned s_best_acc;
    const int q = blockIdx.x, tid = threadIdx.x;
    const RelocQueryDev Q = A.queries[q];
    const int R = Q.n_rows;
    const int32_t* common = A.common + Q.row_off;
    const int32_t* first_word = A.first_word + Q.row_off;
    const float* si = A.si + Q.row_off;
    const size_t lo = (size_t)q * A.list_cap;
    if (tid == 0) { s_max_words = 0; s_gated = 0; s_best_acc = 0; }
    __syncthreads();
    {   // maxCommonWords (:771-776)
        int m = 0;
        for (int r = tid; r < R; r += kSelThreads) m = max(m, common[r]);
        if (m > 0) atomicMax(&s_max_words, m);
    }
    __syncthreads();
    const int min_words = (int)((float)s_max_words * 0.8f);  // :778
    // the keyframes that pass the word gate take their si as score state (:785-796); none when no keyframe shares a word (:767)
    for (int r = tid; r < R; r += kSelThreads) {
        const int c = common[r];
        if (c > 0 && c > min_words) {
            const int slot = atomicAdd(&s_gated, 1);
            if (slot < kRelocMaxLive) s_key[slot] = ((unsigned long long)(unsigned)first_word[r] << 32) | (unsigned)r;
            Q.score[r] = si[r];
        }
    }
    __syncthreads();
    const int G = min(s_gated, kRelocMaxLive);
    int P = 1;
    while (P < G) P <<= 1;
    for (int i = G + tid; i < P; i += kSelThreads) s_key[i] = ~0ull;
    __syncthreads();
    // lKFsSharingWords order: (smallest shared word, sequence number); the pool's rows are in sequence order
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += kSelThreads) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = s_key[i], b = s_key[x];
                    if (((i & k) == 0) == (a > b)) { s_key[i] = b; s_key[x] = a; }
                }
            }
            __syncthreads();
        }
    // accumulate the score over the covisibility list (:805-830)
    for (int i = tid; i < G; i += kSelThreads) {
        const int r = (int)(unsigned)s_key[i];
        const RelocRowDev* row = Q.rows + r;
        float best_score = si[r];
        float acc = best_score;
        int best = r;
        const int nc = row->n_cov;
        for (int k = 0; k < nc; ++k) {
            const int r2 = row->cov[k];
            if (r2 < 0 || common[r2] <= 0) continue;  // mnRelocQuery != F->mnId
            const float s2 = Q.score[r2];
            acc += s2;
            if (s2 > best_score) { best = r2; best_score = s2; }
        }
        if (i < A.list_cap) {
            A.sc_row[lo + i] = r; A.sc_kf[lo + i] = row->kf_id; A.sc_words[lo + i] = common[r]; A.sc_si[lo + i] = si[r];
            A.sc_acc[lo + i] = acc; A.sc_best_row[lo + i] = best; A.sc_best[lo + i] = Q.rows[best].kf_id;
        }
        // bestAccScore starts at 0 and only a greater accScore replaces it (:802, 828): the maximum over the positive ones, whose float
        // bits order like unsigned integers
        if (acc > 0.0f) atomicMax(&s_best_acc, __float_as_uint(acc));
    }
    __syncthreads();
    const float min_score = 0.75f * __uint_as_float(s_best_acc);  // :833
    int* s_first = reinterpret_cast<int*>(s_key);                  // [2 * kRelocMaxLive] >= R
    for (int r = tid; r < R; r += kSelThreads) s_first[r] = INT_MAX;
    __syncthreads();
    const int L = min(G, A.list_cap);
    for (int i = tid; i < L; i += kSelThreads) {
        const int b = A.sc_best_row[lo + i];
        if (A.sc_acc[lo + i] > min_score && Q.rows[b].map_id == Q.map_id) atomicMin(&s_first[b], i);
    }
    __syncthreads();
    // the candidates in list order: every thread owns `per` consecutive entries, an exclusive scan over the threads places them
    const int per = (L + kSelThreads - 1) / kSelThreads;
    const int i0 = tid * per, i1 = min(i0 + per, L);
    int mine = 0;
    for (int i = i0; i < i1; ++i) mine += s_first[A.sc_best_row[lo + i]] == i;
    s_scan[tid] = mine;
    __syncthreads();
    for (int d = 1; d < kSelThreads; d <<= 1) {
        const int v = tid >= d ? s_scan[tid - d] : 0;
        __syncthreads();
        s_scan[tid] += v;
        __syncthreads();
    }
    int pos = s_scan[tid] - mine;
    for (int i = i0; i < i1; ++i)
        if (s_first[A.sc_best_row[lo + i]] == i) {
            if (pos < A.capacity) A.candidates[(size_t)q * A.capacity + pos] = A.sc_best[lo + i];
            ++pos;
        }
    if (tid == kSelThreads - 1) { A.n_candidates[q] = s_scan[tid]; A.n_scored[q] = s_gated; }
}


// ---- the refinement ladder (SF/src/Tracking.cc:3562-3631); one workgroup per hypothesis ----------------------------------------------
// :3568-3581: mvpMapPoints[j] = vvpMapPointMatches[i][j] where vbInliers[j], else NULL; sFound = those points
__global__ __launch_bounds__(256) void k_reloc_ladder_init(RelocLadder L) {
    const int h = blockIdx.x, tid = threadIdx.x;
    const TrackFrameDev& F = L.frames[h];
    const size_t base = (size_t)h * L.capacity;
    for (int q = tid; q < F.n_q; q += 256) L.found[F.q_off + q] = 0;
    __syncthreads();
    for (int i = tid; i < L.capacity; i += 256) {
        int m = -1;
        if (i < F.n_keys && L.in_inlier[base + i]) m = L.in_match[base + i];
        if (m >= F.n_q) m = -1;
        L.assign[base + i] = m;
        L.outlier_of_key[base + i] = 0;
        if (m >= 0) L.found[F.q_off + m] = 1;
    }
    if (tid == 0) {
        L.active[h] = 1; L.status[h] = 0; L.n_good[h] = 0; L.n_additional[2 * h] = 0; L.n_additional[2 * h + 1] = 0; L.n_matches[h] = 0;
    }
    for (int k = tid; k < 21; k += 256) L.stage_poses[21 * (size_t)h + k] = 0.0;
}

// The edges of Optimizer::PoseOptimization over every keypoint that holds a point, in keypoint order (stereo when uRight >= 0), at the frame's
// current pose -- for the hypotheses that reach PoseOptimization number `stage`: all (0), nadditional + nGood >= 50 after the first search (1,
// :3597), nGood + nadditional >= 50 after the second (2, :3612).  The others get no edges.
__global__ __launch_bounds__(256) void k_reloc_ladder_edges(RelocLadder L, int stage) {
    const int h = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    const TrackFrameDev& F = L.frames[h];
    const int base = h * L.capacity;
    __shared__ int s_wave[4];
    bool act = L.active[h] != 0;
    if (stage > 0 && act) {
        const int nadd = L.n_matches[h];
        act = nadd + L.n_good[h] >= 50;
        if (tid == 0) { L.n_additional[2 * h + stage - 1] = nadd; L.status[h] |= stage == 1 ? kRelocSearch1 : kRelocSearch2; }
    }
    __syncthreads();  // every thread has read active / n_good
    if (tid == 0) { L.active[h] = act ? 1 : 0; L.frames[h].slot = -1; }
    if (!act) { if (tid == 0) L.probs[h] = PoseProblem{base, 0}; return; }
    if (tid < 7) L.poses[7 * h + tid] = (double)F.pose7[tid];
    const float* ur = L.u_right + (size_t)L.frame_of_hyp[h] * L.capacity;
    int carry = 0;
    for (int i0 = 0; i0 < F.n_keys; i0 += 256) {
        const int i = i0 + tid;
        const int m = i < F.n_keys ? L.assign[base + i] : -1;
        int incl = m >= 0 ? 1 : 0;
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int before = 0, tot = 0;
        for (int k = 0; k < 4; ++k) { const int w = s_wave[k]; before += k < wave ? w : 0; tot += w; }
        __syncthreads();
        if (m >= 0) {
            const int e = carry + before + incl - 1;
            const MatchKey k = L.keys[F.key_off + i];
            BaEdge ed;
            ed.point = e; ed.pose = 0;
            ed.u = (double)k.x; ed.v = (double)k.y; ed.ur = (double)ur[i];
            ed.info = (double)L.inv_sigma2[k.octave];
            L.edges[base + e] = ed;
            const float* X = L.kf_Xw + 3 * (size_t)(F.q_off + m);
            L.Xw[3 * (size_t)(base + e)] = (double)X[0]; L.Xw[3 * (size_t)(base + e) + 1] = (double)X[1]; L.Xw[3 * (size_t)(base + e) + 2] = (double)X[2];
            L.edge_kp[base + e] = i;
        }
        carry += tot;
    }
    if (tid == 0) L.probs[h] = PoseProblem{base, carry};
}

// After PoseOptimization number `stage`: nGood and the pose (SetPose inside PoseOptimization), mvbOutlier, the discard of the outliers after
// the first and the third one -- not after the second (:3599-3609) --, and the branch that follows: nGood < 10 leaves the frame as it is
// (:3585); 10 <= nGood < 50 goes to the (10, 100) search; after the second, 30 < nGood < 50 goes to the (3, 64) search with sFound = every
// held point (:3603-3609).  The occupancy of the search (a held point blocks its keypoint) is written here.
__global__ __launch_bounds__(256) void k_reloc_ladder_after(RelocLadder L, int stage) {
    const int h = blockIdx.x, tid = threadIdx.x;
    if (!L.active[h]) return;
    const TrackFrameDev& F = L.frames[h];
    const size_t base = (size_t)h * L.capacity;
    const int n_good = L.inliers[h], n = L.probs[h].n;
    const bool rejected = stage == 0 && n_good < 10;
    const bool discard = (stage == 0 && !rejected) || stage == 2;
    const bool search = stage == 0 ? (!rejected && n_good < 50) : stage == 1 ? (n_good > 30 && n_good < 50) : false;
    for (int i = tid; i < L.capacity; i += 256) L.outlier_of_key[base + i] = 0;
    __syncthreads();
    for (int e = tid; e < n; e += 256) {
        const int i = L.edge_kp[base + e];
        const uint8_t o = L.outlier[base + e];
        L.outlier_of_key[base + i] = o;
        if (o && discard) L.assign[base + i] = -1;
    }
    __syncthreads();
    if (search) {
        if (stage == 1) {  // sFound = every point the frame holds
            for (int q = tid; q < F.n_q; q += 256) L.found[F.q_off + q] = 0;
            __syncthreads();
        }
        for (int i = tid; i < L.capacity; i += 256) {
            const int m = L.assign[base + i];
            L.occupied[base + i] = m >= 0;
            if (stage == 1 && m >= 0) L.found[F.q_off + m] = 1;
        }
    }
    if (tid < 7) {
        const double v = L.poses[7 * h + tid];
        L.stage_poses[21 * (size_t)h + 7 * stage + tid] = v;
        L.frames[h].pose7[tid] = (float)v;
    }
    if (tid == 0) {
        int st = L.status[h] | (stage == 0 ? kRelocOpt1 : stage == 1 ? kRelocOpt2 : kRelocOpt3);
        if (rejected) st |= kRelocRejected;
        if (!search && !rejected && n_good >= 50) st |= kRelocSuccess;
        L.status[h] = st;
        L.n_good[h] = n_good;
        L.active[h] = search ? 1 : 0;
        L.frames[h].slot = search ? h : -1;
        L.frames[h].th = stage == 0 ? 10.0f : 3.0f;
        L.n_matches[h] = 0;
    }
}

}  // namespace

void launch_bow_score(const RelocPairDev* pairs, int n_pairs, const int32_t* word, const double* value, int scoring, double* out, hipStream_t st) {
    if (n_pairs > 0) TC2LI_LAUNCH(k_bow_score, dim3((n_pairs + 3) / 4), dim3(256), 0, st, pairs, n_pairs, word, value, scoring, out);
}

void launch_reloc_candidates(const RelocArgs& A, hipStream_t st) {
    if (A.n_queries <= 0) return;
    if (A.max_rows > 0) TC2LI_LAUNCH(k_reloc_rows, dim3((A.max_rows + 3) / 4, A.n_queries), dim3(256), 0, st, A);
    TC2LI_LAUNCH(k_reloc_select, dim3(A.n_queries), dim3(kSelThreads), 0, st, A);
}

void launch_reloc_ladder_init(const RelocLadder& L, hipStream_t st) {
    if (L.n_hyps > 0) TC2LI_LAUNCH(k_reloc_ladder_init, dim3(L.n_hyps), dim3(256), 0, st, L);
}
void launch_reloc_ladder_edges(const RelocLadder& L, int stage, hipStream_t st) {
    if (L.n_hyps > 0) TC2LI_LAUNCH(k_reloc_ladder_edges, dim3(L.n_hyps), dim3(256), 0, st, L, stage);
}
void launch_reloc_ladder_after(const RelocLadder& L, int stage, hipStream_t st) {
    if (L.n_hyps > 0) TC2LI_LAUNCH(k_reloc_ladder_after, dim3(L.n_hyps), dim3(256), 0, st, L, stage);
}

}  // namespace tc2li

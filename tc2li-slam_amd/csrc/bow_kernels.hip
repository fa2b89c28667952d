// The ORB vocabulary on the device (bow_host.cpp sequences it):
//   * k_bow_descend: TemplatedVocabulary::transform(feature, word_id, weight, &nid, levelsup) (SF/Thirdparty/DBoW2/DBoW2/
//     TemplatedVocabulary.h:1230-1271) -- one row of 16 lanes per descriptor, lane c takes children c, c + 16, ... of the current node,
//     the row minimum of dist * 2^16 + c is the reference's first-minimum rule (strict < in child order);
//   * k_bow_rank / k_bow_emit / k_bow_norm: the BowVector and FeatureVector of every frame (:1139-1206, BowVector.cpp:34-84,
//     FeatureVector.cpp:31-45) -- a stable rank of every feature in (node, index) and (word, index) order, one workgroup per frame, and
//     the normalisation as one ordered pass in ascending word order;
//   * k_bow_search / k_bow_count: ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (SF/src/ORBmatcher.cc:232-434) -- one wavefront per
//     (pair, common node), then the rotation histogram and ComputeThreeMaxima (:2021-2062) per pair;
//   * k_bow_search_ref / k_bow_ref_edges / k_bow_ref_finish: Tracking::TrackReferenceKeyFrame (SF/src/Tracking.cc:2603-2662) around them
//     and the pose-optimisation kernel (pose_opt_kernel.hip).
// Integer arithmetic everywhere except the word values, whose sums run in the reference's order on one lane.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "bow_device.hpp"
#include "rot_hist.hpp"

namespace tc2li {

namespace {

constexpr int kTile = 1024;  // features per LDS tile of the per-frame ranking

// the minimum of the lane's row of 16, in every lane of the row (all 16 lanes of the row must be active)
__device__ __forceinline__ unsigned row_min_u32(unsigned v) {
    v = min(v, (unsigned)dpp_take<0xB1>((int)v)); v = min(v, (unsigned)dpp_take<0x4E>((int)v));
    v = min(v, (unsigned)dpp_take<0x141>((int)v)); v = min(v, (unsigned)dpp_take<0x140>((int)v));
    return v;
}

// FORB::distance (DBoW2/FORB.cpp:81-101): popcount of the 8 XORed 32-bit words
__device__ __forceinline__ unsigned hamming(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) + __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) +
           __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

}  // namespace

// ---- the descent: 16 descriptors per workgroup, grid (descriptor blocks, frames) ----------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_descend(BowVocDev V, const uint8_t* __restrict__ desc, const BowFrameDev* __restrict__ frames,
                                                     int nid_level, BowOutDev O) {
    const BowFrameDev F = frames[blockIdx.y];
    const int i0 = blockIdx.x * 16;
    if (i0 >= F.n) return;  // the whole workgroup
    const int i = i0 + (int)(threadIdx.x >> 4), sub = threadIdx.x & 15;
    bool done = i >= F.n || V.n_words == 0;  // TemplatedVocabulary::empty(): no words, nothing is added
    uint4 q0 = make_uint4(0, 0, 0, 0), q1 = q0;
    if (!done) {
        const uint4* q = reinterpret_cast<const uint4*>(desc + 32 * (size_t)(F.src_row + i));
        q0 = q[0]; q1 = q[1];
    }
    BowNodeDev nd = V.nodes[0];
    int cur = 0, level = 0, nid = nid_level <= 0 ? 0 : -1;
    // every row stays in the loop until the wavefront's last row has reached its leaf: the DPP minimum needs the whole row active
    while (__any(!done)) {
        unsigned best = 0xffffffffu;
        if (!done) {
            for (int c = sub; c < nd.cnt; c += 16) {
                const uint4* r = V.rows + 2 * (size_t)(nd.first + c);
                const uint4 a = r[0], b = r[1];
                best = min(best, (hamming(a, b, q0, q1) << 16) | (unsigned)c);
            }
        }
        best = row_min_u32(best);
        if (!done) {
            cur = nd.first + (int)(best & 0xffffu);
            nd = V.nodes[cur];
            ++level;
            if (level == nid_level) nid = nd.ref;
            if (nd.cnt == 0) done = true;  // isLeaf() is children.empty()
        }
    }
    if (sub == 0 && i < F.n) {
        int32_t w = -1, n = -1;
        if (V.n_words > 0 && V.weight[cur] > 0) {  // not stopped
            w = nd.word;
            n = nid >= 0 ? nid : nd.ref;  // a leaf above nid_level: its own id (the reference leaves nid unset)
        }
        O.word[F.out_off + i] = w;
        O.node[F.out_off + i] = n;
    }
}

// ---- per frame: the rank of every kept feature in (node, index) order, whether it is the first of its node / word, the features
// that share its word, and the frame's counts -----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_rank(const BowFrameDev* __restrict__ frames, BowOutDev O) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const BowFrameDev F = frames[f];
    __shared__ int2 s_t[kTile];
    __shared__ int s_n[3];
    if (tid < 3) s_n[tid] = 0;
    for (int i0 = 0; i0 < F.n; i0 += 256) {
        const int i = i0 + tid;
        const int nd = i < F.n ? O.node[F.out_off + i] : -1, wd = i < F.n ? O.word[F.out_off + i] : -1;
        int rn = 0, cw = 0;
        bool first_n = true, first_w = true;
        for (int t0 = 0; t0 < F.n; t0 += kTile) {
            const int tn = min(kTile, F.n - t0);
            __syncthreads();
            for (int j = tid; j < tn; j += 256) s_t[j] = make_int2(O.node[F.out_off + t0 + j], O.word[F.out_off + t0 + j]);
            __syncthreads();
            if (wd >= 0) {
                for (int j = 0; j < tn; ++j) {
                    const int2 e = s_t[j];
                    if (e.y < 0) continue;
                    const bool before = t0 + j < i;
                    rn += (e.x < nd || (e.x == nd && before)) ? 1 : 0;
                    cw += e.y == wd ? 1 : 0;
                    if (before) { first_n = first_n && e.x != nd; first_w = first_w && e.y != wd; }
                }
            }
        }
        if (wd >= 0) {
            O.rank[F.out_off + i] = (uint32_t)rn;
            O.flags[F.out_off + i] = (first_n ? 1 : 0) | (first_w ? 2 : 0) | (cw << 2);
            atomicAdd(&s_n[0], 1);
            if (first_n) atomicAdd(&s_n[1], 1);
            if (first_w) atomicAdd(&s_n[2], 1);
        }
    }
    __syncthreads();
    if (tid == 0) { O.n_valid[f] = s_n[0]; O.n_nodes[f] = s_n[1]; O.n_words[f] = s_n[2]; }
}

// ---- per frame: the FeatureVector (node ids ascending, feature indices in feature order per node) and the BowVector entries before
// normalisation -- TF / TF_IDF: BowVector::addWeight adds the weight once per feature, IDF / BINARY: addIfNotExist keeps the first --
__global__ __launch_bounds__(256) void k_bow_emit(const BowFrameDev* __restrict__ frames, int weighting, const double* __restrict__ word_weight,
                                                  BowOutDev O) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const BowFrameDev F = frames[f];
    __shared__ int4 s_t[kTile];
    const int base = F.out_off;
    for (int i0 = 0; i0 < F.n; i0 += 256) {
        const int i = i0 + tid;
        const int nd = i < F.n ? O.node[base + i] : -1, wd = i < F.n ? O.word[base + i] : -1;
        int slot_n = 0, slot_w = 0;
        for (int t0 = 0; t0 < F.n; t0 += kTile) {
            const int tn = min(kTile, F.n - t0);
            __syncthreads();
            for (int j = tid; j < tn; j += 256) {
                const int w = O.word[base + t0 + j];
                s_t[j] = make_int4(O.node[base + t0 + j], w, w >= 0 ? O.flags[base + t0 + j] : 0, 0);
            }
            __syncthreads();
            if (wd >= 0) {
                for (int j = 0; j < tn; ++j) {
                    const int4 e = s_t[j];
                    slot_n += ((e.z & 1) && e.x < nd) ? 1 : 0;
                    slot_w += ((e.z & 2) && e.y < wd) ? 1 : 0;
                }
            }
        }
        if (wd >= 0) {
            const int rank = (int)O.rank[base + i], fl = O.flags[base + i];
            O.fv_index[base + rank] = i;
            if (fl & 1) { O.fv_node[base + slot_n] = nd; O.fv_offset[base + f + slot_n] = rank; }
            if (fl & 2) {
                const double w = word_weight[wd];
                double v = w;
                if (weighting == 0 || weighting == 1)
                    for (int c = 1; c < (fl >> 2); ++c) v += w;
                O.bow_word[base + slot_w] = wd;
                O.bow_value[base + slot_w] = v;
            }
        }
    }
    if (tid == 0) O.fv_offset[base + f + O.n_nodes[f]] = O.n_valid[f];
}

// ---- per frame: BowVector::normalize (BowVector.cpp:62-84) with the scoring's norm (ScoringObject.h:74-89), or DOT_PRODUCT's
// division by the number of words under TF / TF_IDF (TemplatedVocabulary.h:1176-1182); the norm is one pass in ascending word order ----
__global__ __launch_bounds__(64) void k_bow_norm(const BowFrameDev* __restrict__ frames, int scoring, int weighting, BowOutDev O) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const int base = frames[f].out_off, nw = O.n_words[f];
    double* v = O.bow_value + base;
    if (scoring == 5) {  // DOT_PRODUCT: mustNormalize() is false
        if ((weighting == 0 || weighting == 1) && nw > 0) {
            const double nd = (double)nw;
            for (int p = tid; p < nw; p += 64) v[p] /= nd;
        }
        return;
    }
    __shared__ double s_v[kTile];
    __shared__ double s_norm;
    double norm = 0.0;
    for (int p0 = 0; p0 < nw; p0 += kTile) {
        const int pn = min(kTile, nw - p0);
        __syncthreads();
        for (int p = tid; p < pn; p += 64) s_v[p] = v[p0 + p];
        __syncthreads();
        if (tid == 0) {
            if (scoring == 1) for (int p = 0; p < pn; ++p) norm += s_v[p] * s_v[p];   // L2
            else for (int p = 0; p < pn; ++p) norm += fabs(s_v[p]);                   // L1
        }
    }
    if (tid == 0) s_norm = scoring == 1 ? sqrt(norm) : norm;
    __syncthreads();
    norm = s_norm;
    if (norm > 0.0)
        for (int p = tid; p < nw; p += 64) v[p] /= norm;
}

// ---- SearchByBoW, one common node on one wavefront.  The keyframe's features of the node in order; the frame's across the lanes
// (position j at lane j % 64, bit j / 64 of its taken mask).  best = wave minimum of dist * 2^16 + j (the first index that reaches the
// minimum); second = the minimum over everything else, ties included -- what the strict-< update of bestDist1 / bestDist2 leaves.
// kf_rows / kf_hp are indexed by keyframe feature, f_rows by frame feature, match (the pair's row) by frame feature ----------------
__device__ __forceinline__ void bow_match_node(const uint4* __restrict__ kf_rows, const uint8_t* __restrict__ kf_hp, const int32_t* __restrict__ kf_idx,
                                               int kf_n, const uint4* __restrict__ f_rows, const int32_t* __restrict__ f_idx, int f_n, float nn_ratio,
                                               int32_t* __restrict__ match) {
    const int lane = threadIdx.x & 63;
    uint64_t taken = 0;
    for (int a = 0; a < kf_n; ++a) {
        const int kfi = kf_idx[a];
        if (!kf_hp[kfi]) continue;  // !pMP || pMP->isBad()
        const uint4 q0 = kf_rows[2 * (size_t)kfi], q1 = kf_rows[2 * (size_t)kfi + 1];
        unsigned best = 0xffffffffu, second = 256;
        for (int c = 0; c * 64 < f_n; ++c) {
            const int j = c * 64 + lane;
            if (j < f_n && !((taken >> c) & 1)) {
                const int fi = f_idx[j];
                const uint4 b0 = f_rows[2 * (size_t)fi], b1 = f_rows[2 * (size_t)fi + 1];
                const unsigned dist = hamming(q0, q1, b0, b1), key = (dist << 16) | (unsigned)j;
                if (key < best) { second = min(second, best >> 16); best = key; }
                else second = min(second, dist);
            }
        }
        const unsigned wbest = wave_min_u32(best);
        const unsigned wsecond = wave_min_u32(best == wbest ? second : min(best >> 16, 256u));
        const unsigned d1 = wbest >> 16;
        if (d1 <= 50 && (float)d1 < nn_ratio * (float)wsecond) {  // TH_LOW; mfNNratio
            const int j = (int)(wbest & 0xffffu);
            if (lane == (j & 63)) taken |= 1ull << (j >> 6);
            if (lane == 0) match[f_idx[j]] = kfi;
        }
    }
}

// tc2li_search_by_bow_batch: the common nodes were found on the host; everything is in the staged arrays
__global__ __launch_bounds__(256) void k_bow_search(const BowTaskDev* __restrict__ tasks, int n_tasks, const BowPairDev* __restrict__ pairs,
                                                    const uint8_t* __restrict__ desc, const uint8_t* __restrict__ has_point,
                                                    const int32_t* __restrict__ fv_index, int32_t* __restrict__ match) {
    const int t = blockIdx.x * 4 + wave_in_block();
    if (t >= n_tasks) return;  // the whole wavefront
    const BowTaskDev T = tasks[t];
    const BowPairDev P = pairs[T.pair];
    const uint4* rows = reinterpret_cast<const uint4*>(desc);
    bow_match_node(rows + 2 * (size_t)P.kf_key, has_point + P.kf_key, fv_index + T.kf_pos, T.kf_n, rows + 2 * (size_t)P.f_key,
                   fv_index + T.f_pos, T.f_n, P.nn_ratio, match + P.out_off);
}

// tc2li_track_reference_keyframe_batch: one task per node of the reference keyframe (pair = frame); the frame's FeatureVector is the
// transform's output on the device, the node is looked up there (binary search, ascending node ids).  Frame features beyond 4096 in one
// node are refused by the host before the call (at most capacity features per frame, capacity <= 4096).
__global__ __launch_bounds__(256) void k_bow_search_ref(const BowTaskDev* __restrict__ tasks, int n_tasks, const BowPairDev* __restrict__ pairs,
                                                        const uint8_t* __restrict__ kf_desc, const uint8_t* __restrict__ kf_has_point,
                                                        const int32_t* __restrict__ kf_fv_index, const int32_t* __restrict__ kf_node,
                                                        const uint8_t* __restrict__ f_desc, BowOutDev O, int32_t* __restrict__ match) {
    const int t = blockIdx.x * 4 + wave_in_block();
    if (t >= n_tasks) return;  // the whole wavefront
    const BowTaskDev T = tasks[t];
    const BowPairDev P = pairs[T.pair];
    const int base = P.out_off, node = kf_node[t];
    int lo = 0, hi = O.n_nodes[T.pair];  // first slot with fv_node >= node
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (O.fv_node[base + mid] < node) lo = mid + 1; else hi = mid;
    }
    if (lo >= O.n_nodes[T.pair] || O.fv_node[base + lo] != node) return;
    const int f0 = O.fv_offset[base + T.pair + lo], f1 = O.fv_offset[base + T.pair + lo + 1];
    const uint4* krows = reinterpret_cast<const uint4*>(kf_desc);
    const uint4* frows = reinterpret_cast<const uint4*>(f_desc);
    bow_match_node(krows + 2 * (size_t)P.kf_key, kf_has_point + P.kf_key, kf_fv_index + T.kf_pos, T.kf_n, frows + 2 * (size_t)P.f_key,
                   O.fv_index + base + f0, f1 - f0, P.nn_ratio, match + base);
}

// ---- per pair: nmatches and, with check_orientation, the rotation histogram and ComputeThreeMaxima (ORBmatcher.cc:347-361, 413-431;
// rot_hist.hpp).  kf_angle is indexed from P.kf_key, f_angle from P.f_key ------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_count(const BowPairDev* __restrict__ pairs, const float* __restrict__ kf_angle, const float* __restrict__ f_angle,
                                                   int32_t* __restrict__ match, int32_t* __restrict__ n_matches) {
    const int p = blockIdx.x, tid = threadIdx.x;
    const BowPairDev P = pairs[p];
    __shared__ int s_count[kRotHistLength];
    __shared__ int s_ind[3];
    __shared__ int s_nm;
    if (tid < kRotHistLength) s_count[tid] = 0;
    if (tid == 0) s_nm = 0;
    __syncthreads();
    int nm = 0;
    for (int i = tid; i < P.f_n; i += 256) {
        const int m = match[P.out_off + i];
        if (m < 0) continue;
        ++nm;
        if (P.check_orientation) atomicAdd(&s_count[rot_hist_bin(kf_angle[P.kf_key + m], f_angle[P.f_key + i])], 1);
    }
    atomicAdd(&s_nm, nm);
    __syncthreads();
    if (!P.check_orientation) { if (tid == 0) n_matches[p] = s_nm; return; }
    if (tid == 0) rot_hist_three_maxima(s_count, s_ind);
    __syncthreads();
    int removed = 0;
    for (int i = tid; i < P.f_n; i += 256) {
        const int m = match[P.out_off + i];
        if (m < 0) continue;
        const int bin = rot_hist_bin(kf_angle[P.kf_key + m], f_angle[P.f_key + i]);
        if (bin != s_ind[0] && bin != s_ind[1] && bin != s_ind[2]) { match[P.out_off + i] = -1; ++removed; }
    }
    atomicSub(&s_nm, removed);
    __syncthreads();
    if (tid == 0) n_matches[p] = s_nm;
}

// ---- TrackReferenceKeyFrame (SF/src/Tracking.cc:2603-2662): with at least 15 matches the edge list of Optimizer::PoseOptimization over
// every keypoint that now holds a point, in keypoint order (stereo when uRight >= 0, invSigma2[octave]), at the last frame's pose; with
// fewer, no edges.  One workgroup per frame ----------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bow_ref_edges(const BowPairDev* __restrict__ pairs, const BowRefConst C, const MatchKey* __restrict__ keys,
                                                       const float* __restrict__ u_right, const int32_t* __restrict__ match,
                                                       const int32_t* __restrict__ n_matches, const float* __restrict__ kf_Xw,
                                                       const float* __restrict__ last_pose7, PoseProblem* __restrict__ probs,
                                                       BaEdge* __restrict__ edges, double* __restrict__ Xw, int32_t* __restrict__ edge_kp,
                                                       double* __restrict__ poses) {
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = wave_in_block();
    const BowPairDev P = pairs[f];
    const int base = P.out_off;
    __shared__ int s_wave[4];
    if (tid < 7) poses[7 * f + tid] = (double)last_pose7[7 * f + tid];  // SetPose(mLastFrame.GetPose())
    if (n_matches[f] < 15) { if (tid == 0) probs[f] = PoseProblem{base, 0}; return; }
    int carry = 0;
    for (int i0 = 0; i0 < P.f_n; i0 += 256) {
        const int i = i0 + tid;
        const int m = i < P.f_n ? match[base + i] : -1;
        // exclusive scan of the edge flags over the workgroup
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
            const MatchKey k = keys[P.f_key + i];
            BaEdge ed;
            ed.point = e; ed.pose = 0;
            ed.u = (double)k.x; ed.v = (double)k.y; ed.ur = (double)u_right[base + i];
            ed.info = (double)C.inv_sigma2[k.octave];
            edges[base + e] = ed;
            const float* X = kf_Xw + 3 * (size_t)(P.kf_key + m);
            Xw[3 * (size_t)(base + e)] = (double)X[0]; Xw[3 * (size_t)(base + e) + 1] = (double)X[1]; Xw[3 * (size_t)(base + e) + 2] = (double)X[2];
            edge_kp[base + e] = i;
        }
        carry += tot;
    }
    if (tid == 0) probs[f] = PoseProblem{base, carry};
}

// Tracking.cc:2640-2656: outliers lose their point (nmatches--), nmatchesMap counts the inliers whose point has observations; a frame with
// fewer than 15 matches fails: the last pose, every match -1, n_inliers -1
__global__ __launch_bounds__(256) void k_bow_ref_finish(const BowPairDev* __restrict__ pairs, const int32_t* __restrict__ n_matches,
                                                        const PoseProblem* __restrict__ probs, const uint8_t* __restrict__ outlier,
                                                        const int32_t* __restrict__ edge_kp, const int32_t* __restrict__ inliers,
                                                        const uint8_t* __restrict__ kf_observed, int32_t* __restrict__ match,
                                                        int32_t* __restrict__ n_inliers, int32_t* __restrict__ n_matches_map) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const BowPairDev P = pairs[f];
    const int base = P.out_off;
    if (n_matches[f] < 15) {
        for (int i = tid; i < P.f_n; i += 256) match[base + i] = -1;
        if (tid == 0) { n_inliers[f] = -1; n_matches_map[f] = 0; }
        return;
    }
    __shared__ int s_map;
    if (tid == 0) s_map = 0;
    __syncthreads();
    const int n = probs[f].n;
    int nm = 0;
    for (int e = tid; e < n; e += 256) {
        const int i = edge_kp[base + e];
        if (outlier[base + e]) match[base + i] = -1;
        else if (kf_observed[P.kf_key + match[base + i]]) ++nm;
    }
    atomicAdd(&s_map, nm);
    __syncthreads();
    if (tid == 0) { n_inliers[f] = inliers[f]; n_matches_map[f] = s_map; }
}

void launch_bow_descend(const BowVocDev& V, const uint8_t* desc, const BowFrameDev* frames, int n_frames, int max_n, int nid_level,
                        const BowOutDev& O, hipStream_t st) {
    if (n_frames <= 0 || max_n <= 0) return;
    TC2LI_LAUNCH(k_bow_descend, dim3((max_n + 15) / 16, n_frames), dim3(256), 0, st, V, desc, frames, nid_level, O);
}

void launch_bow_assemble(const BowVocDev&, const double* word_weight, const BowFrameDev* frames, int n_frames, int scoring, int weighting,
                         const BowOutDev& O, hipStream_t st) {
    if (n_frames <= 0) return;
    TC2LI_LAUNCH(k_bow_rank, dim3(n_frames), dim3(256), 0, st, frames, O);
    TC2LI_LAUNCH(k_bow_emit, dim3(n_frames), dim3(256), 0, st, frames, weighting, word_weight, O);
    TC2LI_LAUNCH(k_bow_norm, dim3(n_frames), dim3(64), 0, st, frames, scoring, weighting, O);
}

void launch_bow_search(const BowTaskDev* tasks, int n_tasks, const BowPairDev* pairs, int n_pairs, const uint8_t* desc, const float* angle,
                       const uint8_t* has_point, const int32_t* fv_index, int32_t* match, int32_t* n_matches, hipStream_t st) {
    if (n_tasks > 0) TC2LI_LAUNCH(k_bow_search, dim3((n_tasks + 3) / 4), dim3(256), 0, st, tasks, n_tasks, pairs, desc, has_point, fv_index, match);
    if (n_pairs > 0) TC2LI_LAUNCH(k_bow_count, dim3(n_pairs), dim3(256), 0, st, pairs, angle, angle, match, n_matches);
}

void launch_bow_reference(const BowRefArgs& A, hipStream_t st) {
    if (A.n_frames <= 0) return;
    if (A.n_tasks > 0)
        TC2LI_LAUNCH(k_bow_search_ref, dim3((A.n_tasks + 3) / 4), dim3(256), 0, st, A.tasks, A.n_tasks, A.pairs, A.kf_desc, A.kf_has_point,
                     A.kf_fv_index, A.kf_node, A.f_desc, A.O, A.match);
    TC2LI_LAUNCH(k_bow_count, dim3(A.n_frames), dim3(256), 0, st, A.pairs, A.kf_angle, A.f_angle, A.match, A.n_matches);
    TC2LI_LAUNCH(k_bow_ref_edges, dim3(A.n_frames), dim3(256), 0, st, A.pairs, A.C, A.keys, A.u_right, A.match, A.n_matches, A.kf_Xw, A.last_pose7,
                 A.probs, A.edges, A.Xw, A.edge_kp, A.poses);
}

void launch_bow_reference_finish(const BowRefArgs& A, hipStream_t st) {
    if (A.n_frames <= 0) return;
    TC2LI_LAUNCH(k_bow_ref_finish, dim3(A.n_frames), dim3(256), 0, st, A.pairs, A.n_matches, A.probs, A.outlier, A.edge_kp, A.inliers, A.kf_observed,
                 A.match, A.n_inliers, A.n_matches_map);
}

}  // namespace tc2li

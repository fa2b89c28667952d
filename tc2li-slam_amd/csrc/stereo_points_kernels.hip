// Stereo map points and the keyframe decision of tracking on gfx950 (SF/src/Tracking.cc:2942-3076 NeedNewKeyFrame, :3078-3212
// CreateNewKeyFrame, :2676-2734 UpdateLastFrame, :2477-2495 StereoInitialization).  One workgroup of four wavefronts per frame, one launch:
//   counts     every wavefront owns a contiguous run of the frame's keypoints and counts those with depth, those the walk treats as close
//              (depth <= th_depth), NeedNewKeyFrame's tracked / non-tracked close ones and the reference keyframe's tracked points; the
//              lane sums go through wave_sum_i32 (launch.hpp) and 20 ints of LDS.  Bytes per keypoint: 4 (depth) + 1 + 1 (held, outlier).
//   decision   newkf::decide (stereo_points_device.hpp), evaluated by every lane on the same scalars: the workgroup stays or leaves as one.
//   keys       depth bits << 32 | index for the keypoints with depth, compacted into the LDS by a 64-lane ballot and prefix popcount.  A
//              positive float orders as its bit pattern (+inf included), so ascending keys are std::sort's order on pair<float, int>.
//              The wavefronts' runs are contiguous, so the compaction keeps index order: mode ALL is done here.
//   sort       bitonic network over the next power of two (at most 4096 keys = 32 KB), padded with all-ones keys; log2(P) (log2(P) + 1) / 2
//              stages, a barrier after each.  A lane handles the pair (i, i | j) with i = its number with a 0 inserted at bit log2(j): from
//              j = 32 up the lanes of a 32-lane group read and write consecutive 8-byte words (conflict-free, the bank rule of 8-byte
//              LDS reads); the five stages with j < 32 of every merge touch two 8-byte words per 16 bytes and pay a 2-way conflict.  At
//              most 78 stages of 8 pairs per lane: tens of microseconds per frame against the milliseconds of the batch's transfers, so
//              the network is left plain.
//   walk       entries taken = min(M, max(c, max_point) + 1) -- the closed form of the reference's exit test (include/tc2li_hip.h); every
//              wavefront owns a contiguous run of the sorted entries, marks the created ones (held != 1) in bit 63 of their keys (free: the
//              depth is positive), the runs' counts are exchanged through the LDS, and the created entries are un-projected and written in
//              sorted order at ballot / prefix-popcount positions.  A created point costs 8 B (x, y) in and 16 B out.
// A frame without keypoints, without a positive depth or with a "no" passes every barrier with the whole workgroup: all branches around
// barriers test values that are the same in every lane.
#include "launch.hpp"
#include "stereo_points_device.hpp"

namespace tc2li {

constexpr int kSpThreads = 256;
constexpr int kSpWaves = kSpThreads / 64;

__global__ __launch_bounds__(kSpThreads) void k_stereo_points(StereoPointsBatch B) {
    __shared__ unsigned long long keys[kStereoPointsMaxKeys];
    __shared__ int red[kSpWaves * 5];
    __shared__ int wave_created[kSpWaves];
    const int tid = threadIdx.x, lane = tid & 63, w = wave_in_block();
    const unsigned long long below = (1ull << lane) - 1ull;                          // the lanes before this one
    const StereoFrameDev& F = B.frames[blockIdx.x];
    const int n = min(F.n, kStereoPointsMaxKeys);                                    // the host refuses more
    const float th_depth = F.th_depth;
    const float* depth = B.depth + F.off;
    const uint8_t* held = B.held + F.off;
    // ---- counts ----
    const int run = (n + kSpThreads - 1) / kSpThreads * 64;
    const int i0 = min(n, w * run), i1 = min(n, i0 + run);
    int n_depth = 0, n_near = 0, n_tracked = 0, n_non_tracked = 0, n_ref = 0;
    for (int i = i0 + lane; i < i1; i += 64) {
        const float z = depth[i];
        if (newkf::has_depth(z)) { ++n_depth; n_near += !(z > th_depth); }
        if (B.decide && newkf::close_for_counts(z, th_depth)) {                      // :2990-2996
            if (held[i] != 0 && !B.outlier[F.off + i]) ++n_tracked;
            else ++n_non_tracked;
        }
    }
    if (B.decide && F.n_ref > 0) {
        const int n_kfs = B.decisions[blockIdx.x].n_kfs;
        const int32_t* nobs = B.ref_nobs + F.ref_off;
        for (int i = tid; i < F.n_ref; i += kSpThreads) n_ref += newkf::ref_match(nobs[i], n_kfs);
    }
    n_depth = wave_sum_i32(n_depth); n_near = wave_sum_i32(n_near); n_tracked = wave_sum_i32(n_tracked);
    n_non_tracked = wave_sum_i32(n_non_tracked); n_ref = wave_sum_i32(n_ref);
    if (lane == 0) { red[5 * w] = n_depth; red[5 * w + 1] = n_near; red[5 * w + 2] = n_tracked; red[5 * w + 3] = n_non_tracked; red[5 * w + 4] = n_ref; }
    __syncthreads();
    int M = 0, c = 0, tracked = 0, non_tracked = 0, ref = 0, before = 0;             // before: keys of the wavefronts in front of this one
    for (int v = 0; v < kSpWaves; ++v) {
        if (v < w) before += red[5 * v];
        M += red[5 * v]; c += red[5 * v + 1]; tracked += red[5 * v + 2]; non_tracked += red[5 * v + 3]; ref += red[5 * v + 4];
    }
    // ---- decision ----
    bool create = true;
    if (B.decide) {
        const KeyframeDecisionDev& D = B.decisions[blockIdx.x];
        tc2li_keyframe_verdict v;
        v.n_ref_matches = F.n_ref >= 0 ? ref : D.n_ref_matches;
        newkf::decide(D, tracked, non_tracked, v.n_ref_matches, &v);
        v.n_tracked_close = tracked; v.n_non_tracked_close = non_tracked; v.pad_ = 0;
        if (tid == 0) B.verdicts[blockIdx.x] = v;
        create = v.need && !(D.flags & newkf::kCreateBlocked);
    }
    const bool all = !B.decide && F.mode == TC2LI_STEREO_POINTS_ALL;
    if (all && n <= 500) create = false;                                             // :2433
    int taken = 0, n_created = 0;
    if (create && M > 0) {
        // ---- keys ----
        int at = before;
        for (int s = i0; s < i1; s += 64) {
            const int i = s + lane;
            const float z = i < i1 ? depth[i] : 0.0f;
            const bool has = newkf::has_depth(z);
            const unsigned long long m = __ballot(has);
            if (has) keys[at + __popcll(m & below)] = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
            at += __popcll(m);
        }
        taken = M;
        if (!all) {
            // ---- sort ----
            int P = 1;
            while (P < M) P <<= 1;
            for (int i = M + tid; i < P; i += kSpThreads) keys[i] = ~0ull;
            __syncthreads();
            for (int k = 2; k <= P; k <<= 1)
                for (int j = k >> 1; j > 0; j >>= 1) {
                    for (int t = tid; t < (P >> 1); t += kSpThreads) {
                        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
                        const unsigned long long a = keys[i], b = keys[l];
                        if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
                    }
                    __syncthreads();
                }
            const int stop = max(c, F.max_point);                                    // :3199, :2731 in closed form
            if (stop < M) taken = stop + 1;
        } else {
            __syncthreads();
        }
        // ---- walk ----
        const int run2 = (taken + kSpThreads - 1) / kSpThreads * 64;
        const int j0 = min(taken, w * run2), j1 = min(taken, j0 + run2);
        int mine = 0;
        for (int s = j0; s < j1; s += 64) {
            const int j = s + lane;
            bool make = false;
            if (j < j1) {
                const unsigned long long key = keys[j];
                make = all || held[(unsigned)key] != 1;                              // :3156-3162, :2704-2707
                if (make) keys[j] = key | (1ull << 63);
            }
            mine += __popcll(__ballot(make));
        }
        if (lane == 0) wave_created[w] = mine;
        __syncthreads();
        int out = 0;
        for (int v = 0; v < kSpWaves; ++v) {
            if (v < w) out += wave_created[v];
            n_created += wave_created[v];
        }
        const float* xy = B.xy + 2 * (size_t)F.off;
        for (int s = j0; s < j1; s += 64) {
            const int j = s + lane;
            const unsigned long long key = j < j1 ? keys[j] : 0ull;
            const bool make = key >> 63;
            const unsigned long long m = __ballot(make);
            if (make) {
                const int i = (int)(unsigned)key;
                const size_t o = (size_t)F.off + out + __popcll(m & below);
                float X[3];
                newkf::unproject(xy[2 * i], xy[2 * i + 1], __uint_as_float((unsigned)(key >> 32) & 0x7fffffffu), B.cx, B.cy, B.invfx, B.invfy,
                                 F.Rwc, F.Ow, X);
                B.created_keypoint[o] = i;
                B.x3D[3 * o] = X[0]; B.x3D[3 * o + 1] = X[1]; B.x3D[3 * o + 2] = X[2];
            }
            out += __popcll(m);
        }
    }
    if (tid == 0) {
        int32_t* counts = B.counts + 3 * (size_t)blockIdx.x;
        counts[0] = n_created; counts[1] = taken; counts[2] = M;
    }
}

void launch_stereo_points(const StereoPointsBatch& B, hipStream_t st) {
    if (B.n_frames > 0) TC2LI_LAUNCH(k_stereo_points, dim3(B.n_frames), dim3(kSpThreads), 0, st, B);
}

}  // namespace tc2li

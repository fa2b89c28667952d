// KeyFrameCulling / MapPointCulling of local mapping on gfx950 (SF/src/LocalMapping.cc:913-1065, :360-399).  Integer work over the flat
// graph: no f64, no MFMA, no float atomics; the bound is the gathers over the points' observation rows.
//   k_cull_count    one workgroup per (problem, local keyframe): nMPs / nRedundant of :959-1019 on the INITIAL state.  Lanes run over the
//                   keyframe's slots, each lane walks its point's observation row.  Algorithmic bytes per problem: the sum over the
//                   local keyframes of slots x (4 + 4 + 1 B: point, depth, octave) plus, for the slots that pass the gates of :966-977,
//                   1 + 4 B of the point (bad, nObs) and its observation row x (4 + 1 B: keyframe, octave; + 1 B alive in a recount).
//   k_cull_resolve  one workgroup per problem walks `local` in order.  A keyframe none of whose points lost an observation to an earlier
//                   cull of this call takes the counts of k_cull_count; any other ("dirty") is recounted on the current state by the
//                   whole workgroup.  SetBadFlag's erasure (KeyFrame.cc:605-611, MapPoint.cc:177-210) runs over the slots in parallel:
//                   one lane per point takes the keyframe's observation out of the row, lowers nObs, marks the point changed and, at
//                   nObs <= 2, bad (a bad point is never walked again, so its row is left as it is).  The gates of :1023-1054 and the
//                   link edits are evaluated uniformly / written by one lane.  Everything a later iteration reads was written before a
//                   workgroup barrier of an earlier one.
//   k_mp_cull       one lane per entry of mlpRecentAddedMapPoints.
// The wavefront's number is taken as a scalar (wave_in_block) where the reduction's LDS address derives from it; problem and keyframe
// come from blockIdx.
#include "culling_device.hpp"
#include "launch.hpp"

namespace tc2li {

constexpr int kCullThreads = 256;

// nMPs and nRedundantObservations of keyframe kf (:959-1019) by the whole workgroup, the sums in every lane.  kInitial: no observation has
// been erased yet, the alive bytes are not read.  red: 8 ints of LDS.
template <bool kInitial>
__device__ __forceinline__ void count_keyframe(const CullBatch& B, const CullProblemDev& P, int kf, int* red, int* n_mps_out, int* n_red_out) {
    const int32_t* row = B.slot_offsets + P.slot_row_off;
    const int s0 = row[kf], s1 = row[kf + 1];
    const float th_depth = B.kf_th_depth[P.kf_off + kf];
    const int32_t* slot_point = B.slot_point + P.slot_off;
    const float* slot_depth = B.slot_depth + P.slot_off;
    const int8_t* slot_octave = B.slot_octave + P.slot_off;
    const int32_t* obs_row = B.obs_offsets + P.obs_row_off;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int8_t* obs_octave = B.obs_octave + P.obs_off;
    const uint8_t* obs_dead = B.obs_dead + P.obs_off;
    int n_mps = 0, n_red = 0;
    for (int s = s0 + (int)threadIdx.x; s < s1; s += kCullThreads) {
        const int p = slot_point[s];
        if (p < 0 || B.point_bad[P.point_off + p]) continue;                         // :966-968
        const float depth = slot_depth[s];
        if (depth > th_depth || depth < 0.0f) continue;                              // :972
        ++n_mps;                                                                     // :976
        if (B.point_nobs[P.point_off + p] > cull::kThObs) {                          // :977
            const int level = (int)slot_octave[s] + 1;
            const int o1 = obs_row[p + 1];
            int n = 0;
            for (int o = obs_row[p]; o < o1; ++o) {                                  // :984-1011
                const bool alive = kInitial || !obs_dead[o];
                if (alive && obs_kf[o] != kf && (int)obs_octave[o] <= level && ++n > cull::kThObs) break;
            }
            n_red += n > cull::kThObs;                                               // :1012-1015
        }
    }
    n_mps = wave_sum_i32(n_mps);
    n_red = wave_sum_i32(n_red);
    const int w = wave_in_block();
    if ((threadIdx.x & 63) == 0) { red[2 * w] = n_mps; red[2 * w + 1] = n_red; }
    __syncthreads();
    *n_mps_out = red[0] + red[2] + red[4] + red[6];
    *n_red_out = red[1] + red[3] + red[5] + red[7];
    __syncthreads();
}

__global__ __launch_bounds__(kCullThreads) void k_cull_count(CullBatch B) {
    __shared__ int red[8];
    const int e = blockIdx.x;
    const CullProblemDev& P = B.problems[B.problem_of_local[e]];
    const int kf = B.local[e];
    int n_mps, n_red;
    count_keyframe<true>(B, P, kf, red, &n_mps, &n_red);
    if (threadIdx.x == 0) { B.spec[2 * e] = n_mps; B.spec[2 * e + 1] = n_red; }
}

__global__ __launch_bounds__(kCullThreads) void k_cull_resolve(CullBatch B) {
    __shared__ int red[8];
    const int tid = threadIdx.x;
    const CullProblemDev& P = B.problems[blockIdx.x];
    const bool inertial = P.flags & 1, imu_initialized = P.flags & 2, inertial_ba2 = P.flags & 4, abort_ba = P.flags & 8;
    const int32_t* slot_row = B.slot_offsets + P.slot_row_off;
    const int32_t* slot_point = B.slot_point + P.slot_off;
    int keyframes_in_map = P.keyframes_in_map;
    bool any_erased = false;
    int count = 0;
    while (count < P.n_local) {
        const int i = count++;                                                       // :952
        const int e = P.local_off + i;
        const int kf = B.local[e];
        const int g = P.kf_off + kf;
        if ((B.kf_flags[g] & 3) || B.kf_bad[g]) {                                    // :955
            if (tid == 0) B.verdict[e] = TC2LI_CULL_SKIPPED;
            continue;
        }
        const int s0 = slot_row[kf], s1 = slot_row[kf + 1];
        int dirty = 0;
        if (any_erased) {
            for (int s = s0 + tid; s < s1; s += kCullThreads) {
                const int p = slot_point[s];
                if (p >= 0 && B.point_changed[P.point_off + p]) dirty = 1;
            }
            dirty = __syncthreads_or(dirty);
        }
        int n_mps, n_red;
        if (dirty) count_keyframe<false>(B, P, kf, red, &n_mps, &n_red);
        else { n_mps = B.spec[2 * e]; n_red = B.spec[2 * e + 1]; }
        int verdict = 0;
        bool go_on = false;
        int prev = -1, next = -1;
        if (cull::redundant(n_red, n_mps, inertial)) {                               // :1021
            verdict = TC2LI_CULL_REDUNDANT;
            if (inertial) {
                prev = B.kf_prev[g]; next = B.kf_next[g];
                const bool has_links = prev >= 0 && next >= 0;
                const cull::Gate gate = cull::inertial_gate(keyframes_in_map, B.kf_id[g], P.current_id, P.last_id, has_links,
                                                            has_links ? B.kf_time[P.kf_off + prev] : 0.0, has_links ? B.kf_time[P.kf_off + next] : 0.0,
                                                            B.kf_imu_pos + 3 * (size_t)g, B.kf_imu_pos + 3 * (size_t)(P.kf_off + (has_links ? prev : kf)),
                                                            imu_initialized, inertial_ba2);
                go_on = gate == cull::kGateContinue;
                if (gate == cull::kGateMerge) verdict |= TC2LI_CULL_MERGED | TC2LI_CULL_SET_BAD;
            } else {
                verdict |= TC2LI_CULL_SET_BAD;                                       // :1057
            }
        }
        const bool erase = (verdict & TC2LI_CULL_SET_BAD) && !(B.kf_flags[g] & 4);
        if ((verdict & TC2LI_CULL_SET_BAD) && !erase) verdict |= TC2LI_CULL_DEFERRED;   // KeyFrame.cc:593-597
        if (tid == 0) { B.verdict[e] = verdict; B.n_mps[e] = n_mps; B.n_redundant[e] = n_red; }
        if (verdict & TC2LI_CULL_SET_BAD) {
            // every lane has decided on the same state: only now may it change (a lane that read a link or a flag after the change
            // would part from the others at the next barrier)
            __syncthreads();
            if ((verdict & TC2LI_CULL_MERGED) && tid == 0) {                         // :1038-1041
                B.kf_prev[P.kf_off + next] = prev;
                B.kf_next[P.kf_off + prev] = next;
                B.kf_next[g] = -1;
                B.kf_prev[g] = -1;
            }
            if (erase) {                                                             // KeyFrame.cc:605-611
                const int32_t* obs_row = B.obs_offsets + P.obs_row_off;
                const int32_t* obs_kf = B.obs_kf + P.obs_off;
                const uint8_t* obs_weight = B.obs_weight + P.obs_off;
                uint8_t* obs_dead = B.obs_dead + P.obs_off;
                const int stamp = count;   // one per pass, never 0
                for (int s = s0 + tid; s < s1; s += kCullThreads) {
                    const int p = slot_point[s];
                    if (p < 0) continue;
                    const int gp = P.point_off + p;
                    if (B.point_bad[gp]) continue;                                   // no observations left (MapPoint.cc:233)
                    if (atomicExch(&B.point_claim[gp], stamp) == stamp) continue;    // another slot of this keyframe holds the point too
                    const int o1 = obs_row[p + 1];
                    int w = 0;
                    bool held = false;
                    for (int o = obs_row[p]; o < o1; ++o)
                        if (obs_kf[o] == kf && !obs_dead[o]) { obs_dead[o] = 1; w += obs_weight[o]; held = true; }
                    if (!held) continue;                                             // MapPoint.cc:182
                    const int n = B.point_nobs[gp] - w;                              // :187-192
                    B.point_nobs[gp] = n;
                    B.point_changed[gp] = 1;
                    if (n <= 2) B.point_bad[gp] = 1;                                 // :203-209
                }
                if (tid == 0) B.kf_bad[g] = 1;
                --keyframes_in_map;                                                  // Map::EraseKeyFrame
                any_erased = true;
            }
            __syncthreads();   // before anything of a later iteration reads it
        }
        if (go_on) continue;                                                         // :1026, :1029 jump over the closing test
        if ((count > 20 && abort_ba) || count > 100) break;                          // :1060
    }
    if (tid == 0) B.n_visited[blockIdx.x] = count;
    for (int i = count + tid; i < P.n_local; i += kCullThreads) B.verdict[P.local_off + i] = TC2LI_CULL_NOT_VISITED;
}

__global__ __launch_bounds__(256) void k_mp_cull(MpCullBatch B) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B.n_points) return;
    B.action[i] = cull::map_point_action(B.bad[i] != 0, B.n_found[i], B.n_visible[i], B.first_kf_id[i], B.n_obs[i], B.current_kf_id[i], B.th_obs);
}

void launch_keyframe_culling(const CullBatch& B, hipStream_t st) {
    if (B.n_local > 0) TC2LI_LAUNCH(k_cull_count, dim3(B.n_local), dim3(kCullThreads), 0, st, B);
    if (B.n_problems > 0) TC2LI_LAUNCH(k_cull_resolve, dim3(B.n_problems), dim3(kCullThreads), 0, st, B);
}

void launch_map_point_culling(const MpCullBatch& B, hipStream_t st) {
    if (B.n_points > 0) TC2LI_LAUNCH(k_mp_cull, dim3((B.n_points + 255) / 256), dim3(256), 0, st, B);
}

}  // namespace tc2li

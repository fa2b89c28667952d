// Device side of tc2li_keyframe_culling_batch / tc2li_map_point_culling_batch (include/tc2li_hip.h "local mapping: culling"):
// culling_host.cpp validates and concatenates the problems, culling_kernels.hip counts every local keyframe on the initial state, then
// walks each problem's list in order with the side effects of every cull applied.  The decision rules that the kernels and the host entry
// share are the inline functions at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

namespace tc2li {

// One problem = one LocalMapping::KeyFrameCulling call.  The tables of all problems are concatenated; indices stay problem-local and the
// kernels add the problem's offsets.  The two CSR offset tables have one more row than their table per problem, hence their own starts.
struct CullProblemDev {
    int32_t kf_off, n_kf;              // keyframe table
    int32_t slot_row_off, slot_off;    // slot_offsets rows start here (kf_off + problem index); slot arrays start at slot_off
    int32_t local_off, n_local;
    int32_t point_off, n_points;
    int32_t obs_row_off, obs_off;      // obs_offsets rows (point_off + problem index); observation arrays
    int32_t keyframes_in_map;
    int32_t flags;                     // bit 0 inertial, 1 imu_initialized, 2 inertial_ba2, 3 abort_ba
    int64_t current_id, last_id;
};

struct CullBatch {
    int n_problems, n_local;           // n_local: over all problems
    const CullProblemDev* problems;
    const int32_t* problem_of_local;   // [n_local]
    const uint8_t* kf_flags;
    const int64_t* kf_id;
    const double* kf_time;
    const float* kf_imu_pos;           // [kf][3]
    const float* kf_th_depth;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const float* slot_depth;
    const int8_t* slot_octave;
    const int32_t* local;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int8_t* obs_octave;
    const uint8_t* obs_weight;
    // the state the resolve kernel changes: uploaded with the initial values (point_nobs, point_bad, kf_prev, kf_next) or zeroed
    int32_t* kf_prev;
    int32_t* kf_next;
    int32_t* point_nobs;
    uint8_t* point_bad;
    uint8_t* kf_bad;                   // [kf] SetBadFlag went through in this call
    uint8_t* obs_dead;                 // [obs] erased
    uint8_t* point_changed;            // [point] an erasure took an observation from it
    int32_t* point_claim;              // [point] the last erasure pass that looked at it (a point held by two slots is handled once)
    // out
    int32_t* spec;                     // [n_local][2] nMPs, nRedundant on the initial state
    int32_t* verdict;                  // [n_local]
    int32_t* n_mps;
    int32_t* n_redundant;
    int32_t* n_visited;                // [n_problems]
};
void launch_keyframe_culling(const CullBatch& B, hipStream_t st);

struct MpCullBatch {
    int n_points, th_obs;
    const uint8_t* bad;
    const int32_t* n_found;
    const int32_t* n_visible;
    const int64_t* first_kf_id;
    const int32_t* n_obs;
    const int64_t* current_kf_id;
    uint8_t* action;
};
void launch_map_point_culling(const MpCullBatch& B, hipStream_t st);

namespace cull {

constexpr int kNd = 21;                // LocalMapping.cc:919
constexpr int kThObs = 3;              // :959-960

// :1021 with redundant_th of :923-929 (mbMonocular is false): int > float * int is evaluated in float
__host__ __device__ inline bool redundant(int n_redundant, int n_mps, bool inertial) {
    const float th = inertial ? 0.5f : 0.9f;
    return (float)n_redundant > th * (float)n_mps;
}

enum Gate { kGateContinue = 0, kGateNothing = 1, kGateMerge = 2 };
// :1025-1053 for a redundant keyframe of an inertial map: continue (the closing test is jumped over), nothing, or merge + SetBadFlag.
// time_prev / time_next / pos_prev are read only when both links exist.
__host__ __device__ inline Gate inertial_gate(int keyframes_in_map, int64_t kf_id, int64_t current_id, int64_t last_id, bool has_links,
                                              double time_prev, double time_next, const float* pos, const float* pos_prev,
                                              bool imu_initialized, bool inertial_ba2) {
    if (keyframes_in_map <= kNd) return kGateContinue;                                        // :1025
    if ((uint64_t)kf_id > (uint64_t)current_id - 2u) return kGateContinue;                    // :1028, unsigned long
    if (!has_links) return kGateNothing;                                                      // :1031
    const float t = (float)(time_next - time_prev);                                           // :1033
    if ((imu_initialized && (uint64_t)kf_id < (uint64_t)last_id && (double)t < 3.) || (double)t < 0.5) return kGateMerge;   // :1035
    if (inertial_ba2 || !(t < 3.0f)) return kGateNothing;                                     // :1044
    const float x = pos[0] - pos_prev[0], y = pos[1] - pos_prev[1], z = pos[2] - pos_prev[2];
    const float norm = sqrtf(x * x + (y * y + z * z));   // the summation order that defines parity (include/tc2li_hip.h)
    return (double)norm < 0.02 ? kGateMerge : kGateNothing;
}

// LocalMapping::MapPointCulling's chain of rules (:379-397) for one point
__host__ __device__ inline uint8_t map_point_action(bool bad, int n_found, int n_visible, int64_t first_kf_id, int n_obs,
                                                    int64_t current_kf_id, int th_obs) {
    if (bad) return 1;
    if ((float)n_found / (float)n_visible < 0.25f) return 2;                                  // MapPoint::GetFoundRatio
    const int age = (int)((uint32_t)(int)current_kf_id - (uint32_t)(int)first_kf_id);         // (int)a - (int)b, wrapping
    if (age >= 2 && n_obs <= th_obs) return 3;
    if (age >= 3) return 4;
    return 0;
}

}  // namespace cull
}  // namespace tc2li

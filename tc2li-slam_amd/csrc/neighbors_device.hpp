// Shared between the host entries (neighbors_host.cpp) and the kernel (neighbors_kernels.hip) of LocalMapping::SearchInNeighbors
// (SF/src/LocalMapping.cc:728-837; include/tc2li_hip.h "tc2li_search_in_neighbors_batch").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

#include "mappoint_device.hpp"
#include "matcher_device.hpp"

struct tc2li_keyframe_store;

namespace tc2li {

constexpr int kNbThreads = 256;
constexpr int kNbMaxObs = kMaxObservations;   // a point's observations: the descriptor step of k_map_points_refresh
constexpr int kNbMaxKeys = kMaxMatchKeys;     // keypoints of a keyframe = the longest stage-1 list; longer lists go in pieces of this
constexpr int kNbMaxPoints = 16384;           // points of a problem: one flag byte each in LDS
constexpr int kNbMaxKeyframes = 2048;         // keyframes of a problem: one flag byte each in LDS
constexpr int kNbMaxTargets = 210;
constexpr int kNbCounts = 8;
enum { kNbStatus = 0, kNbTargets, kNbCandidates, kNbOps, kNbObs, kNbRefreshed, kNbFused1, kNbFused2 };

// one keyframe row of a problem as both sides read it: the arrays of its store slot (device memory for the kernel, host memory for
// the host twin), the feature grid, the image bounds, and this problem's pose with the camera centre
struct NbKf {
    const float* keys;          // tc2li_keypoint records
    const uint8_t* desc;
    const float* u_right;
    const int32_t* cell_start;  // [kCellsPlus1]
    const uint16_t* items;
    int32_t n, pad_;
    float q[4], t[3], Ow[3], bounds[4];
};
struct NbConsts {
    float fx, fy, cx, cy, bf, log_scale_factor;
    int32_t n_levels, pad_;
    const float *scale_factors, *inv_level_sigma2;
};
struct NbObs { int32_t kf, idx; };

// where the tables of one problem start in the concatenated tables of the batch
struct NbProblemDev {
    int32_t n_kf, n_points, current, flags;            // flags: bit 0 inertial, bit 1 abort
    int32_t kf_off, kf_row_off, covis_off, slot_off;   // *_row_off: into the offset tables (one entry more per problem)
    int32_t point_off, point_row_off, obs_off, n_obs;
    int32_t pool_off, pool_size, op_off, op_room;
    int32_t obs_out_off, obs_out_room, snap_off, pad_;
    float last_level_scale; int32_t pad2_[3];
};
struct NbBatch {
    const NbProblemDev* problems;
    const NbKf* kfs;
    const uint8_t* kf_flags; const int32_t* prev_kf;
    const int32_t *covis_offsets, *covis, *slot_offsets;
    const uint8_t* point_flags; const int32_t* ref_kf; const float* ref_scale;
    const int32_t *obs_offsets, *obs_kf, *obs_index;
    NbConsts c;
    // state: uploaded with the initial values, changed in place
    int32_t* slot_point; uint8_t* points /* tc2li_map_point records */; int32_t *nobs, *found, *visible;
    // work
    NbObs* pool; int32_t *p_start, *p_len, *p_cap, *snap;
    // outputs
    int32_t *counts, *targets, *target_fused, *candidates; int32_t* ops /* tc2li_neighbors_op records */;
    uint8_t* bad; int32_t *replaced, *obs_offsets_out, *obs_kf_out, *obs_index_out, *desc_kf, *desc_index;
    uint8_t* refreshed; float *normals, *min_dist, *max_dist;
};
void launch_search_in_neighbors(const NbBatch& B, int n_problems, hipStream_t st);

// the device arrays of a store slot (pose fields untouched) and 1 + its highest octave; false: the slot is empty or out of range
bool keyframe_store_neighbors(tc2li_keyframe_store* S, int slot, NbKf* out, int32_t* n_levels);

}  // namespace tc2li

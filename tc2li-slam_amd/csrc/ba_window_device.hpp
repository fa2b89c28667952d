// Device side of tc2li_ba_window_batch (include/tc2li_hip.h "local mapping: the window of the local BA"): ba_window_host.cpp validates and
// concatenates the problems, ba_window_kernels.hip walks them -- marks, first occurrences, pose order, edge offsets in one workgroup per
// problem, then the edges and points by several workgroups per problem.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

namespace tc2li {

constexpr int kBawThreads = 256;           // per problem in k_baw_gather, per block in k_baw_edges
constexpr int kBawLdsKeyframes = 2048;     // up to here the marks of a problem's keyframes live in LDS (8 KB), beyond in global memory
constexpr int kBawLdsPoints = 8192;        // up to here the first-occurrence keys of a problem's points live in LDS (32 KB), beyond in global memory
constexpr int kBawEdgeBlocks = 8;          // workgroups per problem in k_baw_edges

// the marks of a keyframe (one int each): the three bits below, and from bit 3 up its place among the poses once that is known
constexpr int kBawMarkedLocal = 1;         // mnBALocalForKF == pKF->mnId (:66, :73)
constexpr int kBawLocal = 2;               // in lLocalKeyFrames (:65, :75)
constexpr int kBawFixed = 4;               // in lFixedCameras (:119)
constexpr int kBawPoseShift = 3;

// Where the keyframe store keeps the two arrays of a slot that the edges read (keyframe_store.cpp).
struct BawStore {
    const uint8_t* slots;                  // slot s starts at slots + s * stride
    size_t stride, keys, u_right;          // tc2li_keypoint [n] at +keys, float [n] at +u_right
};
// n_keypoints [max_keyframes] (-1: empty) and n_levels (1 + the highest octave held) of every slot, under the store's lock.
void keyframe_store_baw(tc2li_keyframe_store* store, BawStore* where, int32_t* n_keypoints, int32_t* n_levels, int capacity);
int keyframe_store_slots(const tc2li_keyframe_store* store);

// One problem = one gather.  The tables of all problems are concatenated; indices stay problem-local and the kernels add the problem's
// offsets.  The CSR offset tables have one more row than their table per problem, hence their own starts.
struct BawProblemDev {
    int64_t init_kf_id;
    int32_t kf_off, n_kf;                  // kf_slot, kf_id, kf_flags, poses7, marks scratch; slot_offsets rows start at kf_off + problem index
    int32_t slot_off;                      // slot_point
    int32_t cov_off, n_cov;                // cov_kf; the list scratch starts at cov_off + 2 * problem index and has n_cov + 2 entries
    int32_t point_off, n_points;           // point_flags, positions, per-point scratch; obs_offsets rows start at point_off + problem index
    int32_t obs_off;                       // obs_kf, obs_index
    int32_t current;
    int32_t mark_off;                      // start of the problem's marks in the global scratch, -1: they fit in LDS
    int32_t first_off;                     // start of the problem's first-occurrence keys in the global scratch, -1: they fit in LDS
    int32_t pose_off, pose_cap;            // pose_row / poses7_out / fixed
    int32_t pointo_off, point_cap;         // point_row / points3_out
    int32_t edge_off, edge_cap;            // edges
    int32_t pad_;
};

struct BawBatch {
    int n_problems;
    const BawProblemDev* problems;
    BawStore store;
    const float* inv_level_sigma2;
    const int32_t* kf_slot;
    const int64_t* kf_id;
    const uint8_t* kf_flags;
    const double* poses7;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const int32_t* cov_kf;
    const uint8_t* point_flags;
    const double* positions;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* obs_index;
    // scratch
    int32_t* marks_global;                 // marks of the problems with more than kBawLdsKeyframes keyframes
    int32_t* first_global;                 // first-occurrence keys of the problems with more than kBawLdsPoints points
    int32_t* kf_pose;                      // [all keyframes] the keyframe's place among the poses (k_baw_edges reads it), -1: none
    int32_t* members;                      // [all keyframes] the rows that get a pose, compacted
    int32_t* list_kf;                      // per problem n_cov + 2: lLocalKeyFrames as rows
    int32_t* list_start;                   // per problem n_cov + 2: where the slots of list keyframe i start in the concatenation
    int32_t* listed;                       // [all points] lLocalMapPoints as rows, complete whatever the capacity
    int32_t* edge_start;                   // [all points] by place in `listed`: the first edge of the point
    // out
    int32_t* counts;                       // [n_problems][TC2LI_BA_WINDOW_COUNTS]
    int32_t* lidar_pose_index;             // [n_problems][TC2LI_BA_WINDOW_MAX_LIDAR]
    int32_t* pose_row;
    double* poses7_out;
    uint8_t* fixed;
    int32_t* point_row;
    double* points3_out;
    tc2li_ba_edge* edges;
};
void launch_ba_window(const BawBatch& B, hipStream_t st);

}  // namespace tc2li

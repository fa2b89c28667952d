// Device side of tc2li_ba_window_batch (include/tc2li_hip.h "local mapping: the window of the local BA"): ba_window_host.cpp validates and
// concatenates the problems, ba_window_kernels.hip walks them -- marks, first occurrences, pose order, edge offsets in one workgroup per
// problem, then the edges and points by several workgroups per problem.  What this gather shares with the inertial one is in
// window_gather_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "window_gather_device.hpp"

namespace tc2li {

// the marks of a keyframe (one int each): the three bits below, and from bit 3 up its place among the poses once that is known
constexpr int kBawMarkedLocal = 1;         // mnBALocalForKF == pKF->mnId (:66, :73)
constexpr int kBawLocal = 2;               // in lLocalKeyFrames (:65, :75)
constexpr int kBawFixed = 4;               // in lFixedCameras (:119)
constexpr int kBawPoseShift = 3;

// What the visual gather adds to a problem (WindowProblemDev) and to a batch (WindowBatch).
struct BawProblemDev : WindowProblemDev {
    int32_t cov_off, n_cov;                // cov_kf; the list scratch starts at cov_off + 2 * problem index and has n_cov + 2 entries
    int32_t pose_off, pose_cap;            // pose_row / poses7_out / fixed
    int32_t cov_row1;                      // 0: cov_kf is the uploaded list.  Else 1 + the row of BawBatch::ord_offsets whose ordered row of the
                                           // resident map graph is the list; n_cov is then the most entries it can have
    int64_t init_kf_id;
};

struct BawBatch : WindowBatch {            // vertex_of is the keyframe's place among the poses
    const double* poses7;
    const int32_t* cov_kf;
    const int32_t* ord_offsets;            // the ordered connections of the resident map graph (MgConnTables), read where cov_row1 != 0
    const int32_t* ord_kf;
    int32_t ord_rows, ord_cap;             // rows of ord_offsets and entries of ord_kf per sequence and generation
    // scratch
    int32_t* list_kf;                      // per problem n_cov + 2: lLocalKeyFrames as rows
    // out
    int32_t* counts;                       // [n_problems][TC2LI_BA_WINDOW_COUNTS]
    int32_t* lidar_pose_index;             // [n_problems][TC2LI_BA_WINDOW_MAX_LIDAR]
    int32_t* pose_row;
    double* poses7_out;
    uint8_t* fixed;
};
void launch_ba_window(const BawBatch& B, hipStream_t st);

}  // namespace tc2li

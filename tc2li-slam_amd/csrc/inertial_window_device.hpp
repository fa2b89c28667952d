// Device side of tc2li_inertial_window_batch (include/tc2li_hip.h "local mapping: the window of the inertial local BA"):
// inertial_window_host.cpp validates and concatenates the problems, inertial_window_kernels.hip walks them -- chain, marks, first
// occurrences, the greedy fixed observers, vertex order, links and edge offsets in one workgroup per problem, then the edges and points by
// several workgroups per problem.  What this gather shares with the visual one is in window_gather_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "window_gather_device.hpp"

namespace tc2li {

constexpr int kIwMaxOpt = TC2LI_INERTIAL_WINDOW_MAX_OPT;

// the marks of a keyframe (one int each): three bits, and from bit 8 up the number of its edges (mVisEdges)
constexpr int kIwLocal = 1;                // mnBALocalForKF == pKF->mnId (:509, :515; taken back by :550)
constexpr int kIwFixedMark = 2;            // mnBAFixedForKF == pKF->mnId (:546, :551, :597)
constexpr int kIwFixedList = 4;            // in lFixedKeyFrames (:545, :552, :600)
constexpr int kIwEdgeShift = 8;

// What the inertial gather adds to a problem (WindowProblemDev) and to a batch (WindowBatch).
struct IwProblemDev : WindowProblemDev {
    int32_t nd;                            // Nd of :500
    int32_t rec_init, with_lidar;
    int32_t vertex_off, vertex_cap;        // kf_row / keyframes_out / fixed / has_imu
    int32_t link_cap;                      // links / link_kf2_row: kIwMaxOpt per problem
};

struct IwBatch : WindowBatch {             // vertex_of is the keyframe's place among the vertices
    const int32_t* prev_kf;
    const double* states;                  // [all keyframes][33]
    // out
    int32_t* counts;                       // [n_problems][TC2LI_INERTIAL_WINDOW_COUNTS]
    int32_t* lidar_pose_index;             // [n_problems][TC2LI_INERTIAL_WINDOW_MAX_LIDAR]
    tc2li_inertial_link* links;            // [n_problems][kIwMaxOpt]
    int32_t* link_kf2_row;                 // [n_problems][kIwMaxOpt]
    int32_t* kf_row;
    double* keyframes_out;                 // [vertices][33]
    uint8_t* fixed;
    uint8_t* has_imu;
};
void launch_inertial_window(const IwBatch& B, hipStream_t st);

}  // namespace tc2li

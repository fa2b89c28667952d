// Device side of tc2li_inertial_window_batch (include/tc2li_hip.h "local mapping: the window of the inertial local BA"):
// inertial_window_host.cpp validates and concatenates the problems, inertial_window_kernels.hip walks them -- chain, marks, first
// occurrences, the greedy fixed observers, vertex order, links and edge offsets in one workgroup per problem, then the edges and points by
// several workgroups per problem.  The slot arrays of the keyframe store are found as in ba_window_device.hpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_window_device.hpp"

namespace tc2li {

constexpr int kIwThreads = 256;            // per problem in k_iw_gather, per block in k_iw_edges
constexpr int kIwLdsKeyframes = 2048;      // up to here the marks of a problem's keyframes live in LDS (8 KB), beyond in global memory
constexpr int kIwLdsPoints = 8192;         // up to here the first-occurrence keys of a problem's points live in LDS (32 KB), beyond in global memory
constexpr int kIwEdgeBlocks = 8;           // workgroups per problem in k_iw_edges
constexpr int kIwMaxOpt = TC2LI_INERTIAL_WINDOW_MAX_OPT;

// the marks of a keyframe (one int each): three bits, and from bit 8 up the number of its edges (mVisEdges)
constexpr int kIwLocal = 1;                // mnBALocalForKF == pKF->mnId (:509, :515; taken back by :550)
constexpr int kIwFixedMark = 2;            // mnBAFixedForKF == pKF->mnId (:546, :551, :597)
constexpr int kIwFixedList = 4;            // in lFixedKeyFrames (:545, :552, :600)
constexpr int kIwEdgeShift = 8;

// One problem = one gather.  The tables of all problems are concatenated; indices stay problem-local and the kernels add the problem's
// offsets.  The CSR offset tables have one more row than their table per problem, hence their own starts.
struct IwProblemDev {
    int32_t kf_off, n_kf;                  // kf_slot, kf_id, kf_flags, prev_kf, states, kf_vertex / members scratch; slot_offsets rows start at kf_off + problem index
    int32_t slot_off;                      // slot_point
    int32_t point_off, n_points;           // point_flags, positions, per-point scratch; obs_offsets rows start at point_off + problem index
    int32_t obs_off;                       // obs_kf, obs_index
    int32_t current, nd;                   // Nd of :500
    int32_t rec_init, with_lidar;
    int32_t mark_off;                      // start of the problem's marks in the global scratch, -1: they fit in LDS
    int32_t first_off;                     // start of the problem's first-occurrence keys in the global scratch, -1: they fit in LDS
    int32_t vertex_off, vertex_cap;        // kf_row / keyframes_out / fixed / has_imu
    int32_t pointo_off, point_cap;         // point_row / points3_out
    int32_t edge_off, edge_cap;            // edges
    int32_t link_cap, pad_;                // links / link_kf2_row: kIwMaxOpt per problem
};

struct IwBatch {
    int n_problems;
    const IwProblemDev* problems;
    BawStore store;
    const float* inv_level_sigma2;
    const int32_t* kf_slot;
    const int64_t* kf_id;
    const uint8_t* kf_flags;
    const int32_t* prev_kf;
    const double* states;                  // [all keyframes][33]
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const uint8_t* point_flags;
    const double* positions;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* obs_index;
    // scratch
    int32_t* marks_global;                 // marks of the problems with more than kIwLdsKeyframes keyframes
    int32_t* first_global;                 // first-occurrence keys of the problems with more than kIwLdsPoints points
    int32_t* kf_vertex;                    // [all keyframes] the keyframe's place among the vertices (k_iw_edges reads it), -1: none
    int32_t* members;                      // [all keyframes] the rows that get a vertex, compacted
    int32_t* listed;                       // [all points] lLocalMapPoints as rows, complete whatever the capacity
    int32_t* edge_start;                   // [all points] by place in `listed`: the first edge of the point
    // out
    int32_t* counts;                       // [n_problems][TC2LI_INERTIAL_WINDOW_COUNTS]
    int32_t* lidar_pose_index;             // [n_problems][TC2LI_INERTIAL_WINDOW_MAX_LIDAR]
    tc2li_inertial_link* links;            // [n_problems][kIwMaxOpt]
    int32_t* link_kf2_row;                 // [n_problems][kIwMaxOpt]
    int32_t* kf_row;
    double* keyframes_out;                 // [vertices][33]
    uint8_t* fixed;
    uint8_t* has_imu;
    int32_t* point_row;
    double* points3_out;
    tc2li_ba_edge* edges;
};
void launch_inertial_window(const IwBatch& B, hipStream_t st);

}  // namespace tc2li

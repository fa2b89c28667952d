// Device side of tc2li_ba_window_structure_batch (include/tc2li_hip.h "the optimiser's index structure of a window"): what
// ba_build_structure (ba_structure.hpp) makes from the downloaded window, built from the gather's device output (BawBatch,
// ba_window_device.hpp) without the window leaving the device.  ba_structure_kernels.hip writes every window's arrays into a scratch area
// sized from the gather's capacities and a small size record; the host reads the records, lays out the input blocks (ba_input_layout) and
// moves the pieces there device to device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ba_window_device.hpp"

namespace tc2li {

constexpr int kBasThreads = 256;        // per window in k_bas_structure, per block of slots in k_bas_blocks
constexpr int kBasMaxFree = 24;         // kSchurLeanMaxFree: the lean sparse path
constexpr int kBasMaxPoses = 1024;      // the poses' marks / numbers live in LDS (4 KB)
constexpr int kBasMaxPoints = 6144;     // the points' first edge, first slot (24 KB each) and place in the slice (6 KB) live in LDS: 59 KB in all

enum BasStatus : int32_t {
    kBasNone = 0,        // nothing built: the window is ABORTED or a list did not fit (the host answers from the counts)
    kBasBuilt = 1,
    kBasDeclined = 2,    // outside the device range: more than kBasMaxFree free poses, kBasMaxPoses poses or kBasMaxPoints points
    kBasInvalid = 3      // a listed point without an edge, a point with more than 256 edges, more than 256 points in a group
};
// what the host needs of a window before it can place the pieces (ba_detail::BaStructureSizes follows from it)
struct BasSizes {
    int32_t status, n_free, n_free_edges, n_schur_slices, n_groups, n_blocks, max_group_landmarks, pad_;
};
// where a window's arrays start in the scratch area (ints; blk_rows in bytes); every start is a multiple of 16 bytes
struct BasWindowDev {
    int64_t pose_var, pt_off, pt_edges, pv_off, fl_off, fl_pose, fl_lm, fl_place, fl_edge, slice_off, grp_k0, grp_l0, blk_off, blk_rows;
    int32_t max_blocks;                 // room of blk_off / blk_rows in blocks of 256 slots
    int32_t use_lidar;                  // the keyframes of lidar_pose_index count as used (the window gets the LiDAR edge)
};
struct BasBatch {
    int n_windows, max_blocks;          // max_blocks: the largest of the windows' max_blocks (the second launch's grid)
    const BawProblemDev* problems;      // the gather's: offsets and capacities of its outputs
    const int32_t* counts;
    const int32_t* lidar_pose_index;
    const uint8_t* fixed;
    const int32_t* edge_start;
    const tc2li_ba_edge* edges;
    const BasWindowDev* windows;
    int32_t* scratch;
    uint8_t* scratch_rows;
    BasSizes* sizes;
};
void launch_ba_structure(const BasBatch& B, hipStream_t st);

// The outlier rule after the BA (OptimizerWithLidar.cc:402-449) for one window, no point bad: the monocular edges with chi2 > 5.991 or a
// depth that is not positive in creation order, then the stereo edges with 7.815 -- the arithmetic of tc2li_ba_window_outliers.  edges,
// chi2 and depth_positive are device memory; erase_pose / erase_point [capacity] and n_erase (the count, whatever the capacity) are
// pinned host memory, written by the kernel.
struct BasOutlierTask {
    const tc2li_ba_edge* edges;
    const double* chi2;
    const uint8_t* depth_positive;
    int32_t *erase_pose, *erase_point, *n_erase;
    int32_t n_edges, capacity;
};
void launch_ba_outliers(const BasOutlierTask* tasks /* pinned */, int n, hipStream_t st);

// ---- what ba_window_host.cpp lends to a follow-up of the gather ------------------------------------------------------------------------
// The gather of tc2li_ba_window_batch with two hooks: after_gather runs when the gather's kernels are queued (the outputs are in device
// memory, nothing is downloaded yet), after_download when the counts and lists are in the problems' host arrays and no list was short of
// room.  Both run under the lock of the gather's buffers, which stay as they are until the call returns.  A negative return ends the call
// with that code.
struct BawFollow {
    virtual ~BawFollow() {}
    virtual int after_gather(const BawBatch& B, const BawProblemDev* dev, hipStream_t st) = 0;
    virtual int after_counts() { return 0; }   // the counts are in the problems' arrays, every list fits, no list is written yet
    virtual int after_download(const BawBatch& B, const BawProblemDev* dev, hipStream_t st) = 0;
};
// space: which set of buffers (0: tc2li_ba_window_batch's own; 1 + g: the one that goes with lock-step context g).  edges_optional: a
// problem whose `edges` is NULL keeps its edges on the device (they are gathered into room for every observation, and not downloaded).
struct MgLease;   // map_graph_host.hpp
int ba_window_batch_run(const char* entry, tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                        const float* inv_level_sigma2, int n_levels, void* stream, BawFollow* follow, int space, bool edges_optional,
                        MgLease* resident = nullptr);
// resident: the problems carry no table; problem p reads sequence resident->seq[p] of the map graph, whose lock the lease holds.
// resident_windows makes such problems of a graph-reading entry's (windows: a copy of them) and takes the lease.
int resident_cov(const char* entry, MgLease* lease, const tc2li_ba_window_problem* windows, int n_problems);   // ... and reads the neighbour lists from the graph
int resident_windows(const char* entry, MgLease* lease, tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences, int n_problems,
                     std::vector<tc2li_ba_window_problem>* windows);

}  // namespace tc2li

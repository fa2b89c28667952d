// What the two gathers of a local-BA window from the flat graph share on the device: tc2li_ba_window_batch (ba_window_device.hpp,
// ba_window_kernels.hip) and tc2li_inertial_window_batch (inertial_window_device.hpp, inertial_window_kernels.hip).  Both list the points
// of their window's keyframes by first occurrence, count every point's edges, give the marked keyframes a vertex in id order, and then
// write points and edges with the one kernel k_window_edges.  The records below are the part of a problem and of a batch that this
// needs; each gather derives its own from them.  The functions are __forceinline__ and live here so that both kernel files inline them
// (no device linkage between translation units); window_gather_host.hpp is the host side of the same split.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"
#include "launch.hpp"

namespace tc2li {

constexpr int kWinThreads = 256;           // per problem in the gather kernels, per block in k_window_edges
constexpr int kWinLdsKeyframes = 2048;     // up to here the marks of a problem's keyframes live in LDS (8 KB), beyond in global memory
constexpr int kWinLdsPoints = 8192;        // up to here the first-occurrence keys of a problem's points live in LDS (32 KB), beyond in global memory
constexpr int kWinEdgeBlocks = 8;          // workgroups per problem in k_window_edges

// Where the keyframe store keeps the two arrays of a slot that the edges read (keyframe_store.cpp).
struct BawStore {
    const uint8_t* slots;                  // slot s starts at slots + s * stride
    size_t stride, keys, u_right;          // tc2li_keypoint [n] at +keys, float [n] at +u_right
};
// n_keypoints [max_keyframes] (-1: empty) and n_levels (1 + the highest octave held) of every slot, under the store's lock.
void keyframe_store_baw(tc2li_keyframe_store* store, BawStore* where, int32_t* n_keypoints, int32_t* n_levels, int capacity);
int keyframe_store_slots(const tc2li_keyframe_store* store);

// One problem = one gather.  The tables of all problems are concatenated; indices stay problem-local and the kernels add the problem's
// offsets.  The CSR offset tables have one more row than their table per problem, hence their own starts.  The graph tables have starts
// of their own (t_*, slot_row, obs_row) beside those of the scratch and of the gather's own tables (kf_off, point_off): a batch of host
// arrays fills them with the same places (WindowTransfer::add), a batch that reads the resident map graph (map_graph_device.hpp) with
// the places of the problem's sequence in the slab, which two problems may share.
struct WindowProblemDev {
    int32_t kf_off, n_kf;                  // the gather's own keyframe tables (cov-independent inputs it uploads per problem), vertex_of / members
    int32_t slot_off;                      // slot_point of a batch of host arrays (= t_slot there)
    int32_t point_off, n_points;           // per-point scratch: listed, edge_start
    int32_t obs_off;                       // obs_kf, obs_index of a batch of host arrays (= t_obs there)
    int32_t t_kf, t_slot, t_point, t_obs;  // kf_slot, kf_id, kf_flags, poses7 | slot_point | point_flags, positions | obs_kf, obs_index
    int32_t slot_row, obs_row;             // the first row of the problem's slot_offsets / obs_offsets
    int32_t current;
    int32_t mark_off;                      // start of the problem's marks in the global scratch, -1: they fit in LDS
    int32_t first_off;                     // start of the problem's first-occurrence keys in the global scratch, -1: they fit in LDS
    int32_t pointo_off, point_cap;         // point_row / points3_out
    int32_t edge_off, edge_cap;            // edges
};

struct WindowBatch {
    int n_problems;
    int problem_bytes;                     // the gather's problem record begins with a WindowProblemDev and is this long
    const void* problems;
    BawStore store;
    const float* inv_level_sigma2;
    const int32_t* kf_slot;
    const int64_t* kf_id;
    const uint8_t* kf_flags;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const uint8_t* point_flags;
    const double* positions;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* obs_index;
    // scratch
    int32_t* marks_global;                 // marks of the problems with more than kWinLdsKeyframes keyframes
    int32_t* first_global;                 // first-occurrence keys of the problems with more than kWinLdsPoints points
    int32_t* vertex_of;                    // [all keyframes] the keyframe's place among the poses / vertices (k_window_edges reads it), -1: none
    int32_t* members;                      // [all keyframes] the rows that get a vertex, compacted
    int32_t* listed;                       // [all points] lLocalMapPoints as rows, complete whatever the capacity
    int32_t* edge_start;                   // [all points] by place in `listed`: the first edge of the point
    int32_t* n_emit;                       // [n_problems] the listed points k_window_edges writes: all of them when the window came out (the
                                           // status is OK) and every list fits its device capacity, else 0 -- the host then answers from the
                                           // counts (another status, or TC2LI_ERR_CAPACITY) and reads no list
    // out
    int32_t* point_row;
    double* points3_out;
    tc2li_ba_edge* edges;
};
// problem i of the batch as the gather's own record, or as its common part
template <class Problem>
__host__ __device__ __forceinline__ const Problem& window_problem(const WindowBatch& B, int i) {
    return *reinterpret_cast<const Problem*>(static_cast<const uint8_t*>(B.problems) + (size_t)i * B.problem_bytes);
}
// after a gather kernel, on its stream (ba_window_kernels.hip)
void launch_window_edges(const WindowBatch& B, hipStream_t st);

// The LDS / global choice of a problem's marks and first-occurrence keys, made once per workgroup: problem(marks, first) is inlined four
// times, so that inside it the address space of both arrays is known.
template <class Problem>
__device__ __forceinline__ void window_dispatch(const WindowBatch& B, const WindowProblemDev& P, int* lds_marks, int* lds_first, Problem problem) {
    if (P.mark_off < 0 && P.first_off < 0) problem(lds_marks, lds_first);
    else if (P.mark_off < 0) problem(lds_marks, B.first_global + P.first_off);
    else if (P.first_off < 0) problem(B.marks_global + P.mark_off, lds_first);
    else problem(B.marks_global + P.mark_off, B.first_global + P.first_off);
}

// lLocalMapPoints: the points of the keyframes rows[0 .. n_rows) in the order of their first occurrence.  The slots of those keyframes,
// concatenated in list order, are numbered q = 0, 1, ...; every slot does an integer atomicMin of q on its point's key (first[], all
// 0x7fffffff on entry), the slot whose q is the minimum is the point's first occurrence, and a block prefix sum over those in q order is
// the point's place -- no sort, and minima do not depend on their order.  A point whose flags meet bad_mask is passed over.  q0, the
// number of the first slot of rows[li], is the sum of the slot counts of rows[0 .. li): every thread walks all of the list anyway and
// keeps that sum as it goes, so it is stored nowhere.  rows may be global memory or LDS; all threads arrive.  Returns the number listed;
// `listed` is complete after the caller's next barrier.
__device__ __forceinline__ int window_list_points(const int32_t* rows, int n_rows, const int32_t* slot_row, const int32_t* slot_point,
                                                  const uint8_t* pflags, int bad_mask, int* first, int32_t* listed, int* scan) {
    const int tid = threadIdx.x;
    int q0 = 0;
    for (int li = 0; li < n_rows; ++li) {
        const int k = rows[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0;
        for (int s = tid; s < len; s += kWinThreads) {
            const int p = slot_point[s0 + s];
            if (p >= 0 && !(pflags[p] & bad_mask)) atomicMin(&first[p], q0 + s);
        }
        q0 += len;
    }
    __syncthreads();
    int n_listed = 0;
    q0 = 0;
    for (int li = 0; li < n_rows; ++li) {
        const int k = rows[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0;
        for (int base = 0; base < len; base += kWinThreads) {
            const int s = base + tid;
            const int p = s < len ? slot_point[s0 + s] : -1;
            const bool take = p >= 0 && first[p] == q0 + s;                          // only a point that passed the flags has a key
            int tot;
            const int at = block_scan_excl<kWinThreads>(take ? 1 : 0, scan, &tot);
            if (take) listed[n_listed + at] = p;
            n_listed += tot;
        }
        q0 += len;
    }
    return n_listed;
}

// The rows that get a vertex, compacted into `members` in row order, and vertex_of cleared.  word(mark) says in bit 0 whether the row is
// a member and may count something else about it in bit 16: both ride in the one prefix sum (at most 256 of each per step).  Returns the
// members; *n_counted is the sum of the bits 16.  All threads arrive; ends with a barrier.
template <class Word>
__device__ __forceinline__ int window_compact_members(const int* marks, int n_kf, int32_t* members, int32_t* vertex_of, int* scan, int* n_counted,
                                                      Word word) {
    int n_members = 0, n_high = 0;
    for (int base = 0; base < n_kf; base += kWinThreads) {
        const int k = base + (int)threadIdx.x;
        const int v = k < n_kf ? word(marks[k]) : 0;
        int tot;
        const int at = block_scan_excl<kWinThreads>(v, scan, &tot);
        if (v & 1) members[n_members + (at & 0xffff)] = k;
        if (k < n_kf) vertex_of[k] = -1;
        n_members += tot & 0xffff;
        n_high += tot >> 16;
    }
    __syncthreads();
    *n_counted = n_high;
    return n_members;
}

// Vertex-id order: a pose's place is the number of members with a smaller (kf_id, row); members ascend by row.  A few hundred members at
// most: members^2 / 256 compares per thread.  vertex_of gets every member's place, and write(row, place, id) is called for the places
// below cap.  Ends with a barrier: vertex_of was written by other threads.
template <class Write>
__device__ __forceinline__ void window_rank_members(const int64_t* kf_id, const int32_t* members, int n_members, int32_t* vertex_of, int cap,
                                                    Write write) {
    for (int i = threadIdx.x; i < n_members; i += kWinThreads) {
        const int k = members[i];
        const int64_t id = kf_id[k];
        int r = 0;
        for (int j = 0; j < n_members; ++j) {
            const int64_t idj = kf_id[members[j]];
            r += (idj < id || (idj == id && j < i)) ? 1 : 0;
        }
        vertex_of[k] = r;
        if (r < cap) write(k, r, id);
    }
    __syncthreads();
}

}  // namespace tc2li

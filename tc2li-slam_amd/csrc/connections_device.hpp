// Device side of tc2li_update_connections_batch / tc2li_update_best_covisibles_batch (include/tc2li_hip.h "local mapping: covisibility
// graph"): connections_host.cpp validates and concatenates the problems, connections_kernels.hip votes, orders the current keyframe's
// lists, then orders the list of every changed neighbour.  The key that defines the order is shared with the host entry.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

namespace tc2li {

constexpr int kConnThreads = 256;          // per problem in k_conn_vote
constexpr int kConnLdsKeyframes = 2048;    // up to here the vote counters of a problem live in LDS (8 KB), beyond in global memory
constexpr int kConnRankLanes = 64;         // one wavefront orders one list

// One problem = one KeyFrame::UpdateConnections call.  The tables of all problems are concatenated; indices stay problem-local and the
// kernels add the problem's offsets.  The CSR offset tables have one more row than their table per problem, hence their own starts.
struct ConnProblemDev {
    int32_t kf_off, n_kf;
    int32_t conn_row_off, conn_off;        // conn_offsets rows start here (kf_off + problem index); conn arrays start at conn_off
    int32_t slot_off, n_slots;
    int32_t point_off;
    int32_t obs_row_off, obs_off;          // obs_offsets rows (point_off + problem index); obs_kf
    int32_t current;
    int32_t flags;                         // bit 0 first_connection, bit 1 is_init_kf
    int32_t hist_off;                      // start of the problem's counters in the global scratch, -1: they fit in LDS
    int32_t counter_off, counter_cap;      // counter_kf / counter_weight
    int32_t ordered_off, ordered_cap;      // ordered_*, touched_*, item scratch; changed_offsets starts at ordered_off + problem index
    int32_t changed_off, changed_cap;      // changed_kf / changed_weight
};

struct ConnBatch {
    int n_problems, n_items;               // n_items: the ordered capacities of all problems
    const ConnProblemDev* problems;
    const int32_t* problem_of_item;        // [n_items]
    const uint8_t* kf_flags;
    const int32_t* conn_offsets;
    const int32_t* conn_kf;
    const int32_t* conn_weight;
    const int32_t* slot_point;
    const uint8_t* point_bad;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    // scratch
    int32_t* hist;                         // counters of the problems with more than kConnLdsKeyframes keyframes
    int32_t* touched_weight;               // [n_items] the weight AddConnection carries to touched_kf
    int32_t* item_off;                     // [n_items] where the neighbour's list starts in the problem's changed_*, -1: unchanged
    uint8_t* item_found;                   // [n_items] the neighbour's row holds the current keyframe already
    // out
    int32_t* counts;                       // [n_problems][TC2LI_CONNECTIONS_COUNTS]
    int32_t* counter_kf;
    int32_t* counter_weight;
    int32_t* ordered_kf;
    int32_t* ordered_weight;
    int32_t* touched_kf;
    uint8_t* touched_changed;
    int32_t* changed_offsets;
    int32_t* changed_kf;
    int32_t* changed_weight;
};
void launch_update_connections(const ConnBatch& B, hipStream_t st);

struct CovisBatch {
    int n_rows;
    const int32_t* row_offsets;
    const int32_t* row_kf;
    const int32_t* row_weight;
    const uint8_t* bad;
    int32_t* out_count;                    // [n_rows] entries that are not bad
    int32_t* out_kf;                       // the ordered list of row r starts at row_offsets[r]
    int32_t* out_weight;
};
void launch_update_best_covisibles(const CovisBatch& B, hipStream_t st);

namespace conn {

// The order of KeyFrame.cc:224 / :461 as one unsigned number: std::sort on pair<int, KeyFrame*> ascends by (weight, keyframe), the lists
// are its result read from the back.  Rows are distinct within a list, so the keys are, and an entry's place in the list is the number
// of keys greater than its own.  0 is no key (a bad keyframe, a lane past the end).
__host__ __device__ inline uint64_t key(int32_t weight, int32_t kf) {
    return ((((uint64_t)((uint32_t)weight ^ 0x80000000u)) << 32) | (uint32_t)kf) + 1u;
}
__host__ __device__ inline int32_t key_kf(uint64_t k) { return (int32_t)(uint32_t)(k - 1u); }
__host__ __device__ inline int32_t key_weight(uint64_t k) { return (int32_t)((uint32_t)((k - 1u) >> 32) ^ 0x80000000u); }

}  // namespace conn
}  // namespace tc2li

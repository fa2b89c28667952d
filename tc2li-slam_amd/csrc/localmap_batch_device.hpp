// Shared between the host entry and the kernels of tc2li_local_map_update_batch: Tracking::UpdateLocalMap for many sequences in one call.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "localmap_device.hpp"

namespace tc2li {

constexpr int kLmbLdsKeyframes = 2048;  // up to this many keyframes the vote counters and marks of a problem live in LDS
constexpr int kLmbPointGroups = 8;      // workgroups per problem in the point phase: the grid is n_problems times this
constexpr int kLmbThreads = 256;

// one problem: the sequence's mirror (its graph tables; its scratch is not used) and where the problem's rows start in the batch's tables
struct LmbProblem {
    LocalMapDev map;
    int32_t fp_off, n_fp;      // frame points / cleared flags
    int32_t temporal_last_kf;
    int32_t key_off;           // first-occurrence keys [n_points]
    int32_t vote_off;          // vote counters and marks [n_keyframes] in the work buffer, -1: in LDS
    int32_t list_off;          // local keyframes [n_keyframes]; the reversed offsets table starts at list_off + the problem's number
    int32_t pad_[2];
};

struct LmbBatch {
    int32_t n_problems;
    const LmbProblem* problems;
    const int32_t* frame_points;
    // work: keys, votes and marks are zero when the first kernel starts
    int32_t* keys;          // 0x7fffffff - the first position of a point in its problem's reversed concatenation, 0: not met
    int32_t* votes;
    uint8_t* marks;
    int32_t* kf_list;
    int32_t* rev_base;
    int32_t* info;          // [n_problems][2]: local keyframes, entries of the reversed concatenation
    int32_t* block_counts;  // [n_problems * kLmbPointGroups] kept entries of every slice
    int32_t* block_base;    // where a slice's kept entries start in lists
    int32_t* lists;         // per problem [local keyframes | local points], the problems one after the other without gaps
    // outputs
    int32_t* counts;        // [n_problems][TC2LI_LOCAL_MAP_COUNTS]
    int32_t* seg;           // [n_problems + 1] where a problem's lists start in lists; the last entry is their total
    uint8_t* cleared;
};

void launch_local_map_batch(const LmbBatch& B, hipStream_t st);

}  // namespace tc2li

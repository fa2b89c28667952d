// Shared between the host entries (process_keyframe_host.cpp) and the kernels (process_keyframe_kernels.hip) of
// LocalMapping::ProcessNewKeyFrame (SF/src/LocalMapping.cc:312-352; include/tc2li_hip.h "tc2li_process_new_keyframe_batch").
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

#include "connections_device.hpp"
#include "neighbors_device.hpp"

namespace tc2li {

constexpr int kPkThreads = 256;             // per problem in k_pkf_associate
constexpr int kPkRefreshWaves = 4;          // wavefronts (= points) per workgroup of k_pkf_refresh
constexpr int kPkMaxObs = kNbMaxObs;        // a point's observations after the call: the descriptor rows of a wavefront in LDS
constexpr int kPkCounts = TC2LI_PROCESS_KEYFRAME_COUNTS;
enum { kPkStatus = 0, kPkAssociated, kPkRecent, kPkObs };
constexpr int kPkNoSlot = 0x7fffffff;       // first_slot of a point that no slot associates

// one keyframe row of a problem: what the refresh reads of its store slot (device memory for the kernels, host memory for the twin)
struct PkKf {
    const uint8_t* desc;                    // nullptr: kf_slot -1, a row that observes no point of the slot row
    float centre[3];
    int32_t pad_;
};

// Where the tables of one problem start in the concatenated tables of the batch.  The keyframe, slot, point and observation tables are
// laid out as ConnProblemDev lays them out (the connection kernels read them): offset tables have one row more per problem.
struct PkProblemDev {
    int32_t n_kf, n_slots, n_points, current;
    int32_t kf_off, slot_off, point_off, point_row_off;
    int32_t obs_off, obs_out_off;           // the entry rows; the end-state rows (room: entry rows + occupied slots)
    int32_t list_off, item_off;             // associated_* / recent (room: occupied slots); the problem's first item of k_pkf_refresh
    const float* u_right;                   // of the current keyframe's slot
    float last_level_scale; int32_t pad_;
};
struct PkBatch {
    int n_problems, n_items;                // n_items: the occupied slots of all problems, the most points the refresh can meet
    const PkProblemDev* problems;
    const PkKf* kfs;
    const uint8_t* kf_flags;
    const int32_t* slot_point;
    const uint8_t* point_bad;
    const float* positions; const int32_t *nobs, *ref_kf; const float* ref_scale;
    const int32_t *obs_offsets, *obs_kf, *obs_index;
    int32_t* first_slot;                    // work, [points]: the lowest slot that associates the point, kPkNoSlot: none
    // outputs
    int32_t *counts, *associated_slot, *associated_point, *recent, *nobs_out;
    int32_t *obs_offsets_out, *obs_kf_out, *obs_index_out, *desc_kf, *desc_index;
    uint8_t* refreshed; float *normals, *min_dist, *max_dist;
};
void launch_process_keyframe(const PkBatch& B, hipStream_t st);

// tc2li_host_update_connections_batch's body for problems that are valid already (connections_host.cpp): the sizes into counts, and with
// `write` the lists when those of every problem fit.  -> n_problems, or TC2LI_ERR_CAPACITY with the error set under `entry`.
int host_connections(const char* entry, const tc2li_connections_problem* problems, int n_problems, bool write);
// "" or what is wrong with a problem (the checks of tc2li_update_connections_batch)
const char* connections_what_is_wrong(const tc2li_connections_problem& in);

}  // namespace tc2li

// Device side of the resident map graph (include/tc2li_hip.h "the map graph resident on the device"): map_graph_host.cpp keeps the slab,
// the per-row metadata and the checks, map_graph_kernels.hip applies an edit log.  The slab is table-major -- every table holds all
// sequences, a sequence's part at sequence * capacity -- so that a gather (ba_window_kernels.hip) reads a sequence's tables at 32-bit
// starts from one base pointer per table, as it reads the concatenated tables of a batch of host arrays.  The observation CSR cannot be
// edited in place: it has two generations per sequence, an apply reads the one and writes the other, and the host remembers which is
// current.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"
#include "connections_device.hpp"

namespace tc2li {

constexpr int kMgThreads = 256;            // per sequence in k_mg_apply, per block in k_mg_write
constexpr int kMgLdsRow = 256;             // up to here (old entries + the ADD edits of the row) a touched observation row is merged in LDS, beyond in global memory
constexpr int kMgWriteBlocks = 8;          // workgroups per sequence in k_mg_write
// A touched observation row finds its edits by walking the log from its first to its last edit.  The sum of those stretches over the
// touched rows of one log is the work of one workgroup; the host refuses a log beyond this many edit reads (a few milliseconds of one
// workgroup), so that no log can hold a shared card for long.  One keyframe's worth of edits -- one edit per point -- reads one each.
constexpr int64_t kMgMaxWalk = 1 << 22;

struct MgTables {
    int32_t* kf_slot;                      // [S][cap_kf]
    int64_t* kf_id;
    uint8_t* kf_flags;
    double* poses7;                        // [S][cap_kf][7]
    int32_t* slot_offsets;                 // [S][cap_kf + 1]
    int32_t* slot_point;                   // [S][cap_slot]
    uint8_t* point_flags;                  // [S][cap_pt]
    double* positions;                     // [S][cap_pt][3]
    int32_t* obs_offsets;                  // [S][2][cap_pt + 1]
    int32_t* obs_kf;                       // [S][2][cap_obs]
    int32_t* obs_index;
    // scratch of an apply, per sequence
    int32_t* pt_head;                      // [S][cap_pt] the first edit of the log on the point's observation row, 0x7fffffff: untouched
    int32_t* pt_last;                      // the last one
    int32_t* pt_len;                       // the row's new length
    int32_t* pt_stage;                     // first the row's ADD edits counted, then where its merged row is staged
    int32_t* touched;                      // the touched rows, compacted
    int32_t* stage_kf;                     // [S][cap_obs] the merged rows until the new offsets are known
    int32_t* stage_index;
    int32_t cap_kf, cap_slot, cap_pt, cap_obs;
};

// One sequence of an apply: 64 bytes.  The sizes are the resident ones before the log; the host has checked every edit against them.
struct MgApplyDev {
    int32_t sequence, generation;          // the observation CSR that is current
    int32_t n_kf, n_points, n_slot, n_obs;
    int32_t edit_off, n_edits, value_off;  // the sequence's part of the batch's edits and values
    int32_t n_points_new;                  // n_points + the ADD_POINT edits of the log
    int32_t pad_[6];
};
static_assert(sizeof(MgApplyDev) == 64, "an apply moves 64 bytes per sequence beside its edits and values");

struct MgApplyBatch {
    MgTables T;
    int n;
    const MgApplyDev* deltas;
    const tc2li_map_graph_edit* edits;
    const double* values;
    int32_t* totals;                       // [n] the observation entries of every sequence after its log
};
void launch_map_graph_apply(const MgApplyBatch& B, hipStream_t st);

// ---- the commit of solved local-BA windows (map_graph_commit_kernels.hip; include/tc2li_hip.h "the closing step of
// LocalLVBundleAdjustment") ----
// A committed window is one MgApplyDev record and nothing else from the host: the first six members as an apply has them (n_edits = two per
// erase pair, value_off 0, n_points_new = n_points), and in pad_ where the window lies in the gather's device output and in the device
// copy of the erase lists.
enum MgCommitPad { kMgcPoseOff = 0, kMgcPointOff = 1, kMgcPoses = 2, kMgcPoints = 3, kMgcEraseAt = 4, kMgcEraseCap = 5 };
constexpr int kMgcThreads = 256;           // per block of the scatter kernel
constexpr int kMgcNoEdit = -1;             // no op: k_mg_apply passes over it.  In place of a SET_SLOT whose keyframe row holds no such slot, and of both
                                           // edits of an erase pair the erase-log kernel could not resolve: the host then sees the window's status word
                                           // and drops the whole commit before any table is written
struct MgCommitBatch {
    MgTables T;
    int n, n_erasing;                      // records; the first n_erasing of them have erase pairs
    int max_rows;                          // the largest n_poses + n_points among the records (the scatter's grid)
    uint32_t flags;                        // TC2LI_BA_COMMIT_*
    const MgApplyDev* records;
    // the gather's device output with the final estimate written back over it, and the outlier kernel's device output
    const int32_t* pose_row;
    const uint8_t* fixed;
    const double* poses7;
    const int32_t* point_row;
    const double* points3;
    const int32_t* erase;                  // a window's pairs: the pose indices at erase_at, the point indices at erase_at + erase_cap
    tc2li_map_graph_edit* edits;           // out: the erase log of record r at records[r].edit_off
    int32_t* status;                       // out [n_erasing]: 0, or 1 when a pair was not resolved
};
void launch_map_graph_commit_erase_log(const MgCommitBatch& B, hipStream_t st);
void launch_map_graph_commit_scatter(const MgCommitBatch& B, hipStream_t st);

// ---- the covisibility graph of the resident map (include/tc2li_hip.h "the covisibility graph on the resident map graph") ----
// Two CSRs over the keyframe rows of every sequence, in an allocation of their own made by tc2li_map_graph_connections_reserve: the
// weights (mConnectedKeyFrameWeights, a row ascending by keyframe row) and the ordered lists (mvpOrderedConnectedKeyFrames /
// mvOrderedWeights as last written).  Neither can be edited in place -- rows grow, and the current keyframe's rows are replaced -- so
// both have two generations, as the observation CSR has: an update reads the one and writes the whole of the other, and the host flips
// the sequence's generation only when every sequence of the call fitted its reserve.  Until then the written generation is not the
// state: that is what makes a refused call leave no trace.
struct MgConnTables {
    int32_t* conn_offsets;                 // [S][2][cap_kf + 1]
    int32_t* conn_kf;                      // [S][2][cap_e]
    int32_t* conn_weight;
    int32_t* ord_offsets;                  // [S][2][cap_kf + 1]
    int32_t* ord_kf;                       // [S][2][cap_e]
    int32_t* ord_weight;
    int32_t cap_e;
};
enum MgConnMode { kMgcUpdate = 0, kMgcErase = 1 };
// One sequence of an update or an erase: 64 bytes, and all that goes up.
struct MgConnDev {
    int32_t sequence, obs_generation, conn_generation;
    int32_t n_kf;                          // the resident keyframe rows
    int32_t conn_rows;                     // the rows the connection offsets cover; the rows appended since are empty and get their offsets first
    int32_t current;                       // the keyframe of the call
    int32_t slot_begin, n_slots;           // its slot row within the sequence's slot_point
    int64_t init_kf_id;
    int32_t first_connection, mode;
    int32_t pad_[4];
};
static_assert(sizeof(MgConnDev) == 64, "an update of the connections moves 64 bytes per sequence");
constexpr int kMgcStatusWords = 4;         // per sequence, device to host: fitted, weight entries, ordered entries of the written generation, 0

struct MgConnBatch {
    MgTables T;
    MgConnTables C;
    int n, max_kf;                         // records; the most keyframe rows among them (the grid of the neighbours' kernel)
    const MgConnDev* records;
    ConnBatch B;                           // the resident tables and the scratch as the kernels of tc2li_update_connections_batch read them
    ConnProblemDev* problems;              // [n] written by the first kernel from the records (= B.problems)
    int32_t* row_of;                       // [n][2][cap_kf] scratch: a keyframe row's place among the changed touched ones (-1: none), their new list lengths
    int32_t* status;                       // [n][kMgcStatusWords]
};
void launch_map_graph_connections(const MgConnBatch& M, hipStream_t st);

// A sequence as a gather reads it: the sizes, and where its tables start in the slab's tables (WindowProblemDev::t_*, slot_row, obs_row).
struct MgSequenceView {
    int32_t n_kf, n_points, n_slot, n_obs;
    int32_t t_kf, t_slot, t_point, t_obs, slot_row, obs_row;
    const int32_t* kf_store_slot;          // host: the store slot of every keyframe row
    const int32_t* kf_keys;                // host: the keypoints that slot held when the row's observation indices were checked
    // the ordered connections, for a gather that takes its neighbour list from them: the sequence's current generation of ord_offsets as
    // a row of MgConnTables::ord_offsets, the keyframe rows those offsets cover (a row beyond is empty) and the entries of the CSR
    int32_t ord_row, conn_rows, n_ordered;
};

}  // namespace tc2li

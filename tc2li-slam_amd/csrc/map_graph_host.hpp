// How a gather reads the resident map graph (map_graph_host.cpp): a lease holds the graph's lock for the length of the gather, says
// where the tables of every problem's sequence lie, and notes on release what the gather uploaded.
#pragma once
#include <vector>

#include "ba_window_device.hpp"
#include "map_graph_device.hpp"

namespace tc2li {

struct MgLease {
    tc2li_map_graph_handle* graph = nullptr;
    const int32_t* sequences = nullptr;
    int n = 0;
    MgTables T{};
    std::vector<MgSequenceView> seq;       // per problem
    int64_t uploaded = -1;                 // host-to-device bytes of the gather, -1: it did not get that far
    MgConnTables C{};                      // the connections (all NULL before tc2li_map_graph_connections_reserve)
    bool cov_resident = false;             // the gather reads every problem's neighbour list from the ordered row of its current keyframe

    MgLease() {}
    MgLease(const MgLease&) = delete;
    MgLease& operator=(const MgLease&) = delete;
    ~MgLease();
    // 0, or TC2LI_ERR_INVALID with the error set: a graph of another store, a sequence out of range or never set
    int acquire(const char* entry, tc2li_map_graph_handle* g, tc2li_keyframe_store* store, const int32_t* sequences, int n);
};

// ---- the commit of solved windows (include/tc2li_hip.h "the closing step of LocalLVBundleAdjustment"), called by the solve entry under
// the lease of its gather ----
// A committed window whose result the lock-step group left on the device.
struct MgCommitWindow {
    int32_t sequence;
    int32_t pose_off, point_off, n_poses, n_points;   // where it lies in the gather's device output
    int32_t n_erase, erase_at, erase_cap;             // ... and in the device copy of the erase lists
    const int32_t* erase_point;                       // host: its erase_point [n_erase], for the walk bound of the erase log
};
// The gather's device output with the final estimate written back over poses7 / points3, and the device copy of the erase lists.
struct MgCommitSource {
    const int32_t* pose_row;
    const uint8_t* fixed;
    const double* poses7;
    const int32_t* point_row;
    const double* points3;
    const int32_t* erase;
};
// The tables of one sequence of the lease's graph as host arrays (a window finished on the host path builds its log from them).
struct MgHostTables {
    std::vector<int32_t> kf_slot, slot_offsets, slot_point, obs_offsets, obs_kf, obs_index;
    std::vector<int64_t> kf_id;
    std::vector<uint8_t> kf_flags, point_flags;
    std::vector<double> poses7, positions;
    tc2li_map_graph_tables tables{};
};
int map_graph_read(const char* entry, const MgLease& lease, int sequence, MgHostTables* out);
// device_windows through the commit kernels, host_logs through the apply; no sequence twice among them (the caller has checked).  Every
// check comes before the first write to a table: a negative return leaves the graph as it was.
int map_graph_commit(const char* entry, const MgLease& lease, const MgCommitSource& src, const std::vector<MgCommitWindow>& device_windows,
                     const tc2li_map_graph_delta* host_logs, int n_host_logs, uint32_t flags, hipStream_t st);

}  // namespace tc2li

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

    MgLease() {}
    MgLease(const MgLease&) = delete;
    MgLease& operator=(const MgLease&) = delete;
    ~MgLease();
    // 0, or TC2LI_ERR_INVALID with the error set: a graph of another store, a sequence out of range or never set
    int acquire(const char* entry, tc2li_map_graph_handle* g, tc2li_keyframe_store* store, const int32_t* sequences, int n);
};

}  // namespace tc2li

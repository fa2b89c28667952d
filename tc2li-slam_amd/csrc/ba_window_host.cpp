// tc2li_ba_window_batch / tc2li_host_ba_window_batch / tc2li_ba_window_limits / tc2li_ba_window_outliers (include/tc2li_hip.h "local
// mapping: the window of the local BA"): the gather of OptimizerWithLidar::LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:63-130,
// :157-187, :226-253, :263-384) and its outlier rule (:402-449) on a flat copy of the graph.  This file validates the problems and either
// walks them in plain C++ with the reference's mark fields or concatenates them for ba_window_kernels.hip.  ba_window_batch_run is the
// device entry with two hooks for what follows the gather on the device (ba_structure_device.hpp: the structure kernels, the BA).  What
// this gather does as the inertial one does -- the graph checks, the three passes of the host entry, the edge records, the common tables'
// way to the device and back -- is window_gather_host.hpp's; here are the checks, the walk, the tables and the outputs that are its own.
#include <algorithm>
#include <cstring>

#include "ba_structure_device.hpp"
#include "ba_window_device.hpp"
#include "map_graph_host.hpp"
#include "window_gather_host.hpp"

namespace tc2li {
namespace {

// "" or what is wrong with the problem
const char* validate(const tc2li_ba_window_problem& in, const SlotTable& slots, int n_levels, bool edges_optional) {
    if (in.n_keyframes < 0 || in.n_points < 0 || in.n_cov < 0) return "negative size";
    if (in.pose_capacity < 0 || in.point_capacity < 0 || in.edge_capacity < 0) return "negative capacity";
    if (!in.kf_slot || !in.kf_id || !in.kf_flags || !in.poses7 || !in.slot_offsets || !in.obs_offsets || !in.counts || !in.lidar_pose_index)
        return "null kf_slot, kf_id, kf_flags, poses7, slot_offsets, obs_offsets, counts or lidar_pose_index";
    if (in.current < 0 || in.current >= in.n_keyframes) return "current out of range";
    if ((in.n_cov && !in.cov_kf) || (in.n_points && (!in.point_flags || !in.positions))) return "null cov_kf, point_flags or positions";
    if (in.pose_capacity && (!in.pose_row || !in.poses7_out || !in.fixed)) return "null pose output";
    if (in.point_capacity && (!in.point_row || !in.points3_out)) return "null point output";
    if (in.edge_capacity && !in.edges && !edges_optional) return "null edges";
    return validate_graph(in, slots, n_levels, [](int) { return ""; }, [&]() -> const char* {
        std::vector<uint8_t> named(in.n_keyframes, 0);
        named[in.current] = 1;
        for (int i = 0; i < in.n_cov; ++i) {
            const int k = in.cov_kf[i];
            if (k < 0 || k >= in.n_keyframes) return "cov_kf out of range";
            if (named[k]) return "cov_kf names a row twice or the current keyframe";
            named[k] = 1;
        }
        return "";
    });
}

// The same for a problem whose tables are a sequence of the resident map graph: the tables were checked when they were set and edited, so
// what is left is the problem's own -- sizes, outputs, current, cov_kf -- and, in O(n_keyframes), that the store still holds the slots of
// the sequence's keyframe rows with no octave beyond n_levels.
const char* validate_resident(const tc2li_ba_window_problem& in, const MgSequenceView& seq, const SlotTable& slots, int n_levels, bool edges_optional) {
    if (in.n_cov < 0) return "negative size";
    if (in.pose_capacity < 0 || in.point_capacity < 0 || in.edge_capacity < 0) return "negative capacity";
    if (!in.counts || !in.lidar_pose_index) return "null counts or lidar_pose_index";
    if (in.current < 0 || in.current >= in.n_keyframes) return "current out of range";
    if (in.n_cov && !in.cov_kf) return "null cov_kf";
    if (in.pose_capacity && (!in.pose_row || !in.poses7_out || !in.fixed)) return "null pose output";
    if (in.point_capacity && (!in.point_row || !in.points3_out)) return "null point output";
    if (in.edge_capacity && !in.edges && !edges_optional) return "null edges";
    const int n_store = (int)slots.n.size();
    for (int k = 0; k < in.n_keyframes; ++k) {
        const int s = seq.kf_store_slot[k];
        if (s < 0 || s >= n_store || slots.n[s] < 0) return "a kf_slot is empty or out of range";
        if (slots.levels[s] > n_levels) return "a slot holds an octave outside [0, n_levels)";
        // the resident obs_index were checked against the keypoints the slot held then: a slot put again with fewer would be read beyond its end
        if (slots.n[s] < seq.kf_keys[k]) return "a kf_slot holds fewer keypoints than when the row's observations were checked";
    }
    std::vector<uint8_t> named(in.n_keyframes, 0);
    named[in.current] = 1;
    for (int i = 0; i < in.n_cov; ++i) {
        const int k = in.cov_kf[i];
        if (k < 0 || k >= in.n_keyframes) return "cov_kf out of range";
        if (named[k]) return "cov_kf names a row twice or the current keyframe";
        named[k] = 1;
    }
    return "";
}

// edges_optional: a problem without an edge array leaves its edges on the device, whatever their number
bool fits(const tc2li_ba_window_problem& in, const int32_t* counts, bool edges_optional = false) {
    return counts[TC2LI_BA_WINDOW_N_POSES] <= in.pose_capacity && counts[TC2LI_BA_WINDOW_N_POINTS] <= in.point_capacity &&
           (counts[TC2LI_BA_WINDOW_N_EDGES] <= in.edge_capacity || (edges_optional && !in.edges));
}

int capacity_error(const char* entry, const tc2li_ba_window_problem* problems, int p) {
    const tc2li_ba_window_problem& in = problems[p];
    set_error("%s: problem %d needs room for %d poses, %d points and %d edges and has %d, %d and %d", entry, p, in.counts[TC2LI_BA_WINDOW_N_POSES],
              in.counts[TC2LI_BA_WINDOW_N_POINTS], in.counts[TC2LI_BA_WINDOW_N_EDGES], in.pose_capacity, in.point_capacity, in.edge_capacity);
    return TC2LI_ERR_CAPACITY;
}

// The walk of the reference with its mark fields: mnBALocalForKF / mnBAFixedForKF of a keyframe, mnBALocalForKF of a point, as "== pKF->mnId".
// counts is always written; the lists only with `write`.  Returns whether they fit the capacities.
bool window_one(const tc2li_ba_window_problem& in, const tc2li_keyframe_view* views, const float* inv_level_sigma2, bool write) {
    int32_t* counts = in.counts;
    std::fill(counts, counts + TC2LI_BA_WINDOW_COUNTS, 0);
    enum { kLocalFor = 1, kFixedFor = 2 };
    std::vector<uint8_t> kf_mark(in.n_keyframes, 0), point_mark(in.n_points, 0);
    std::vector<int32_t> local, fixed_cams, listed, clouds;
    auto other = [&](int k) { return (in.kf_flags[k] & 3) != 0; };                   // isBad() || GetMap() != pCurrentMap
    local.push_back(in.current);                                                     // :65
    kf_mark[in.current] |= kLocalFor;                                                // :66
    for (int i = 0; i < in.n_cov; ++i) {                                             // :70-76
        const int k = in.cov_kf[i];
        kf_mark[k] |= kLocalFor;                                                     // :73
        if (!other(k)) local.push_back(k);                                           // :74-75
    }
    int num_fixed = 0;                                                               // :79
    for (int k : local) {                                                            // :82-104
        if (in.kf_id[k] == in.init_kf_id) num_fixed = 1;                             // :85-88
        for (int s = in.slot_offsets[k]; s < in.slot_offsets[k + 1]; ++s) {
            const int p = in.slot_point[s];
            if (p < 0 || (in.point_flags[p] & 3)) continue;                          // :93-94
            if (!point_mark[p]) { listed.push_back(p); point_mark[p] = 1; }          // :97-101
        }
    }
    for (int p : listed)                                                             // :108-122
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            const int k = in.obs_kf[o];
            if (kf_mark[k] & (kLocalFor | kFixedFor)) continue;                      // :115
            kf_mark[k] |= kFixedFor;                                                 // :117
            if (!other(k)) fixed_cams.push_back(k);                                  // :118-119
        }
    num_fixed += (int)fixed_cams.size();                                             // :123
    counts[TC2LI_BA_WINDOW_NUM_FIXED_KF] = num_fixed;
    if (num_fixed == 0) {                                                            // :126-130
        counts[TC2LI_BA_WINDOW_STATUS] = TC2LI_BA_WINDOW_ABORTED;
        return true;
    }
    // the vertices in id order (:157-187)
    std::vector<int32_t> order = local;
    order.insert(order.end(), fixed_cams.begin(), fixed_cams.end());
    const std::vector<int32_t> pose_of = vertices_by_id(in.kf_id, in.n_keyframes, &order);
    for (int k : local)                                                              // :228-233
        if (in.kf_flags[k] & 4) clouds.push_back(k);
    const int n_lidar = clouds.size() > 2 ? (int)std::min<size_t>(clouds.size(), TC2LI_BA_WINDOW_MAX_LIDAR) : 0;   // :235, :244-245
    int n_edges = 0, n_without = 0;
    for (int p : listed) {                                                           // :263-384, counted
        int ne = 0;
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) ne += (!other(in.obs_kf[o]) && in.obs_index[o] >= 0) ? 1 : 0;
        n_edges += ne;
        n_without += ne == 0;
    }
    counts[TC2LI_BA_WINDOW_NUM_OPT_KF] = (int)local.size();                          // :171
    counts[TC2LI_BA_WINDOW_N_POSES] = (int)order.size();
    counts[TC2LI_BA_WINDOW_N_POINTS] = (int)listed.size();
    counts[TC2LI_BA_WINDOW_N_EDGES] = n_edges;
    counts[TC2LI_BA_WINDOW_N_LIDAR] = n_lidar;
    counts[TC2LI_BA_WINDOW_N_POINTS_WITHOUT_EDGE] = n_without;
    if (!fits(in, counts)) return false;
    if (!write) return true;
    for (size_t r = 0; r < order.size(); ++r) {
        const int k = order[r];
        in.pose_row[r] = k;
        memcpy(in.poses7_out + 7 * r, in.poses7 + 7 * (size_t)k, 7 * sizeof(double));
        in.fixed[r] = ((kf_mark[k] & kFixedFor) || in.kf_id[k] == in.init_kf_id) ? 1 : 0;   // :181, :164
    }
    for (int i = 0; i < TC2LI_BA_WINDOW_MAX_LIDAR; ++i) in.lidar_pose_index[i] = i < n_lidar ? pose_of[clouds[i]] : -1;   // :247-253
    emit_points_and_edges(in, views, inv_level_sigma2, listed, pose_of,                 // :263-384
                          [&](int o) { return !other(in.obs_kf[o]) && in.obs_index[o] >= 0; });   // :281, :286, :313
    return true;
}

// [0]: tc2li_ba_window_batch's; [1 + group]: a follow-up's that keeps the buffers for the length of a BA on the lock-step context `group`
struct BawSpaces { PackedSpace s[1 + kMaxLockstepGroups]; };

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_ba_window_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_ba_window_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kWinLdsKeyframes; out[1] = kWinLdsPoints; out[2] = kWinThreads;
    return 3;
}

extern "C" int tc2li_ba_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                                        const uint8_t* point_bad_now, int n_points, int32_t* erase_pose, int32_t* erase_point, int capacity) {
    const char* entry = "tc2li_ba_window_outliers";
    const int rc = outliers_check(entry, edges, edge_chi2, edge_depth_positive, n_edges, n_points, erase_pose, erase_point, capacity,
                                  n_points && !point_bad_now);
    if (rc < 0) return rc;
    // :406-419 for the monocular edges, :436-449 for the stereo ones
    return outliers_emit(entry, edges, n_edges, erase_pose, erase_point, capacity, [&](int i, bool stereo) {
        if ((edges[i].u_right >= 0) != stereo || point_bad_now[edges[i].point]) return false;   // :411, :441
        return edge_chi2[i] > (stereo ? 7.815 : 5.991) || !edge_depth_positive[i];              // :414, :444 (erased: :417, :447)
    });
}

extern "C" int tc2li_host_ba_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_ba_window_problem* problems, int n_problems,
                                          const float* inv_level_sigma2, int n_levels) {
    const char* entry = "tc2li_host_ba_window_batch";
    return host_window_batch(
        entry, views, n_views, problems, n_problems, inv_level_sigma2, n_levels,
        [&](const tc2li_ba_window_problem& in, const SlotTable& slots) { return validate(in, slots, n_levels, false); },
        [&](const tc2li_ba_window_problem& in, bool write) { return window_one(in, views, inv_level_sigma2, write); },
        [&](int p) { return capacity_error(entry, problems, p); });
}

extern "C" int tc2li_ba_window_batch(tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                                     const float* inv_level_sigma2, int n_levels, void* stream) {
    return ba_window_batch_run("tc2li_ba_window_batch", store, problems, n_problems, inv_level_sigma2, n_levels, stream, nullptr, 0, false);
}

// The problems of a graph-reading entry as ba_window_batch_run takes them: no table, the sizes of the problem's sequence.
int tc2li::resident_windows(const char* entry, MgLease* lease, tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences, int n_problems,
                            std::vector<tc2li_ba_window_problem>* windows) {
    if (!store || n_problems < 0) { set_error("%s: null store or negative size", entry); return TC2LI_ERR_INVALID; }
    const int rc = lease->acquire(entry, graph, store, sequences, n_problems);
    if (rc < 0) return rc;
    for (int p = 0; p < n_problems; ++p) {
        tc2li_ba_window_problem& w = (*windows)[p];
        w.kf_slot = nullptr; w.kf_id = nullptr; w.kf_flags = nullptr; w.poses7 = nullptr; w.slot_offsets = nullptr; w.slot_point = nullptr;
        w.point_flags = nullptr; w.positions = nullptr; w.obs_offsets = nullptr; w.obs_kf = nullptr; w.obs_index = nullptr;
        w.n_keyframes = lease->seq[p].n_kf; w.n_points = lease->seq[p].n_points;
    }
    return 0;
}

// 0, or TC2LI_ERR_INVALID: the lease of an entry that reads the neighbour lists from the graph; the problems carry none
int tc2li::resident_cov(const char* entry, MgLease* lease, const tc2li_ba_window_problem* windows, int n_problems) {
    if (!lease->C.ord_kf) { set_error("%s: tc2li_map_graph_connections_reserve was not called", entry); return TC2LI_ERR_INVALID; }
    for (int p = 0; p < n_problems; ++p)
        if (windows[p].cov_kf || windows[p].n_cov) { set_error("%s: problem %d: cov_kf / n_cov must be NULL / 0, the list is the graph's", entry, p); return TC2LI_ERR_INVALID; }
    lease->cov_resident = true;
    return 0;
}

extern "C" int tc2li_ba_window_graph_cov_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                               const tc2li_ba_window_problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels, void* stream) {
    const char* entry = "tc2li_ba_window_graph_cov_batch";
    if (n_problems > 0 && !problems) { set_error("%s: null problems", entry); return TC2LI_ERR_INVALID; }
    std::vector<tc2li_ba_window_problem> windows(problems, problems + std::max(n_problems, 0));
    MgLease lease;
    int rc = resident_windows(entry, &lease, store, graph, sequences, n_problems, &windows);
    if (rc < 0) return rc;
    rc = resident_cov(entry, &lease, windows.data(), n_problems);
    if (rc < 0) return rc;
    return ba_window_batch_run(entry, store, windows.data(), n_problems, inv_level_sigma2, n_levels, stream, nullptr, 0, false, &lease);
}

extern "C" int tc2li_ba_window_graph_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences, const tc2li_ba_window_problem* problems,
                                           int n_problems, const float* inv_level_sigma2, int n_levels, void* stream) {
    const char* entry = "tc2li_ba_window_graph_batch";
    if (n_problems > 0 && !problems) { set_error("%s: null problems", entry); return TC2LI_ERR_INVALID; }
    std::vector<tc2li_ba_window_problem> windows(problems, problems + std::max(n_problems, 0));
    MgLease lease;
    const int rc = resident_windows(entry, &lease, store, graph, sequences, n_problems, &windows);
    if (rc < 0) return rc;
    return ba_window_batch_run(entry, store, windows.data(), n_problems, inv_level_sigma2, n_levels, stream, nullptr, 0, false, &lease);
}

int tc2li::ba_window_batch_run(const char* entry, tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                               const float* inv_level_sigma2, int n_levels, void* stream, BawFollow* follow, int space, bool edges_optional, MgLease* resident) {
    if (!store) {
        set_error("%s: null store", entry);
        return TC2LI_ERR_INVALID;
    }
    SlotTable slots;
    BawStore where{};
    slot_table_from_store(store, &slots, &where);
    if (space < 0 || space > kMaxLockstepGroups) { set_error("%s: no such buffer set", entry); return TC2LI_ERR_INVALID; }
    const int rc = validate_all(entry, problems, n_problems, inv_level_sigma2, n_levels,
                                [&](const tc2li_ba_window_problem& in) {
                                    return resident ? validate_resident(in, resident->seq[&in - problems], slots, n_levels, edges_optional)
                                                    : validate(in, slots, n_levels, edges_optional);
                                });
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    WindowTransfer<tc2li_ba_window_problem, BawProblemDev> T(problems, n_problems);
    size_t n_cov = 0, n_pose = 0;
    T.resident = resident != nullptr;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_ba_window_problem& in = problems[p];
        const int edge_room = edges_optional && !in.edges ? INT_MAX : in.edge_capacity;
        BawProblemDev& d = resident ? T.add(p, edge_room, resident->seq[p].n_slot, resident->seq[p].n_obs) : T.add(p, edge_room);
        if (resident) {
            const MgSequenceView& s = resident->seq[p];
            d.t_kf = s.t_kf; d.t_slot = s.t_slot; d.t_point = s.t_point; d.t_obs = s.t_obs; d.slot_row = s.slot_row; d.obs_row = s.obs_row;
        }
        d.init_kf_id = in.init_kf_id;
        d.cov_off = (int32_t)n_cov; d.n_cov = in.n_cov;
        if (resident && resident->cov_resident) {   // the list is the resident ordered row of current: no keyframe twice, not current itself
            const MgSequenceView& s = resident->seq[p];
            const bool has_row = in.current < s.conn_rows;                           // a row appended since is empty
            d.n_cov = has_row ? std::min(s.n_kf - 1, s.n_ordered) : 0;               // what the list scratch must hold
            d.cov_row1 = has_row ? 1 + s.ord_row + in.current : 0;
        }
        d.pose_off = (int32_t)n_pose; d.pose_cap = std::min(in.pose_capacity, in.n_keyframes);
        n_cov += d.n_cov; n_pose += d.pose_cap;
        if (std::max(T.most_rows(p), n_cov + 2 * (size_t)p) > kMaxRows) return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    T.take_inputs(n_levels);
    size_t o_pose, o_cov;
    const bool cov_resident = resident && resident->cov_resident;
    if (resident) { o_pose = o_cov = T.io.off; T.io.off += cov_resident ? 0 : n_cov * 4; }   // the poses are resident; cov_kf follows the level table
    else { o_pose = T.io.take(T.n_kf * 56); o_cov = T.io.take(n_cov * 4); }
    T.take_outputs(TC2LI_BA_WINDOW_COUNTS);
    const size_t o_p7 = T.io.take(n_pose * 56), o_prow = T.io.take(n_pose * 4), o_fixed = T.io.take(n_pose);
    T.take_work();
    const size_t w_lkf = T.work.take((n_cov + 2 * np) * 4);
    PackedSpace& S = shutdown_owned<BawSpaces>().s[space];
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    TC2LI_HIP_CHECK(T.upload_tables(inv_level_sigma2, n_levels, st, [&](int, const tc2li_ba_window_problem& in, const BawProblemDev& d) {
        if (!resident) T.io.put(o_pose, d.kf_off, in.poses7, (size_t)in.n_keyframes, 56);
        if (!cov_resident) T.io.put(o_cov, d.cov_off, in.cov_kf, (size_t)in.n_cov, 4);
    }));
    if (resident) resident->uploaded = (int64_t)T.up_bytes;
    uint8_t* d = T.d_io;
    const BawProblemDev* dev = T.dev.data();
    BawBatch B{};
    T.bind(B, where);
    B.poses7 = (const double*)(d + o_pose);
    if (resident) {   // the tables of the slab in place of the uploaded ones
        const MgTables& G = resident->T;
        B.kf_slot = G.kf_slot; B.kf_id = G.kf_id; B.kf_flags = G.kf_flags; B.slot_offsets = G.slot_offsets; B.slot_point = G.slot_point;
        B.point_flags = G.point_flags; B.positions = G.positions; B.obs_offsets = G.obs_offsets; B.obs_kf = G.obs_kf; B.obs_index = G.obs_index;
        B.poses7 = G.poses7;
    }
    B.cov_kf = (const int32_t*)(d + o_cov); B.list_kf = T.dev_work<int32_t>(w_lkf);
    if (cov_resident) { B.ord_offsets = resident->C.ord_offsets; B.ord_kf = resident->C.ord_kf; B.ord_rows = resident->T.cap_kf + 1; B.ord_cap = resident->C.cap_e; }
    B.counts = (int32_t*)(d + T.o_counts); B.lidar_pose_index = (int32_t*)(d + T.o_lidar); B.pose_row = (int32_t*)(d + o_prow);
    B.poses7_out = (double*)(d + o_p7); B.fixed = d + o_fixed;
    launch_ba_window(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    if (follow) {
        const int frc = follow->after_gather(B, dev, st);
        if (frc < 0) { (void)stream_wait_blocking(st); return frc; }
    }
    bool edges_wanted = !edges_optional;
    for (int p = 0; p < n_problems && !edges_wanted; ++p) edges_wanted = problems[p].edges != nullptr;
    if (edges_wanted) TC2LI_HIP_CHECK(T.download(T.down_from, T.io.off, st));
    else {   // the edges -- five sevenths of the result -- stay where they are
        TC2LI_HIP_CHECK(T.download(T.down_from, T.o_edges, st));
        TC2LI_HIP_CHECK(T.download(T.o_after_edges, T.io.off, st));
    }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    const int short_of_room =
        T.copy_counts([&](const tc2li_ba_window_problem& in, const int32_t* counts) { return fits(in, counts, edges_optional); });
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    if (follow) {
        const int frc = follow->after_counts();
        if (frc < 0) return frc;
    }
    T.copy_out([&](int, const tc2li_ba_window_problem& in, const BawProblemDev& D) {
        const size_t n_po = (size_t)in.counts[TC2LI_BA_WINDOW_N_POSES];
        T.io.get(in.pose_row, o_prow, D.pose_off, n_po, 4); T.io.get(in.poses7_out, o_p7, D.pose_off, n_po, 56);
        T.io.get(in.fixed, o_fixed, D.pose_off, n_po, 1);
    });
    if (follow) {
        const int frc = follow->after_download(B, dev, st);
        if (frc < 0) return frc;
    }
    return n_problems;
}

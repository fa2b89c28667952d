// tc2li_inertial_window_batch / tc2li_host_inertial_window_batch / tc2li_inertial_window_limits / tc2li_inertial_window_outliers
// (include/tc2li_hip.h "local mapping: the window of the inertial local BA"): the gather of OptimizerWithLidar::LocalLVIBA
// (SF/src/OptimizerWithLidar.cc:489-607, :632-727, :729-800, :832-969; the same text in Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512
// and on) and its outlier rule (:985-1045) on a flat copy of the graph.  This file validates the problems and either walks them in plain C++
// with the reference's mark fields or concatenates them for inertial_window_kernels.hip.  What this gather does as the visual one does
// -- the graph checks, the three passes of the host entry, the edge records, the common tables' way to the device and back -- is
// window_gather_host.hpp's; here are the checks, the walk, the tables and the outputs that are its own.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "inertial_window_device.hpp"
#include "window_gather_host.hpp"

static_assert(sizeof(tc2li_inertial_link) == 32, "ABI layout");
static_assert(sizeof(tc2li_inertial_keyframe) == 264, "ABI layout");
static_assert(sizeof(tc2li_inertial_window_problem) == 232, "ABI layout");

namespace tc2li {
namespace {

int window_nd(const tc2li_inertial_window_problem& in) {                              // :493-500
    return std::min(in.keyframes_in_map - 2, in.large ? TC2LI_INERTIAL_WINDOW_MAX_OPT : 10);
}

// "" or what is wrong with the problem
const char* validate(const tc2li_inertial_window_problem& in, const SlotTable& slots, int n_levels) {
    if (in.n_keyframes < 0 || in.n_points < 0 || in.keyframes_in_map < 0) return "negative size";
    if (in.kf_capacity < 0 || in.point_capacity < 0 || in.edge_capacity < 0 || in.link_capacity < 0) return "negative capacity";
    if (!in.kf_slot || !in.kf_id || !in.kf_flags || !in.prev_kf || !in.states || !in.slot_offsets || !in.obs_offsets || !in.counts ||
        !in.lidar_pose_index)
        return "null kf_slot, kf_id, kf_flags, prev_kf, states, slot_offsets, obs_offsets, counts or lidar_pose_index";
    if (in.current < 0 || in.current >= in.n_keyframes) return "current out of range";
    if (in.n_points && (!in.point_flags || !in.positions)) return "null point_flags or positions";
    if (in.kf_capacity && (!in.kf_row || !in.keyframes_out || !in.fixed || !in.has_imu)) return "null keyframe output";
    if (in.point_capacity && (!in.point_row || !in.points3_out)) return "null point output";
    if (in.edge_capacity && !in.edges) return "null edges";
    if (in.link_capacity && (!in.links || !in.link_kf2_row)) return "null links or link_kf2_row";
    return validate_graph(
        in, slots, n_levels,
        [&](int k) { return (in.prev_kf[k] < -1 || in.prev_kf[k] >= in.n_keyframes) ? "prev_kf out of range" : ""; },
        [&]() -> const char* {
            // the window and the one predecessor behind it name no row twice
            int chain[TC2LI_INERTIAL_WINDOW_MAX_OPT + 1], n = 0;
            chain[n++] = in.current;
            const int want = std::max(window_nd(in), 1) + 1;
            while (n < want && in.prev_kf[chain[n - 1]] >= 0) {
                const int k = in.prev_kf[chain[n - 1]];
                for (int i = 0; i < n; ++i)
                    if (chain[i] == k) return "the prev_kf chain returns to a keyframe of the window";
                chain[n++] = k;
            }
            return "";
        });
}

bool fits(const tc2li_inertial_window_problem& in, const int32_t* counts) {
    return counts[TC2LI_INERTIAL_WINDOW_N_VERTICES] <= in.kf_capacity && counts[TC2LI_INERTIAL_WINDOW_N_POINTS] <= in.point_capacity &&
           counts[TC2LI_INERTIAL_WINDOW_N_EDGES] <= in.edge_capacity && counts[TC2LI_INERTIAL_WINDOW_N_LINKS] <= in.link_capacity;
}

int capacity_error(const char* entry, const tc2li_inertial_window_problem* problems, int p) {
    const tc2li_inertial_window_problem& in = problems[p];
    set_error("%s: problem %d needs room for %d keyframes, %d points, %d edges and %d links and has %d, %d, %d and %d", entry, p,
              in.counts[TC2LI_INERTIAL_WINDOW_N_VERTICES], in.counts[TC2LI_INERTIAL_WINDOW_N_POINTS], in.counts[TC2LI_INERTIAL_WINDOW_N_EDGES],
              in.counts[TC2LI_INERTIAL_WINDOW_N_LINKS], in.kf_capacity, in.point_capacity, in.edge_capacity, in.link_capacity);
    return TC2LI_ERR_CAPACITY;
}

// The walk of the reference with its mark fields: mnBALocalForKF / mnBAFixedForKF of a keyframe, mnBALocalForKF of a point, as
// "== pKF->mnId".  counts is always written; the lists only with `write`.  Returns whether they fit the capacities.
bool window_one(const tc2li_inertial_window_problem& in, const tc2li_keyframe_view* views, const float* inv_level_sigma2, bool write) {
    int32_t* counts = in.counts;
    std::fill(counts, counts + TC2LI_INERTIAL_WINDOW_COUNTS, 0);
    std::vector<uint8_t> local_for(in.n_keyframes, 0), fixed_for(in.n_keyframes, 0), point_mark(in.n_points, 0);
    std::vector<int32_t> opt, fixed_kfs, listed, vis_edges(in.n_keyframes, 0);
    const int Nd = window_nd(in);                                                    // :500
    opt.push_back(in.current);                                                       // :508
    local_for[in.current] = 1;                                                       // :509
    for (int i = 1; i < Nd; ++i) {                                                   // :510-519
        const int pr = in.prev_kf[opt.back()];
        if (pr < 0) break;
        opt.push_back(pr);
        local_for[pr] = 1;
    }
    for (int k : opt)                                                                // :525-539
        for (int s = in.slot_offsets[k]; s < in.slot_offsets[k + 1]; ++s) {
            const int p = in.slot_point[s];
            if (p < 0 || (in.point_flags[p] & 1)) continue;                          // :531-532
            if (!point_mark[p]) { listed.push_back(p); point_mark[p] = 1; }          // :533-537
        }
    if (in.prev_kf[opt.back()] >= 0) {                                               // :543-547
        fixed_kfs.push_back(in.prev_kf[opt.back()]);
        fixed_for[in.prev_kf[opt.back()]] = 1;
    } else {                                                                         // :549-553
        local_for[opt.back()] = 0;
        fixed_for[opt.back()] = 1;
        fixed_kfs.push_back(opt.back());
        opt.pop_back();
    }
    const int N = (int)opt.size();                                                   // :633
    counts[TC2LI_INERTIAL_WINDOW_N_FIXED_KF] = 1;
    if (N == 0) {
        counts[TC2LI_INERTIAL_WINDOW_STATUS] = TC2LI_INERTIAL_WINDOW_EMPTY;
        return true;
    }
    for (int p : listed) {                                                           // :588-607
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            const int k = in.obs_kf[o];
            if (local_for[k] || fixed_for[k]) continue;                              // :595
            fixed_for[k] = 1;                                                        // :597
            if (!(in.kf_flags[k] & 1)) {                                             // :598
                fixed_kfs.push_back(k);
                break;
            }
        }
        if ((int)fixed_kfs.size() >= TC2LI_INERTIAL_WINDOW_MAX_FIXED) break;         // :605-606
    }
    // the vertices in id order (:632-696)
    std::vector<int32_t> order = opt;
    order.insert(order.end(), fixed_kfs.begin(), fixed_kfs.end());
    const std::vector<int32_t> vertex_of = vertices_by_id(in.kf_id, in.n_keyframes, &order);
    std::vector<uint8_t> is_fixed(in.n_keyframes, 0);
    for (int k : fixed_kfs) is_fixed[k] = 1;
    const int n_lidar = (in.with_lidar && N > 5) ? std::min(N, TC2LI_INERTIAL_WINDOW_MAX_LIDAR) : 0;   // :709-712
    auto linked = [&](int i) {                                                       // :738, :743
        const int k = opt[i], pr = in.prev_kf[k];
        return pr >= 0 && (in.kf_flags[k] & 4) && (in.kf_flags[pr] & 4) && (in.kf_flags[k] & 8);
    };
    int n_links = 0;
    for (int i = 0; i < N; ++i) n_links += linked(i) ? 1 : 0;
    auto edge_of = [&](int o) {                                                      // :862, :865, :872, :902
        const int k = in.obs_kf[o];
        return (local_for[k] || fixed_for[k]) && !(in.kf_flags[k] & 3) && in.obs_index[o] >= 0;
    };
    int n_edges = 0, n_without = 0, n_under3 = 0;
    for (int p : listed) {
        int ne = 0;
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o)
            if (edge_of(o)) { ++ne; ++vis_edges[in.obs_kf[o]]; }                     // :874, :905
        n_edges += ne;
        n_without += ne == 0;
    }
    for (int k : order) n_under3 += vis_edges[k] < 3;                       // :972-975
    counts[TC2LI_INERTIAL_WINDOW_N_FIXED_KF] = (int)fixed_kfs.size();
    counts[TC2LI_INERTIAL_WINDOW_N_OPT_KF] = N;
    counts[TC2LI_INERTIAL_WINDOW_N_VERTICES] = (int)order.size();
    counts[TC2LI_INERTIAL_WINDOW_N_POINTS] = (int)listed.size();
    counts[TC2LI_INERTIAL_WINDOW_N_EDGES] = n_edges;
    counts[TC2LI_INERTIAL_WINDOW_N_LINKS] = n_links;
    counts[TC2LI_INERTIAL_WINDOW_N_LIDAR] = n_lidar;
    counts[TC2LI_INERTIAL_WINDOW_N_POINTS_WITHOUT_EDGE] = n_without;
    counts[TC2LI_INERTIAL_WINDOW_N_VERTICES_UNDER_3_EDGES] = n_under3;
    if (!fits(in, counts)) return false;
    if (!write) return true;
    for (size_t r = 0; r < order.size(); ++r) {
        const int k = order[r];
        in.kf_row[r] = k;
        in.keyframes_out[r] = in.states[k];
        in.fixed[r] = is_fixed[k];                                                   // :640, :678
        in.has_imu[r] = (in.kf_flags[k] & 4) ? 1 : 0;                                // :643, :681
    }
    for (int i = 0; i < TC2LI_INERTIAL_WINDOW_MAX_LIDAR; ++i) in.lidar_pose_index[i] = i < n_lidar ? vertex_of[opt[i]] : -1;   // :715-721
    int l = 0;
    for (int i = 0; i < N; ++i) {                                                    // :734-800
        if (!linked(i)) continue;
        tc2li_inertial_link& L = in.links[l];
        L.kf1 = vertex_of[in.prev_kf[opt[i]]];                                       // :746
        L.kf2 = vertex_of[opt[i]];                                                   // :750
        L.robust = (i == N - 1 || in.rec_init) ? 1 : 0;                              // :770
        L.pad_ = 0;
        L.info_scale = i == N - 1 ? 1e-2 : 1.0;                                      // :778-779
        L.preintegrated = nullptr;
        in.link_kf2_row[l++] = opt[i];
    }
    emit_points_and_edges(in, views, inv_level_sigma2, listed, vertex_of, edge_of);  // :845-969
    return true;
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_inertial_window_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_inertial_window_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kWinLdsKeyframes; out[1] = kWinLdsPoints; out[2] = kWinThreads;
    return 3;
}

extern "C" int tc2li_inertial_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                                              const uint8_t* point_bad_now, const float* track_depth, int n_points, double initial_chi2,
                                              double final_chi2, int large, int32_t* rejected, int32_t* erase_pose, int32_t* erase_point,
                                              int capacity) {
    const char* entry = "tc2li_inertial_window_outliers";
    const int rc = outliers_check(entry, edges, edge_chi2, edge_depth_positive, n_edges, n_points, erase_pose, erase_point, capacity,
                                  !rejected || (n_points && (!point_bad_now || !track_depth)));
    if (rc < 0) return rc;
    const float err = (float)initial_chi2, err_end = (float)final_chi2;              // :979, :981
    *rejected = ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !large) ? 1 : 0;   // :1028
    if (*rejected) return 0;                                                         // :1031, before :1036-1045
    const float chi2Mono2 = 5.991f, chi2Stereo2 = 7.815f;                            // :828, :830
    const double mono_far = (double)chi2Mono2, mono_close = (double)(1.5f * chi2Mono2), stereo_th = (double)chi2Stereo2;
    // :990-1004 for the monocular edges, :1008-1021 for the stereo ones (erased: :1002, :1019)
    return outliers_emit(entry, edges, n_edges, erase_pose, erase_point, capacity, [&](int i, bool stereo) {
        if ((edges[i].u_right >= 0) != stereo || point_bad_now[edges[i].point]) return false;   // :996, :1013
        if (stereo) return edge_chi2[i] > stereo_th;                                            // :1016
        const bool close = track_depth[edges[i].point] < 10.f;                                  // :994
        return (edge_chi2[i] > mono_far && !close) || (edge_chi2[i] > mono_close && close) || !edge_depth_positive[i];   // :999
    });
}

extern "C" int tc2li_host_inertial_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_inertial_window_problem* problems,
                                                int n_problems, const float* inv_level_sigma2, int n_levels) {
    const char* entry = "tc2li_host_inertial_window_batch";
    return host_window_batch(
        entry, views, n_views, problems, n_problems, inv_level_sigma2, n_levels,
        [&](const tc2li_inertial_window_problem& in, const SlotTable& slots) { return validate(in, slots, n_levels); },
        [&](const tc2li_inertial_window_problem& in, bool write) { return window_one(in, views, inv_level_sigma2, write); },
        [&](int p) { return capacity_error(entry, problems, p); });
}

extern "C" int tc2li_inertial_window_batch(tc2li_keyframe_store* store, const tc2li_inertial_window_problem* problems, int n_problems,
                                           const float* inv_level_sigma2, int n_levels, void* stream) {
    const char* entry = "tc2li_inertial_window_batch";
    if (!store) {
        set_error("%s: null store", entry);
        return TC2LI_ERR_INVALID;
    }
    SlotTable slots;
    BawStore where{};
    slot_table_from_store(store, &slots, &where);
    const int rc = validate_all(entry, problems, n_problems, inv_level_sigma2, n_levels,
                                [&](const tc2li_inertial_window_problem& in) { return validate(in, slots, n_levels); });
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    constexpr int kMaxVertices = TC2LI_INERTIAL_WINDOW_MAX_OPT + TC2LI_INERTIAL_WINDOW_MAX_FIXED;
    constexpr size_t kState = sizeof(tc2li_inertial_keyframe), kLink = sizeof(tc2li_inertial_link);
    WindowTransfer<tc2li_inertial_window_problem, IwProblemDev> T(problems, n_problems);
    size_t n_vertex = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_window_problem& in = problems[p];
        IwProblemDev& d = T.add(p, in.edge_capacity);
        d.nd = window_nd(in); d.rec_init = in.rec_init ? 1 : 0; d.with_lidar = in.with_lidar ? 1 : 0;
        // the vertices are at most 25 + 200
        d.vertex_off = (int32_t)n_vertex; d.vertex_cap = std::min(std::min(in.kf_capacity, in.n_keyframes), kMaxVertices);
        d.link_cap = std::min(in.link_capacity, kIwMaxOpt);
        n_vertex += d.vertex_cap;
        if (T.most_rows(p) > kMaxRows) return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    T.take_inputs(n_levels);
    const size_t o_state = T.io.take(T.n_kf * kState), o_prev = T.io.take(T.n_kf * 4);
    T.take_outputs(TC2LI_INERTIAL_WINDOW_COUNTS);
    const size_t o_links = T.io.take(np * kIwMaxOpt * kLink), o_lrow = T.io.take(np * kIwMaxOpt * 4), o_kfout = T.io.take(n_vertex * kState),
                 o_krow = T.io.take(n_vertex * 4), o_fixed = T.io.take(n_vertex), o_imu = T.io.take(n_vertex);
    T.take_work();
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceInertialWindow>();   // its own, whatever the visual gather holds
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    TC2LI_HIP_CHECK(T.upload_tables(inv_level_sigma2, n_levels, st, [&](int, const tc2li_inertial_window_problem& in, const IwProblemDev& d) {
        T.io.put(o_state, d.kf_off, in.states, (size_t)in.n_keyframes, kState);
        T.io.put(o_prev, d.kf_off, in.prev_kf, (size_t)in.n_keyframes, 4);
    }));
    uint8_t* d = T.d_io;
    IwBatch B{};
    T.bind(B, where);
    B.prev_kf = (const int32_t*)(d + o_prev); B.states = (const double*)(d + o_state);
    B.counts = (int32_t*)(d + T.o_counts); B.lidar_pose_index = (int32_t*)(d + T.o_lidar); B.links = (tc2li_inertial_link*)(d + o_links);
    B.link_kf2_row = (int32_t*)(d + o_lrow); B.kf_row = (int32_t*)(d + o_krow); B.keyframes_out = (double*)(d + o_kfout); B.fixed = d + o_fixed;
    B.has_imu = d + o_imu;
    launch_inertial_window(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    const int short_of_room = T.copy_counts(fits);
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    T.copy_out([&](int p, const tc2li_inertial_window_problem& in, const IwProblemDev& D) {
        const size_t n_v = (size_t)in.counts[TC2LI_INERTIAL_WINDOW_N_VERTICES], n_l = (size_t)in.counts[TC2LI_INERTIAL_WINDOW_N_LINKS];
        T.io.get(in.kf_row, o_krow, D.vertex_off, n_v, 4); T.io.get(in.keyframes_out, o_kfout, D.vertex_off, n_v, kState);
        T.io.get(in.fixed, o_fixed, D.vertex_off, n_v, 1); T.io.get(in.has_imu, o_imu, D.vertex_off, n_v, 1);
        T.io.get(in.links, o_links, (size_t)p * kIwMaxOpt, n_l, kLink); T.io.get(in.link_kf2_row, o_lrow, (size_t)p * kIwMaxOpt, n_l, 4);
    });
    return n_problems;
}

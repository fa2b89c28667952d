// tc2li_inertial_window_batch / tc2li_host_inertial_window_batch / tc2li_inertial_window_limits / tc2li_inertial_window_outliers
// (include/tc2li_hip.h "local mapping: the window of the inertial local BA"): the gather of OptimizerWithLidar::LocalLVIBA
// (SF/src/OptimizerWithLidar.cc:489-607, :632-727, :729-800, :832-969; the same text in Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512
// and on) and its outlier rule (:985-1045) on a flat copy of the graph.  This file validates the problems and either walks them in plain C++
// with the reference's mark fields or concatenates them for inertial_window_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "inertial_window_device.hpp"

static_assert(sizeof(tc2li_ba_edge) == 40, "ABI layout");
static_assert(sizeof(tc2li_inertial_link) == 32, "ABI layout");
static_assert(sizeof(tc2li_inertial_keyframe) == 264, "ABI layout");
static_assert(sizeof(tc2li_inertial_window_problem) == 232, "ABI layout");

namespace tc2li {
namespace {

bool ascending(const int32_t* off, int n) {
    if (off[0] != 0) return false;
    for (int i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return false;
    return true;
}

// what the entries know of the keyframes behind kf_slot: keypoints (-1: an empty slot) and 1 + the highest octave held
struct SlotTable {
    std::vector<int32_t> n, levels;
};

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
    if (!ascending(in.slot_offsets, in.n_keyframes)) return "slot_offsets do not ascend from 0";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_slot = in.slot_offsets[in.n_keyframes], n_obs = in.obs_offsets[in.n_points];
    if ((n_slot && !in.slot_point) || (n_obs && (!in.obs_kf || !in.obs_index))) return "null slot_point, obs_kf or obs_index";
    const int n_store = (int)slots.n.size();
    for (int k = 0; k < in.n_keyframes; ++k) {
        const int s = in.kf_slot[k];
        if (s < 0 || s >= n_store || slots.n[s] < 0) return "a kf_slot is empty or out of range";
        if (slots.levels[s] > n_levels) return "a slot holds an octave outside [0, n_levels)";
        if (in.prev_kf[k] < -1 || in.prev_kf[k] >= in.n_keyframes) return "prev_kf out of range";
    }
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
    for (int i = 0; i < n_slot; ++i)
        if (in.slot_point[i] < -1 || in.slot_point[i] >= in.n_points) return "slot_point out of range";
    for (int p = 0; p < in.n_points; ++p)
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            const int k = in.obs_kf[o];
            if (k < 0 || k >= in.n_keyframes) return "obs_kf out of range";
            if (o > in.obs_offsets[p] && k <= in.obs_kf[o - 1]) return "an observation row does not ascend strictly by keyframe";
            if (in.obs_index[o] < -1 || in.obs_index[o] >= slots.n[in.kf_slot[k]]) return "obs_index outside the keypoints of the observer's slot";
        }
    return "";
}

int validate_all(const char* entry, const tc2li_inertial_window_problem* problems, int n_problems, const SlotTable& slots,
                 const float* inv_level_sigma2, int n_levels) {
    if (n_problems < 0 || (n_problems && !problems) || !inv_level_sigma2 || n_levels < 1) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    std::vector<const char*> what(n_problems, "");
    tracking_pool().parallel_for(n_problems, [&](int p) { what[p] = validate(problems[p], slots, n_levels); });
    for (int p = 0; p < n_problems; ++p)
        if (what[p][0]) {
            set_error("%s: problem %d: %s", entry, p, what[p]);
            return TC2LI_ERR_INVALID;
        }
    return 0;
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
    std::vector<std::pair<int64_t, int32_t>> order;
    for (int k : opt) order.push_back({in.kf_id[k], k});
    for (int k : fixed_kfs) order.push_back({in.kf_id[k], k});
    std::sort(order.begin(), order.end());
    std::vector<int32_t> vertex_of(in.n_keyframes, -1);
    std::vector<uint8_t> is_fixed(in.n_keyframes, 0);
    for (size_t r = 0; r < order.size(); ++r) vertex_of[order[r].second] = (int32_t)r;
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
    for (auto& v : order) n_under3 += vis_edges[v.second] < 3;                       // :972-975
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
        const int k = order[r].second;
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
    int e = 0;
    for (size_t i = 0; i < listed.size(); ++i) {                                     // :845-969
        const int p = listed[i];
        in.point_row[i] = p;
        memcpy(in.points3_out + 3 * i, in.positions + 3 * (size_t)p, 3 * sizeof(double));   // :849
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            if (!edge_of(o)) continue;
            const int k = in.obs_kf[o], idx = in.obs_index[o];
            const tc2li_keyframe_view& v = views[in.kf_slot[k]];
            const tc2li_keypoint& kp = v.keys[idx];
            const float ur = v.u_right[idx];
            tc2li_ba_edge& E = in.edges[e++];
            E.point = (int32_t)i;
            E.pose = vertex_of[k];
            E.u = (double)kp.x;
            E.v = (double)kp.y;
            E.u_right = ur >= 0.f ? (double)ur : -1.0;
            E.inv_sigma2 = (double)inv_level_sigma2[kp.octave];
        }
    }
    return true;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the device buffers of a call, kept between calls
struct IwSpace {
    std::mutex mu;
    DevBuf<uint8_t> io, work;
    PinnedBuf<uint8_t> h_io;
};

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_inertial_window_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_inertial_window_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kIwLdsKeyframes; out[1] = kIwLdsPoints; out[2] = kIwThreads;
    return 3;
}

extern "C" int tc2li_inertial_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                                              const uint8_t* point_bad_now, const float* track_depth, int n_points, double initial_chi2,
                                              double final_chi2, int large, int32_t* rejected, int32_t* erase_pose, int32_t* erase_point,
                                              int capacity) {
    const char* entry = "tc2li_inertial_window_outliers";
    if (n_edges < 0 || n_points < 0 || capacity < 0 || !rejected || (n_edges && (!edges || !edge_chi2 || !edge_depth_positive)) ||
        (n_points && (!point_bad_now || !track_depth)) || (capacity && (!erase_pose || !erase_point))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    for (int i = 0; i < n_edges; ++i)
        if (edges[i].point < 0 || edges[i].point >= n_points) {
            set_error("%s: edge %d names point %d of %d", entry, i, edges[i].point, n_points);
            return TC2LI_ERR_INVALID;
        }
    const float err = (float)initial_chi2, err_end = (float)final_chi2;              // :979, :981
    *rejected = ((2 * err < err_end || std::isnan(err) || std::isnan(err_end)) && !large) ? 1 : 0;   // :1028
    if (*rejected) return 0;                                                         // :1031, before :1036-1045
    const float chi2Mono2 = 5.991f, chi2Stereo2 = 7.815f;                            // :828, :830
    const double mono_far = (double)chi2Mono2, mono_close = (double)(1.5f * chi2Mono2), stereo_th = (double)chi2Stereo2;
    // vpEdgesMono first (:990-1004), then vpEdgesStereo (:1008-1021), each in creation order
    auto erased = [&](int i, bool stereo) {
        if ((edges[i].u_right >= 0) != stereo || point_bad_now[edges[i].point]) return false;   // :996, :1013
        if (stereo) return edge_chi2[i] > stereo_th;                                            // :1016
        const bool close = track_depth[edges[i].point] < 10.f;                                  // :994
        return (edge_chi2[i] > mono_far && !close) || (edge_chi2[i] > mono_close && close) || !edge_depth_positive[i];   // :999
    };
    int n = 0;
    for (int stereo = 0; stereo < 2; ++stereo)
        for (int i = 0; i < n_edges; ++i) n += erased(i, stereo != 0) ? 1 : 0;
    if (n > capacity) {
        set_error("%s: %d pairs, room for %d", entry, n, capacity);
        return TC2LI_ERR_CAPACITY;
    }
    n = 0;
    for (int stereo = 0; stereo < 2; ++stereo)
        for (int i = 0; i < n_edges; ++i)
            if (erased(i, stereo != 0)) { erase_pose[n] = edges[i].pose; erase_point[n++] = edges[i].point; }   // :1002, :1019
    return n;
}

extern "C" int tc2li_host_inertial_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_inertial_window_problem* problems,
                                                int n_problems, const float* inv_level_sigma2, int n_levels) {
    const char* entry = "tc2li_host_inertial_window_batch";
    if (n_views < 0 || (n_views && !views)) {
        set_error("%s: null or negative views", entry);
        return TC2LI_ERR_INVALID;
    }
    SlotTable slots;
    slots.n.assign(n_views, -1);
    slots.levels.assign(n_views, 0);
    std::vector<uint8_t> broken(n_views, 0);
    tracking_pool().parallel_for(n_views, [&](int s) {
        const tc2li_keyframe_view& v = views[s];
        if (v.n < 0) return;
        if (v.n > 0 && (!v.keys || !v.u_right)) { broken[s] = 1; return; }
        slots.n[s] = v.n;
        int top = 0;
        for (int i = 0; i < v.n; ++i) {
            if (v.keys[i].octave < 0) { broken[s] = 1; return; }
            top = std::max(top, v.keys[i].octave + 1);
        }
        slots.levels[s] = top;
    });
    for (int s = 0; s < n_views; ++s)
        if (broken[s]) {
            set_error("%s: view %d has null keys or u_right, or a negative octave", entry, s);
            return TC2LI_ERR_INVALID;
        }
    const int rc = validate_all(entry, problems, n_problems, slots, inv_level_sigma2, n_levels);
    if (rc < 0) return rc;
    // sizes first: on TC2LI_ERR_CAPACITY no list of any problem is written
    std::vector<uint8_t> ok(n_problems, 1);
    tracking_pool().parallel_for(n_problems, [&](int p) { ok[p] = window_one(problems[p], views, inv_level_sigma2, false); });
    for (int p = 0; p < n_problems; ++p)
        if (!ok[p]) return capacity_error(entry, problems, p);
    tracking_pool().parallel_for(n_problems, [&](int p) { window_one(problems[p], views, inv_level_sigma2, true); });
    return n_problems;
}

extern "C" int tc2li_inertial_window_batch(tc2li_keyframe_store* store, const tc2li_inertial_window_problem* problems, int n_problems,
                                           const float* inv_level_sigma2, int n_levels, void* stream) {
    const char* entry = "tc2li_inertial_window_batch";
    if (!store) {
        set_error("%s: null store", entry);
        return TC2LI_ERR_INVALID;
    }
    SlotTable slots;
    const int n_store = keyframe_store_slots(store);
    slots.n.assign(n_store, -1);
    slots.levels.assign(n_store, 0);
    BawStore where{};
    keyframe_store_baw(store, &where, slots.n.data(), slots.levels.data(), n_store);
    const int rc = validate_all(entry, problems, n_problems, slots, inv_level_sigma2, n_levels);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // where every problem's tables start in the concatenation
    constexpr int kMaxVertices = TC2LI_INERTIAL_WINDOW_MAX_OPT + TC2LI_INERTIAL_WINDOW_MAX_FIXED;
    constexpr size_t kState = sizeof(tc2li_inertial_keyframe);
    std::vector<IwProblemDev> dev(n_problems);
    size_t n_kf = 0, n_slot = 0, n_points = 0, n_obs = 0, n_marks = 0, n_first = 0, n_vertex = 0, n_pointo = 0, n_edge = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_window_problem& in = problems[p];
        IwProblemDev& d = dev[p];
        const int slot_entries = in.slot_offsets[in.n_keyframes], obs_entries = in.obs_offsets[in.n_points];
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.slot_off = (int32_t)n_slot;
        d.point_off = (int32_t)n_points; d.n_points = in.n_points; d.obs_off = (int32_t)n_obs;
        d.current = in.current; d.nd = window_nd(in); d.rec_init = in.rec_init ? 1 : 0; d.with_lidar = in.with_lidar ? 1 : 0;
        d.mark_off = in.n_keyframes > kIwLdsKeyframes ? (int32_t)n_marks : -1;
        d.first_off = in.n_points > kIwLdsPoints ? (int32_t)n_first : -1;
        // no list is longer than its table, and the vertices are at most 25 + 200: the device arrays need no more room, whatever the caller offers
        d.vertex_off = (int32_t)n_vertex; d.vertex_cap = std::min(std::min(in.kf_capacity, in.n_keyframes), kMaxVertices);
        d.pointo_off = (int32_t)n_pointo; d.point_cap = std::min(in.point_capacity, in.n_points);
        d.edge_off = (int32_t)n_edge; d.edge_cap = std::min(in.edge_capacity, obs_entries);
        d.link_cap = std::min(in.link_capacity, kIwMaxOpt); d.pad_ = 0;
        n_kf += in.n_keyframes; n_slot += slot_entries; n_points += in.n_points; n_obs += obs_entries;
        if (d.mark_off >= 0) n_marks += in.n_keyframes;
        if (d.first_off >= 0) n_first += in.n_points;
        n_vertex += d.vertex_cap; n_pointo += d.point_cap; n_edge += d.edge_cap;
        if (std::max(std::max(n_kf + p, n_slot), std::max(n_points + p, n_obs)) > 0x7fffff00u) {
            set_error("%s: the batch up to problem %d has more than 2^31 rows in one table; split it", entry, p);
            return TC2LI_ERR_INVALID;
        }
    }
    const size_t np = (size_t)n_problems;
    // one buffer: [inputs | outputs]; the upload is the first part, the download the second
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_prob = take(np * sizeof(IwProblemDev)), o_sigma = take((size_t)n_levels * 4), o_id = take(n_kf * 8), o_state = take(n_kf * kState),
                 o_pos = take(n_points * 24), o_slot = take(n_kf * 4), o_prev = take(n_kf * 4), o_srow = take((n_kf + np) * 4), o_spt = take(n_slot * 4),
                 o_orow = take((n_points + np) * 4), o_okf = take(n_obs * 4), o_oidx = take(n_obs * 4), o_flags = take(n_kf), o_pflags = take(n_points);
    const size_t up_bytes = off, down_from = off;
    const size_t o_counts = take(np * TC2LI_INERTIAL_WINDOW_COUNTS * 4), o_lidar = take(np * TC2LI_INERTIAL_WINDOW_MAX_LIDAR * 4),
                 o_links = take(np * kIwMaxOpt * sizeof(tc2li_inertial_link)), o_lrow = take(np * kIwMaxOpt * 4), o_kfout = take(n_vertex * kState),
                 o_p3 = take(n_pointo * 24), o_edges = take(n_edge * sizeof(tc2li_ba_edge)), o_krow = take(n_vertex * 4), o_ptrow = take(n_pointo * 4),
                 o_fixed = take(n_vertex), o_imu = take(n_vertex);
    const size_t io_bytes = off;
    off = 0;
    const size_t w_marks = take(n_marks * 4), w_first = take(n_first * 4), w_vertex = take(n_kf * 4), w_members = take(n_kf * 4),
                 w_listed = take(n_points * 4), w_estart = take(n_points * 4);
    const size_t work_bytes = off;
    IwSpace& S = shutdown_owned<IwSpace>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(S.io.ensure(io_bytes));
    TC2LI_HIP_CHECK(S.work.ensure(std::max(work_bytes, (size_t)256)));
    TC2LI_HIP_CHECK(S.h_io.ensure(io_bytes));
    uint8_t* h = S.h_io.p;
    memcpy(h + o_prob, dev.data(), np * sizeof(IwProblemDev));
    memcpy(h + o_sigma, inv_level_sigma2, (size_t)n_levels * 4);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_inertial_window_problem& in = problems[p];
        const IwProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        auto put = [h](size_t o, size_t start, const void* src, size_t count, size_t width) {
            if (count) memcpy(h + o + start * width, src, count * width);
        };
        put(o_id, d.kf_off, in.kf_id, nk, 8); put(o_state, d.kf_off, in.states, nk, kState); put(o_slot, d.kf_off, in.kf_slot, nk, 4);
        put(o_prev, d.kf_off, in.prev_kf, nk, 4); put(o_flags, d.kf_off, in.kf_flags, nk, 1);
        put(o_srow, (size_t)d.kf_off + p, in.slot_offsets, nk + 1, 4);
        put(o_spt, d.slot_off, in.slot_point, (size_t)in.slot_offsets[in.n_keyframes], 4);
        put(o_pflags, d.point_off, in.point_flags, npt, 1); put(o_pos, d.point_off, in.positions, npt, 24);
        put(o_orow, (size_t)d.point_off + p, in.obs_offsets, npt + 1, 4);
        put(o_okf, d.obs_off, in.obs_kf, (size_t)in.obs_offsets[in.n_points], 4);
        put(o_oidx, d.obs_off, in.obs_index, (size_t)in.obs_offsets[in.n_points], 4);
    });
    TC2LI_HIP_CHECK(hipMemcpyAsync(S.io.p, h, up_bytes, hipMemcpyHostToDevice, st));
    uint8_t* d = S.io.p;
    uint8_t* w = S.work.p;
    IwBatch B{};
    B.n_problems = n_problems;
    B.problems = (const IwProblemDev*)(d + o_prob); B.store = where; B.inv_level_sigma2 = (const float*)(d + o_sigma);
    B.kf_slot = (const int32_t*)(d + o_slot); B.kf_id = (const int64_t*)(d + o_id); B.kf_flags = d + o_flags; B.prev_kf = (const int32_t*)(d + o_prev);
    B.states = (const double*)(d + o_state); B.slot_offsets = (const int32_t*)(d + o_srow); B.slot_point = (const int32_t*)(d + o_spt);
    B.point_flags = d + o_pflags; B.positions = (const double*)(d + o_pos); B.obs_offsets = (const int32_t*)(d + o_orow);
    B.obs_kf = (const int32_t*)(d + o_okf); B.obs_index = (const int32_t*)(d + o_oidx);
    B.marks_global = (int32_t*)(w + w_marks); B.first_global = (int32_t*)(w + w_first); B.kf_vertex = (int32_t*)(w + w_vertex);
    B.members = (int32_t*)(w + w_members); B.listed = (int32_t*)(w + w_listed); B.edge_start = (int32_t*)(w + w_estart);
    B.counts = (int32_t*)(d + o_counts); B.lidar_pose_index = (int32_t*)(d + o_lidar); B.links = (tc2li_inertial_link*)(d + o_links);
    B.link_kf2_row = (int32_t*)(d + o_lrow); B.kf_row = (int32_t*)(d + o_krow); B.keyframes_out = (double*)(d + o_kfout); B.fixed = d + o_fixed;
    B.has_imu = d + o_imu; B.point_row = (int32_t*)(d + o_ptrow); B.points3_out = (double*)(d + o_p3); B.edges = (tc2li_ba_edge*)(d + o_edges);
    launch_inertial_window(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(h + down_from, d + down_from, io_bytes - down_from, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    int short_of_room = -1;
    for (int p = 0; p < n_problems; ++p) {
        const int32_t* counts = (const int32_t*)(h + o_counts) + (size_t)p * TC2LI_INERTIAL_WINDOW_COUNTS;
        memcpy(problems[p].counts, counts, TC2LI_INERTIAL_WINDOW_COUNTS * 4);
        if (short_of_room < 0 && !fits(problems[p], counts)) short_of_room = p;
    }
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_inertial_window_problem& in = problems[p];
        const IwProblemDev& D = dev[p];
        const int32_t* counts = in.counts;
        auto get = [h](void* dst, size_t o, size_t start, size_t count, size_t width) {
            if (count) memcpy(dst, h + o + start * width, count * width);
        };
        if (counts[TC2LI_INERTIAL_WINDOW_STATUS] != TC2LI_INERTIAL_WINDOW_OK) return;
        get(in.lidar_pose_index, o_lidar, (size_t)p * TC2LI_INERTIAL_WINDOW_MAX_LIDAR, TC2LI_INERTIAL_WINDOW_MAX_LIDAR, 4);
        const size_t n_v = (size_t)counts[TC2LI_INERTIAL_WINDOW_N_VERTICES], n_pt = (size_t)counts[TC2LI_INERTIAL_WINDOW_N_POINTS],
                     n_l = (size_t)counts[TC2LI_INERTIAL_WINDOW_N_LINKS];
        get(in.kf_row, o_krow, D.vertex_off, n_v, 4); get(in.keyframes_out, o_kfout, D.vertex_off, n_v, kState);
        get(in.fixed, o_fixed, D.vertex_off, n_v, 1); get(in.has_imu, o_imu, D.vertex_off, n_v, 1);
        get(in.point_row, o_ptrow, D.pointo_off, n_pt, 4); get(in.points3_out, o_p3, D.pointo_off, n_pt, 24);
        get(in.edges, o_edges, D.edge_off, (size_t)counts[TC2LI_INERTIAL_WINDOW_N_EDGES], sizeof(tc2li_ba_edge));
        get(in.links, o_links, (size_t)p * kIwMaxOpt, n_l, sizeof(tc2li_inertial_link));
        get(in.link_kf2_row, o_lrow, (size_t)p * kIwMaxOpt, n_l, 4);
    });
    return n_problems;
}

// tc2li_ba_window_batch / tc2li_host_ba_window_batch / tc2li_ba_window_limits / tc2li_ba_window_outliers (include/tc2li_hip.h "local
// mapping: the window of the local BA"): the gather of OptimizerWithLidar::LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:63-130,
// :157-187, :226-253, :263-384) and its outlier rule (:402-449) on a flat copy of the graph.  This file validates the problems and either
// walks them in plain C++ with the reference's mark fields or concatenates them for ba_window_kernels.hip.  ba_window_batch_run is the
// device entry with two hooks for what follows the gather on the device (ba_structure_device.hpp: the structure kernels, the BA).
#include <algorithm>
#include <cstring>

#include "ba_structure_device.hpp"
#include "ba_window_device.hpp"
#include "common.hpp"

static_assert(sizeof(tc2li_ba_edge) == 40, "ABI layout");
static_assert(sizeof(tc2li_keypoint) == 24, "ABI layout");

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
    if (!ascending(in.slot_offsets, in.n_keyframes)) return "slot_offsets do not ascend from 0";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_slot = in.slot_offsets[in.n_keyframes], n_obs = in.obs_offsets[in.n_points];
    if ((n_slot && !in.slot_point) || (n_obs && (!in.obs_kf || !in.obs_index))) return "null slot_point, obs_kf or obs_index";
    const int n_store = (int)slots.n.size();
    for (int k = 0; k < in.n_keyframes; ++k) {
        const int s = in.kf_slot[k];
        if (s < 0 || s >= n_store || slots.n[s] < 0) return "a kf_slot is empty or out of range";
        if (slots.levels[s] > n_levels) return "a slot holds an octave outside [0, n_levels)";
    }
    std::vector<uint8_t> named(in.n_keyframes, 0);
    named[in.current] = 1;
    for (int i = 0; i < in.n_cov; ++i) {
        const int k = in.cov_kf[i];
        if (k < 0 || k >= in.n_keyframes) return "cov_kf out of range";
        if (named[k]) return "cov_kf names a row twice or the current keyframe";
        named[k] = 1;
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

int validate_all(const char* entry, const tc2li_ba_window_problem* problems, int n_problems, const SlotTable& slots, const float* inv_level_sigma2,
                 int n_levels, bool edges_optional = false) {
    if (n_problems < 0 || (n_problems && !problems) || !inv_level_sigma2 || n_levels < 1) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    std::vector<const char*> what(n_problems, "");
    tracking_pool().parallel_for(n_problems, [&](int p) { what[p] = validate(problems[p], slots, n_levels, edges_optional); });
    for (int p = 0; p < n_problems; ++p)
        if (what[p][0]) {
            set_error("%s: problem %d: %s", entry, p, what[p]);
            return TC2LI_ERR_INVALID;
        }
    return 0;
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
    std::vector<std::pair<int64_t, int32_t>> order;
    for (int k : local) order.push_back({in.kf_id[k], k});
    for (int k : fixed_cams) order.push_back({in.kf_id[k], k});
    std::sort(order.begin(), order.end());
    std::vector<int32_t> pose_of(in.n_keyframes, -1);
    for (size_t r = 0; r < order.size(); ++r) pose_of[order[r].second] = (int32_t)r;
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
        const int k = order[r].second;
        in.pose_row[r] = k;
        memcpy(in.poses7_out + 7 * r, in.poses7 + 7 * (size_t)k, 7 * sizeof(double));
        in.fixed[r] = ((kf_mark[k] & kFixedFor) || in.kf_id[k] == in.init_kf_id) ? 1 : 0;   // :181, :164
    }
    for (int i = 0; i < TC2LI_BA_WINDOW_MAX_LIDAR; ++i) in.lidar_pose_index[i] = i < n_lidar ? pose_of[clouds[i]] : -1;   // :247-253
    int e = 0;
    for (size_t i = 0; i < listed.size(); ++i) {                                     // :263-384
        const int p = listed[i];
        in.point_row[i] = p;
        memcpy(in.points3_out + 3 * i, in.positions + 3 * (size_t)p, 3 * sizeof(double));   // :267
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            const int k = in.obs_kf[o], idx = in.obs_index[o];
            if (other(k) || idx < 0) continue;                                       // :281, :286, :313
            const tc2li_keyframe_view& v = views[in.kf_slot[k]];
            const tc2li_keypoint& kp = v.keys[idx];
            const float ur = v.u_right[idx];
            tc2li_ba_edge& E = in.edges[e++];
            E.point = (int32_t)i;
            E.pose = pose_of[k];
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
struct BawSpace {
    std::mutex mu;
    DevBuf<uint8_t> io, work;
    PinnedBuf<uint8_t> h_io;
};
// [0]: tc2li_ba_window_batch's; [1 + group]: a follow-up's that keeps the buffers for the length of a BA on the lock-step context `group`
struct BawSpaces { BawSpace s[1 + kMaxLockstepGroups]; };

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_ba_window_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_ba_window_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kBawLdsKeyframes; out[1] = kBawLdsPoints; out[2] = kBawThreads;
    return 3;
}

extern "C" int tc2li_ba_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                                        const uint8_t* point_bad_now, int n_points, int32_t* erase_pose, int32_t* erase_point, int capacity) {
    const char* entry = "tc2li_ba_window_outliers";
    if (n_edges < 0 || n_points < 0 || capacity < 0 || (n_edges && (!edges || !edge_chi2 || !edge_depth_positive)) || (n_points && !point_bad_now) ||
        (capacity && (!erase_pose || !erase_point))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    for (int i = 0; i < n_edges; ++i)
        if (edges[i].point < 0 || edges[i].point >= n_points) {
            set_error("%s: edge %d names point %d of %d", entry, i, edges[i].point, n_points);
            return TC2LI_ERR_INVALID;
        }
    // vpEdgesMono first (:406-419), then vpEdgesStereo (:436-449), each in creation order
    auto erased = [&](int i, bool stereo) {
        if ((edges[i].u_right >= 0) != stereo || point_bad_now[edges[i].point]) return false;   // :411, :441
        return edge_chi2[i] > (stereo ? 7.815 : 5.991) || !edge_depth_positive[i];              // :414, :444
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
            if (erased(i, stereo != 0)) { erase_pose[n] = edges[i].pose; erase_point[n++] = edges[i].point; }   // :417, :447
    return n;
}

extern "C" int tc2li_host_ba_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_ba_window_problem* problems, int n_problems,
                                          const float* inv_level_sigma2, int n_levels) {
    const char* entry = "tc2li_host_ba_window_batch";
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

extern "C" int tc2li_ba_window_batch(tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                                     const float* inv_level_sigma2, int n_levels, void* stream) {
    return ba_window_batch_run("tc2li_ba_window_batch", store, problems, n_problems, inv_level_sigma2, n_levels, stream, nullptr, 0, false);
}

int tc2li::ba_window_batch_run(const char* entry, tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                               const float* inv_level_sigma2, int n_levels, void* stream, BawFollow* follow, int space, bool edges_optional) {
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
    if (space < 0 || space > kMaxLockstepGroups) { set_error("%s: no such buffer set", entry); return TC2LI_ERR_INVALID; }
    const int rc = validate_all(entry, problems, n_problems, slots, inv_level_sigma2, n_levels, edges_optional);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // where every problem's tables start in the concatenation
    std::vector<BawProblemDev> dev(n_problems);
    size_t n_kf = 0, n_slot = 0, n_cov = 0, n_points = 0, n_obs = 0, n_marks = 0, n_first = 0, n_pose = 0, n_pointo = 0, n_edge = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_ba_window_problem& in = problems[p];
        BawProblemDev& d = dev[p];
        const int slot_entries = in.slot_offsets[in.n_keyframes], obs_entries = in.obs_offsets[in.n_points];
        d.init_kf_id = in.init_kf_id;
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.slot_off = (int32_t)n_slot;
        d.cov_off = (int32_t)n_cov; d.n_cov = in.n_cov;
        d.point_off = (int32_t)n_points; d.n_points = in.n_points; d.obs_off = (int32_t)n_obs;
        d.current = in.current;
        d.mark_off = in.n_keyframes > kBawLdsKeyframes ? (int32_t)n_marks : -1;
        d.first_off = in.n_points > kBawLdsPoints ? (int32_t)n_first : -1;
        // no list is longer than its table: the device arrays need no more room than that, whatever the caller offers
        d.pose_off = (int32_t)n_pose; d.pose_cap = std::min(in.pose_capacity, in.n_keyframes);
        d.pointo_off = (int32_t)n_pointo; d.point_cap = std::min(in.point_capacity, in.n_points);
        d.edge_off = (int32_t)n_edge; d.edge_cap = edges_optional && !in.edges ? obs_entries : std::min(in.edge_capacity, obs_entries);
        n_kf += in.n_keyframes; n_slot += slot_entries; n_cov += in.n_cov; n_points += in.n_points; n_obs += obs_entries;
        if (d.mark_off >= 0) n_marks += in.n_keyframes;
        if (d.first_off >= 0) n_first += in.n_points;
        n_pose += d.pose_cap; n_pointo += d.point_cap; n_edge += d.edge_cap;
        if (std::max(std::max(n_kf + p, n_slot), std::max(std::max(n_cov + 2 * (size_t)p, n_points + p), n_obs)) > 0x7fffff00u) {
            set_error("%s: the batch up to problem %d has more than 2^31 rows in one table; split it", entry, p);
            return TC2LI_ERR_INVALID;
        }
    }
    const size_t np = (size_t)n_problems;
    // one buffer: [inputs | outputs]; the upload is the first part, the download the second
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_prob = take(np * sizeof(BawProblemDev)), o_sigma = take((size_t)n_levels * 4), o_id = take(n_kf * 8), o_pose = take(n_kf * 56),
                 o_pos = take(n_points * 24), o_slot = take(n_kf * 4), o_srow = take((n_kf + np) * 4), o_spt = take(n_slot * 4), o_cov = take(n_cov * 4),
                 o_orow = take((n_points + np) * 4), o_okf = take(n_obs * 4), o_oidx = take(n_obs * 4), o_flags = take(n_kf), o_pflags = take(n_points);
    const size_t up_bytes = off, down_from = off;
    const size_t o_counts = take(np * TC2LI_BA_WINDOW_COUNTS * 4), o_lidar = take(np * TC2LI_BA_WINDOW_MAX_LIDAR * 4), o_p7 = take(n_pose * 56),
                 o_p3 = take(n_pointo * 24), o_edges = take(n_edge * sizeof(tc2li_ba_edge)), o_prow = take(n_pose * 4), o_ptrow = take(n_pointo * 4),
                 o_fixed = take(n_pose);
    const size_t io_bytes = off;
    off = 0;
    const size_t w_marks = take(n_marks * 4), w_first = take(n_first * 4), w_kfpose = take(n_kf * 4), w_members = take(n_kf * 4),
                 w_lkf = take((n_cov + 2 * np) * 4), w_lstart = take((n_cov + 2 * np) * 4), w_listed = take(n_points * 4), w_estart = take(n_points * 4);
    const size_t work_bytes = off;
    BawSpace& S = shutdown_owned<BawSpaces>().s[space];
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(S.io.ensure(io_bytes));
    TC2LI_HIP_CHECK(S.work.ensure(std::max(work_bytes, (size_t)256)));
    TC2LI_HIP_CHECK(S.h_io.ensure(io_bytes));
    uint8_t* h = S.h_io.p;
    memcpy(h + o_prob, dev.data(), np * sizeof(BawProblemDev));
    memcpy(h + o_sigma, inv_level_sigma2, (size_t)n_levels * 4);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_ba_window_problem& in = problems[p];
        const BawProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        auto put = [h](size_t o, size_t start, const void* src, size_t count, size_t width) {
            if (count) memcpy(h + o + start * width, src, count * width);
        };
        put(o_id, d.kf_off, in.kf_id, nk, 8); put(o_pose, d.kf_off, in.poses7, nk, 56); put(o_slot, d.kf_off, in.kf_slot, nk, 4);
        put(o_flags, d.kf_off, in.kf_flags, nk, 1);
        put(o_srow, (size_t)d.kf_off + p, in.slot_offsets, nk + 1, 4);
        put(o_spt, d.slot_off, in.slot_point, (size_t)in.slot_offsets[in.n_keyframes], 4);
        put(o_cov, d.cov_off, in.cov_kf, (size_t)in.n_cov, 4);
        put(o_pflags, d.point_off, in.point_flags, npt, 1); put(o_pos, d.point_off, in.positions, npt, 24);
        put(o_orow, (size_t)d.point_off + p, in.obs_offsets, npt + 1, 4);
        put(o_okf, d.obs_off, in.obs_kf, (size_t)in.obs_offsets[in.n_points], 4);
        put(o_oidx, d.obs_off, in.obs_index, (size_t)in.obs_offsets[in.n_points], 4);
    });
    TC2LI_HIP_CHECK(hipMemcpyAsync(S.io.p, h, up_bytes, hipMemcpyHostToDevice, st));
    uint8_t* d = S.io.p;
    uint8_t* w = S.work.p;
    BawBatch B{};
    B.n_problems = n_problems;
    B.problems = (const BawProblemDev*)(d + o_prob); B.store = where; B.inv_level_sigma2 = (const float*)(d + o_sigma);
    B.kf_slot = (const int32_t*)(d + o_slot); B.kf_id = (const int64_t*)(d + o_id); B.kf_flags = d + o_flags; B.poses7 = (const double*)(d + o_pose);
    B.slot_offsets = (const int32_t*)(d + o_srow); B.slot_point = (const int32_t*)(d + o_spt); B.cov_kf = (const int32_t*)(d + o_cov);
    B.point_flags = d + o_pflags; B.positions = (const double*)(d + o_pos); B.obs_offsets = (const int32_t*)(d + o_orow);
    B.obs_kf = (const int32_t*)(d + o_okf); B.obs_index = (const int32_t*)(d + o_oidx);
    B.marks_global = (int32_t*)(w + w_marks); B.first_global = (int32_t*)(w + w_first); B.kf_pose = (int32_t*)(w + w_kfpose);
    B.members = (int32_t*)(w + w_members); B.list_kf = (int32_t*)(w + w_lkf); B.list_start = (int32_t*)(w + w_lstart);
    B.listed = (int32_t*)(w + w_listed); B.edge_start = (int32_t*)(w + w_estart);
    B.counts = (int32_t*)(d + o_counts); B.lidar_pose_index = (int32_t*)(d + o_lidar); B.pose_row = (int32_t*)(d + o_prow);
    B.poses7_out = (double*)(d + o_p7); B.fixed = d + o_fixed; B.point_row = (int32_t*)(d + o_ptrow); B.points3_out = (double*)(d + o_p3);
    B.edges = (tc2li_ba_edge*)(d + o_edges);
    launch_ba_window(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    if (follow) {
        const int frc = follow->after_gather(B, dev.data(), st);
        if (frc < 0) { (void)stream_wait_blocking(st); return frc; }
    }
    bool edges_wanted = !edges_optional;
    for (int p = 0; p < n_problems && !edges_wanted; ++p) edges_wanted = problems[p].edges != nullptr;
    if (edges_wanted) TC2LI_HIP_CHECK(hipMemcpyAsync(h + down_from, d + down_from, io_bytes - down_from, hipMemcpyDeviceToHost, st));
    else {   // the edges -- five sevenths of the result -- stay where they are
        TC2LI_HIP_CHECK(hipMemcpyAsync(h + down_from, d + down_from, o_edges - down_from, hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(hipMemcpyAsync(h + o_prow, d + o_prow, io_bytes - o_prow, hipMemcpyDeviceToHost, st));
    }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    int short_of_room = -1;
    for (int p = 0; p < n_problems; ++p) {
        const int32_t* counts = (const int32_t*)(h + o_counts) + (size_t)p * TC2LI_BA_WINDOW_COUNTS;
        memcpy(problems[p].counts, counts, TC2LI_BA_WINDOW_COUNTS * 4);
        if (short_of_room < 0 && !fits(problems[p], counts, edges_optional)) short_of_room = p;
    }
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    if (follow) {
        const int frc = follow->after_counts();
        if (frc < 0) return frc;
    }
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_ba_window_problem& in = problems[p];
        const BawProblemDev& D = dev[p];
        const int32_t* counts = in.counts;
        auto get = [h](void* dst, size_t o, size_t start, size_t count, size_t width) {
            if (count) memcpy(dst, h + o + start * width, count * width);
        };
        if (counts[TC2LI_BA_WINDOW_STATUS] != TC2LI_BA_WINDOW_OK) return;
        get(in.lidar_pose_index, o_lidar, (size_t)p * TC2LI_BA_WINDOW_MAX_LIDAR, TC2LI_BA_WINDOW_MAX_LIDAR, 4);
        const size_t n_po = (size_t)counts[TC2LI_BA_WINDOW_N_POSES], n_pt = (size_t)counts[TC2LI_BA_WINDOW_N_POINTS];
        get(in.pose_row, o_prow, D.pose_off, n_po, 4); get(in.poses7_out, o_p7, D.pose_off, n_po, 56); get(in.fixed, o_fixed, D.pose_off, n_po, 1);
        get(in.point_row, o_ptrow, D.pointo_off, n_pt, 4); get(in.points3_out, o_p3, D.pointo_off, n_pt, 24);
        if (in.edges) get(in.edges, o_edges, D.edge_off, (size_t)counts[TC2LI_BA_WINDOW_N_EDGES], sizeof(tc2li_ba_edge));
    });
    if (follow) {
        const int frc = follow->after_download(B, dev.data(), st);
        if (frc < 0) return frc;
    }
    return n_problems;
}

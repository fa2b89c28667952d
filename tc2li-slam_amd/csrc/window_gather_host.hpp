// What the two gathers of a local-BA window share on the host (ba_window_host.cpp, inertial_window_host.cpp; the device side of the same
// split is window_gather_device.hpp): what the entries know of the keyframe slots, the validation of the graph tables, the host entry's
// three passes, the id order of the vertices and the edge records of the plain C++ walk, the outlier entries' frame, and the way of the
// common tables to the device and of counts, points and edges back.  The templates take the problem structure of either entry: the two
// carry the same member names for every graph table, n_keyframes, n_points, current, the point and edge outputs with their capacities,
// counts and lidar_pose_index.
#pragma once
#include <algorithm>
#include <climits>
#include <cstring>

#include "common.hpp"
#include "packed_batch.hpp"
#include "window_gather_device.hpp"

namespace tc2li {

static_assert(sizeof(tc2li_ba_edge) == 40, "ABI layout");
static_assert(sizeof(tc2li_keypoint) == 24, "ABI layout");
// the counts both entries report sit at the same places, and a window that came out has status 0
constexpr int kWinCountStatus = TC2LI_BA_WINDOW_STATUS, kWinCountPoints = TC2LI_BA_WINDOW_N_POINTS, kWinCountEdges = TC2LI_BA_WINDOW_N_EDGES;
constexpr int kWinStatusOk = TC2LI_BA_WINDOW_OK, kWinMaxLidar = TC2LI_BA_WINDOW_MAX_LIDAR;
static_assert(kWinCountStatus == TC2LI_INERTIAL_WINDOW_STATUS && kWinCountPoints == TC2LI_INERTIAL_WINDOW_N_POINTS &&
                  kWinCountEdges == TC2LI_INERTIAL_WINDOW_N_EDGES && kWinStatusOk == TC2LI_INERTIAL_WINDOW_OK &&
                  kWinMaxLidar == TC2LI_INERTIAL_WINDOW_MAX_LIDAR,
              "the shared copy-out reads both count layouts");

// ---- the keyframe slots ----------------------------------------------------------------------------------------------------------------
// what the entries know of the keyframes behind kf_slot: keypoints (-1: an empty slot) and 1 + the highest octave held
struct SlotTable {
    std::vector<int32_t> n, levels;
};

// 0, or TC2LI_ERR_INVALID with the error set
inline int slot_table_from_views(const char* entry, const tc2li_keyframe_view* views, int n_views, SlotTable* slots) {
    if (n_views < 0 || (n_views && !views)) {
        set_error("%s: null or negative views", entry);
        return TC2LI_ERR_INVALID;
    }
    slots->n.assign(n_views, -1);
    slots->levels.assign(n_views, 0);
    std::vector<uint8_t> broken(n_views, 0);
    tracking_pool().parallel_for(n_views, [&](int s) {
        const tc2li_keyframe_view& v = views[s];
        if (v.n < 0) return;
        if (v.n > 0 && (!v.keys || !v.u_right)) { broken[s] = 1; return; }
        slots->n[s] = v.n;
        int top = 0;
        for (int i = 0; i < v.n; ++i) {
            if (v.keys[i].octave < 0) { broken[s] = 1; return; }
            top = std::max(top, v.keys[i].octave + 1);
        }
        slots->levels[s] = top;
    });
    for (int s = 0; s < n_views; ++s)
        if (broken[s]) {
            set_error("%s: view %d has null keys or u_right, or a negative octave", entry, s);
            return TC2LI_ERR_INVALID;
        }
    return 0;
}

inline void slot_table_from_store(tc2li_keyframe_store* store, SlotTable* slots, BawStore* where) {
    const int n_store = keyframe_store_slots(store);
    slots->n.assign(n_store, -1);
    slots->levels.assign(n_store, 0);
    keyframe_store_baw(store, where, slots->n.data(), slots->levels.data(), n_store);
}

// ---- validation ------------------------------------------------------------------------------------------------------------------------
// The checks of the graph tables in the order both entries make them; "" or what is wrong.  Each file's validate calls this after its
// checks of sizes, capacities and null pointers, and hands in what it checks in between: also_keyframe(k) beside the slot of keyframe k,
// keyframe_lists() -- cov_kf, the prev_kf chain -- once the keyframes are known to be sound.
template <class Problem, class AlsoKeyframe, class KeyframeLists>
const char* validate_graph(const Problem& in, const SlotTable& slots, int n_levels, AlsoKeyframe also_keyframe, KeyframeLists keyframe_lists) {
    if (!ascending(in.slot_offsets, in.n_keyframes)) return "slot_offsets do not ascend from 0";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_slot = in.slot_offsets[in.n_keyframes], n_obs = in.obs_offsets[in.n_points];
    if ((n_slot && !in.slot_point) || (n_obs && (!in.obs_kf || !in.obs_index))) return "null slot_point, obs_kf or obs_index";
    const int n_store = (int)slots.n.size();
    for (int k = 0; k < in.n_keyframes; ++k) {
        const int s = in.kf_slot[k];
        if (s < 0 || s >= n_store || slots.n[s] < 0) return "a kf_slot is empty or out of range";
        if (slots.levels[s] > n_levels) return "a slot holds an octave outside [0, n_levels)";
        if (const char* what = also_keyframe(k); what[0]) return what;
    }
    if (const char* what = keyframe_lists(); what[0]) return what;
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

// validate(problem): "" or what is wrong with it
template <class Problem, class Validate>
int validate_all(const char* entry, const Problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels, Validate validate) {
    if (n_problems < 0 || (n_problems && !problems) || !inv_level_sigma2 || n_levels < 1) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "problem", n_problems, invalid_if([&](int p) { return validate(problems[p]); }));
}

// ---- the host entries ------------------------------------------------------------------------------------------------------------------
// A host entry: validate, then size_then_write.  validate(problem, slots) as above; window_one(problem, write) returns whether the lists
// fit; capacity_error(p) sets the error and returns the code.
template <class Problem, class Validate, class WindowOne, class CapacityError>
int host_window_batch(const char* entry, const tc2li_keyframe_view* views, int n_views, const Problem* problems, int n_problems,
                      const float* inv_level_sigma2, int n_levels, Validate validate, WindowOne window_one, CapacityError capacity_error) {
    SlotTable slots;
    int rc = slot_table_from_views(entry, views, n_views, &slots);
    if (rc < 0) return rc;
    rc = validate_all(entry, problems, n_problems, inv_level_sigma2, n_levels, [&](const Problem& in) { return validate(in, slots); });
    if (rc < 0) return rc;
    return size_then_write(n_problems, [&](int p, bool write) { return window_one(problems[p], write); }, capacity_error);
}

// The vertices in id order: `rows` sorted by (kf_id, row); returns every keyframe's place among them, -1: none.
inline std::vector<int32_t> vertices_by_id(const int64_t* kf_id, int n_keyframes, std::vector<int32_t>* rows) {
    std::sort(rows->begin(), rows->end(), [&](int32_t a, int32_t b) { return kf_id[a] != kf_id[b] ? kf_id[a] < kf_id[b] : a < b; });
    std::vector<int32_t> vertex_of(n_keyframes, -1);
    for (size_t r = 0; r < rows->size(); ++r) vertex_of[(*rows)[r]] = (int32_t)r;
    return vertex_of;
}

// The listed points and their edges as the plain C++ walk writes them: row and position of every point, and an edge for every
// observation o of it with edge_of(o), the pixel read from the observer's view.
template <class Problem, class EdgeOf>
void emit_points_and_edges(const Problem& in, const tc2li_keyframe_view* views, const float* inv_level_sigma2, const std::vector<int32_t>& listed,
                           const std::vector<int32_t>& vertex_of, EdgeOf edge_of) {
    int e = 0;
    for (size_t i = 0; i < listed.size(); ++i) {
        const int p = listed[i];
        in.point_row[i] = p;
        memcpy(in.points3_out + 3 * i, in.positions + 3 * (size_t)p, 3 * sizeof(double));
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
}

// ---- the outlier entries ---------------------------------------------------------------------------------------------------------------
// The arguments both outlier entries take; own_fault: what the entry found wrong with the arguments only it has.  0 or TC2LI_ERR_INVALID.
inline int outliers_check(const char* entry, const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                          int n_points, const int32_t* erase_pose, const int32_t* erase_point, int capacity, bool own_fault) {
    if (n_edges < 0 || n_points < 0 || capacity < 0 || own_fault || (n_edges && (!edges || !edge_chi2 || !edge_depth_positive)) ||
        (capacity && (!erase_pose || !erase_point))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    for (int i = 0; i < n_edges; ++i)
        if (edges[i].point < 0 || edges[i].point >= n_points) {
            set_error("%s: edge %d names point %d of %d", entry, i, edges[i].point, n_points);
            return TC2LI_ERR_INVALID;
        }
    return 0;
}

// The (pose, point) pairs to erase: vpEdgesMono first, then vpEdgesStereo, each in creation order; erased(i, stereo) is the entry's rule
// for edge i as a member of that list.  Counted first: on TC2LI_ERR_CAPACITY nothing is written.  Returns the pairs.
template <class Erased>
int outliers_emit(const char* entry, const tc2li_ba_edge* edges, int n_edges, int32_t* erase_pose, int32_t* erase_point, int capacity, Erased erased) {
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
            if (erased(i, stereo != 0)) { erase_pose[n] = edges[i].pose; erase_point[n++] = edges[i].point; }
    return n;
}

// ---- to the device and back ------------------------------------------------------------------------------------------------------------
// The way of a batch through the device, as far as both gathers go it together.  A device entry
//   add()s every problem (the common part of its device record and the running table sizes), fills in its own part and looks at most_rows();
//   take_inputs(), then take()s the places of its own input tables from `io`; take_outputs() and take_work() likewise;
//   ensure()s the buffers, upload_tables() with its own tables put by `own`, bind()s the batch, adds its own pointers and launches;
//   downloads and waits, copy_counts() and -- unless a problem was short of room -- copy_out().
// The buffers, the copies and the wait are PackedTransfer's (packed_batch.hpp).  io is [inputs | outputs], in which the edges come last
// of the common tables (o_edges .. o_after_edges) and the entry's own outputs after them.
template <class Problem, class Dev>
struct WindowTransfer : PackedTransfer {
    const Problem* problems;
    const int n_problems;
    const size_t np;
    std::vector<Dev> dev;
    size_t n_kf = 0, n_slot = 0, n_points = 0, n_obs = 0, n_marks = 0, n_first = 0, n_pointo = 0, n_edge = 0;
    size_t o_prob, o_sigma, o_id, o_pos, o_slot, o_srow, o_spt, o_orow, o_okf, o_oidx, o_flags, o_pflags;
    size_t o_counts, o_lidar, o_p3, o_ptrow, o_edges, o_after_edges;
    size_t w_marks, w_first, w_vertex, w_members, w_listed, w_estart, w_emit;
    int n_counts = 0;
    // the graph tables are resident on the device (map_graph_device.hpp): none is laid out or uploaded, the inputs that do go up lie back
    // to back so that the upload is exactly as long as they are, and the entry binds the tables and fills t_* / slot_row / obs_row itself
    bool resident = false;

    WindowTransfer(const Problem* problems_, int n) : problems(problems_), n_problems(n), np((size_t)n), dev(n) {}

    // where problem p's tables start in the concatenation.  edge_room: the edges the caller has room for; no list is longer than its
    // table, so the device arrays need no more room than that, whatever the caller offers.
    Dev& add(int p, int edge_room) {
        const Problem& in = problems[p];
        return add(p, edge_room, in.slot_offsets[in.n_keyframes], in.obs_offsets[in.n_points]);
    }
    // the same with the entries of the two CSR tables given: the problems of a resident batch carry no table
    Dev& add(int p, int edge_room, int slot_entries, int obs_entries) {
        const Problem& in = problems[p];
        Dev& d = dev[p];
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.slot_off = (int32_t)n_slot;
        d.point_off = (int32_t)n_points; d.n_points = in.n_points; d.obs_off = (int32_t)n_obs;
        d.t_kf = d.kf_off; d.t_slot = d.slot_off; d.t_point = d.point_off; d.t_obs = d.obs_off;
        d.slot_row = d.kf_off + p; d.obs_row = d.point_off + p;
        d.current = in.current;
        d.mark_off = in.n_keyframes > kWinLdsKeyframes ? (int32_t)n_marks : -1;
        d.first_off = in.n_points > kWinLdsPoints ? (int32_t)n_first : -1;
        d.pointo_off = (int32_t)n_pointo; d.point_cap = std::min(in.point_capacity, in.n_points);
        d.edge_off = (int32_t)n_edge; d.edge_cap = std::min(edge_room, obs_entries);
        n_kf += in.n_keyframes; n_slot += slot_entries; n_points += in.n_points; n_obs += obs_entries;
        if (d.mark_off >= 0) n_marks += in.n_keyframes;
        if (d.first_off >= 0) n_first += in.n_points;
        n_pointo += d.point_cap; n_edge += d.edge_cap;
        return d;
    }
    // the longest common table up to and with problem p, in rows; the kernels index with 32 bits
    size_t most_rows(int p) const { return std::max(std::max(n_kf + p, n_slot), std::max(n_points + p, n_obs)); }

    void take_inputs(int n_levels) {
        if (resident) {
            static_assert(sizeof(Dev) % 4 == 0, "the level table and cov_kf follow the records without padding");
            o_prob = io.off; io.off += np * sizeof(Dev);
            o_sigma = io.off; io.off += (size_t)n_levels * 4;
            o_id = o_pos = o_slot = o_srow = o_spt = o_orow = o_okf = o_oidx = o_flags = o_pflags = io.off;
            return;
        }
        o_prob = io.take(np * sizeof(Dev)); o_sigma = io.take((size_t)n_levels * 4); o_id = io.take(n_kf * 8); o_pos = io.take(n_points * 24);
        o_slot = io.take(n_kf * 4); o_srow = io.take((n_kf + np) * 4); o_spt = io.take(n_slot * 4); o_orow = io.take((n_points + np) * 4);
        o_okf = io.take(n_obs * 4); o_oidx = io.take(n_obs * 4); o_flags = io.take(n_kf); o_pflags = io.take(n_points);
    }
    // after the entry's own inputs.  counts_per_problem: TC2LI_*_WINDOW_COUNTS
    void take_outputs(int counts_per_problem) {
        outputs_begin();
        io.off = align256(io.off);   // a resident batch's inputs end where they end
        n_counts = counts_per_problem;
        o_counts = io.take(np * n_counts * 4); o_lidar = io.take(np * kWinMaxLidar * 4); o_p3 = io.take(n_pointo * 24); o_ptrow = io.take(n_pointo * 4);
        o_edges = io.take(n_edge * sizeof(tc2li_ba_edge));
        o_after_edges = io.off;
    }
    void take_work() {
        w_marks = work.take(n_marks * 4); w_first = work.take(n_first * 4); w_vertex = work.take(n_kf * 4); w_members = work.take(n_kf * 4);
        w_listed = work.take(n_points * 4); w_estart = work.take(n_points * 4); w_emit = work.take(np * 4);
    }
    // own(p, problem, its device record): the entry's own tables, put into io
    template <class Own>
    hipError_t upload_tables(const float* inv_level_sigma2, int n_levels, hipStream_t st, Own own) {
        memcpy(io.base + o_prob, dev.data(), np * sizeof(Dev));
        memcpy(io.base + o_sigma, inv_level_sigma2, (size_t)n_levels * 4);
        tracking_pool().parallel_for(n_problems, [&](int p) {
            const Problem& in = problems[p];
            const Dev& d = dev[p];
            if (resident) { own(p, in, d); return; }
            const size_t nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points, n_o = (size_t)in.obs_offsets[in.n_points];
            io.put(o_id, d.kf_off, in.kf_id, nk, 8); io.put(o_slot, d.kf_off, in.kf_slot, nk, 4); io.put(o_flags, d.kf_off, in.kf_flags, nk, 1);
            io.put(o_srow, (size_t)d.kf_off + p, in.slot_offsets, nk + 1, 4);
            io.put(o_spt, d.slot_off, in.slot_point, (size_t)in.slot_offsets[in.n_keyframes], 4);
            io.put(o_pflags, d.point_off, in.point_flags, npt, 1); io.put(o_pos, d.point_off, in.positions, npt, 24);
            io.put(o_orow, (size_t)d.point_off + p, in.obs_offsets, npt + 1, 4);
            io.put(o_okf, d.obs_off, in.obs_kf, n_o, 4); io.put(o_oidx, d.obs_off, in.obs_index, n_o, 4);
            own(p, in, d);
        });
        return upload(st);
    }
    // the common part of the batch
    void bind(WindowBatch& B, const BawStore& where) const {
        uint8_t *d = d_io, *w = d_work;
        B.n_problems = n_problems; B.problem_bytes = (int)sizeof(Dev); B.problems = d + o_prob;
        B.store = where; B.inv_level_sigma2 = (const float*)(d + o_sigma);
        B.kf_slot = (const int32_t*)(d + o_slot); B.kf_id = (const int64_t*)(d + o_id); B.kf_flags = d + o_flags;
        B.slot_offsets = (const int32_t*)(d + o_srow); B.slot_point = (const int32_t*)(d + o_spt);
        B.point_flags = d + o_pflags; B.positions = (const double*)(d + o_pos); B.obs_offsets = (const int32_t*)(d + o_orow);
        B.obs_kf = (const int32_t*)(d + o_okf); B.obs_index = (const int32_t*)(d + o_oidx);
        B.marks_global = (int32_t*)(w + w_marks); B.first_global = (int32_t*)(w + w_first); B.vertex_of = (int32_t*)(w + w_vertex);
        B.members = (int32_t*)(w + w_members); B.listed = (int32_t*)(w + w_listed); B.edge_start = (int32_t*)(w + w_estart);
        B.n_emit = (int32_t*)(w + w_emit);
        B.point_row = (int32_t*)(d + o_ptrow); B.points3_out = (double*)(d + o_p3); B.edges = (tc2li_ba_edge*)(d + o_edges);
    }
    // the downloaded counts into the problems' arrays; fits(problem, counts).  Returns the first problem short of room, or -1.
    template <class Fits>
    int copy_counts(Fits fits) const {
        return tc2li::copy_counts(problems, n_problems, host<const int32_t>(o_counts), n_counts, fits);
    }
    // the downloaded lists of every window that came out into the problems' arrays: lidar_pose_index, the points, the edges where the
    // problem has an array for them, and by own(p, problem, its device record) the entry's own lists
    template <class Own>
    void copy_out(Own own) const {
        tracking_pool().parallel_for(n_problems, [&](int p) {
            const Problem& in = problems[p];
            const Dev& d = dev[p];
            if (in.counts[kWinCountStatus] != kWinStatusOk) return;
            io.get(in.lidar_pose_index, o_lidar, (size_t)p * kWinMaxLidar, kWinMaxLidar, 4);
            const size_t n_pt = (size_t)in.counts[kWinCountPoints];
            io.get(in.point_row, o_ptrow, d.pointo_off, n_pt, 4); io.get(in.points3_out, o_p3, d.pointo_off, n_pt, 24);
            if (in.edges) io.get(in.edges, o_edges, d.edge_off, (size_t)in.counts[kWinCountEdges], sizeof(tc2li_ba_edge));
            own(p, in, d);
        });
    }
};

}  // namespace tc2li

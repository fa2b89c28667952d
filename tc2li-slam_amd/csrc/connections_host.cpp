// tc2li_update_connections_batch / tc2li_host_update_connections_batch / tc2li_update_best_covisibles_batch /
// tc2li_host_update_best_covisibles_batch (include/tc2li_hip.h "local mapping: covisibility graph"): KeyFrame::UpdateConnections
// (SF/src/KeyFrame.cc:391-486) with the AddConnection (:201-214) and UpdateBestCovisibles (:216-238) it triggers, on a flat copy of the
// graph.  This file validates the problems and either walks them in plain C++ or concatenates them for connections_kernels.hip.
#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "connections_device.hpp"
#include "packed_batch.hpp"

namespace tc2li {
namespace {

// "" or what is wrong with the rows of a weight map
const char* validate_rows(const int32_t* offsets, const int32_t* kf, int n_rows, int n_keyframes) {
    for (int r = 0; r < n_rows; ++r)
        for (int j = offsets[r]; j < offsets[r + 1]; ++j) {
            if (kf[j] < 0 || kf[j] >= n_keyframes) return "a keyframe of a weight row is out of range";
            if (j > offsets[r] && kf[j] <= kf[j - 1]) return "a weight row does not ascend strictly by keyframe";
        }
    return "";
}

// "" or what is wrong with problem p
const char* validate(const tc2li_connections_problem& in) {
    if (in.n_keyframes < 0 || in.n_slots < 0 || in.n_points < 0) return "negative size";
    if (in.counter_capacity < 0 || in.ordered_capacity < 0 || in.changed_capacity < 0) return "negative capacity";
    if (!in.kf_flags || !in.conn_offsets || !in.obs_offsets || !in.counts) return "null kf_flags, conn_offsets, obs_offsets or counts";
    if (in.current < 0 || in.current >= in.n_keyframes) return "current out of range";
    if ((in.n_slots && !in.slot_point) || (in.n_points && !in.point_bad)) return "null slot_point or point_bad";
    if (in.counter_capacity && (!in.counter_kf || !in.counter_weight)) return "null counter output";
    if (in.ordered_capacity && (!in.ordered_kf || !in.ordered_weight || !in.touched_kf || !in.touched_changed)) return "null ordered or touched output";
    if (!in.changed_offsets) return "null changed_offsets";
    if (in.changed_capacity && (!in.changed_kf || !in.changed_weight)) return "null changed output";
    if (!ascending(in.conn_offsets, in.n_keyframes)) return "conn_offsets do not ascend from 0";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_conn = in.conn_offsets[in.n_keyframes], n_obs = in.obs_offsets[in.n_points];
    if ((n_conn && (!in.conn_kf || !in.conn_weight)) || (n_obs && !in.obs_kf)) return "null conn_kf, conn_weight or obs_kf";
    const char* rows = validate_rows(in.conn_offsets, in.conn_kf, in.n_keyframes, in.n_keyframes);
    if (rows[0]) return rows;
    for (int i = 0; i < in.n_slots; ++i)
        if (in.slot_point[i] < -1 || in.slot_point[i] >= in.n_points) return "slot_point out of range";
    for (int i = 0; i < n_obs; ++i)
        if (in.obs_kf[i] < 0 || in.obs_kf[i] >= in.n_keyframes) return "obs_kf out of range";
    return "";
}

int validate_all(const char* entry, const tc2li_connections_problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "problem", n_problems, invalid_if([&](int p) { return validate(problems[p]); }));
}

// KeyFrame::UpdateBestCovisibles (:216-238) on keys: sorted ascending (:224), read from the back (:231-232)
int emit_ordered(std::vector<uint64_t>& keys, int32_t* out_kf, int32_t* out_weight) {
    std::sort(keys.begin(), keys.end());
    const int n = (int)keys.size();
    for (int i = 0; i < n; ++i) {
        out_kf[i] = conn::key_kf(keys[n - 1 - i]);
        out_weight[i] = conn::key_weight(keys[n - 1 - i]);
    }
    return n;
}

// The lists that fit the capacities are written; returns whether all did.
bool connections_one(const tc2li_connections_problem& in, bool write) {
    int32_t* counts = in.counts;
    std::fill(counts, counts + TC2LI_CONNECTIONS_COUNTS, 0);
    counts[TC2LI_CONNECTIONS_PARENT] = -1;
    std::vector<int32_t> counter(in.n_keyframes, 0);
    for (int s = 0; s < in.n_slots; ++s) {                                           // :404-423
        const int p = in.slot_point[s];
        if (p < 0 || in.point_bad[p]) continue;                                      // :408, :411
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
            const int kf = in.obs_kf[o];
            if (kf == in.current || (in.kf_flags[kf] & 3)) continue;                 // :418
            ++counter[kf];
        }
    }
    int n_counter = 0, n_pairs = 0, nmax = 0, kf_max = -1;
    for (int k = 0; k < in.n_keyframes; ++k) {                                       // :439-453
        if (!counter[k]) continue;
        ++n_counter;
        if (counter[k] > nmax) { nmax = counter[k]; kf_max = k; }
        n_pairs += counter[k] >= TC2LI_CONNECTIONS_TH;
    }
    if (n_counter == 0) return true;                                                 // :426-427
    const bool by_max = n_pairs == 0;                                                // :455-459
    if (by_max) n_pairs = 1;
    counts[TC2LI_CONNECTIONS_STATUS] = TC2LI_CONNECTIONS_UPDATED;
    counts[TC2LI_CONNECTIONS_N_COUNTER] = n_counter;
    counts[TC2LI_CONNECTIONS_N_ORDERED] = n_pairs;
    if (n_counter > in.counter_capacity || n_pairs > in.ordered_capacity) return false;
    std::vector<int32_t> touched, lens;
    std::vector<uint8_t> found_at;
    std::vector<uint64_t> keys;
    for (int k = 0; k < in.n_keyframes; ++k)
        if (by_max ? k == kf_max : counter[k] >= TC2LI_CONNECTIONS_TH) { touched.push_back(k); keys.push_back(conn::key(counter[k], k)); }
    if (in.first_connection && !in.is_init_kf) counts[TC2LI_CONNECTIONS_PARENT] = conn::key_kf(*std::max_element(keys.begin(), keys.end()));   // :478-483
    // AddConnection in every touched keyframe (:201-211)
    std::vector<uint8_t> changed(n_pairs);
    int n_changed = 0, n_entries = 0;
    const int cur_alive = (in.kf_flags[in.current] & 1) ? 0 : 1;
    for (int i = 0; i < n_pairs; ++i) {
        const int k = touched[i];
        int alive = 0, held = 0;
        bool found = false;
        for (int j = in.conn_offsets[k]; j < in.conn_offsets[k + 1]; ++j) {
            if (in.conn_kf[j] == in.current) { found = true; held = in.conn_weight[j]; }
            else alive += (in.kf_flags[in.conn_kf[j]] & 1) ? 0 : 1;
        }
        changed[i] = !(found && held == counter[k]);                                 // :205-210
        found_at.push_back(found);
        lens.push_back(changed[i] ? alive + cur_alive : 0);
        n_changed += changed[i];
        n_entries += lens[i];
    }
    counts[TC2LI_CONNECTIONS_N_CHANGED] = n_changed;
    counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] = n_entries;
    if (n_entries > in.changed_capacity) return false;
    if (!write) return true;
    for (int k = 0, a = 0; k < in.n_keyframes; ++k)                                  // :473
        if (counter[k]) { in.counter_kf[a] = k; in.counter_weight[a++] = counter[k]; }
    emit_ordered(keys, in.ordered_kf, in.ordered_weight);                            // :461-475
    int c = 0, off = 0;
    for (int i = 0; i < n_pairs; ++i) {
        const int k = touched[i];
        in.touched_kf[i] = k;
        in.touched_changed[i] = changed[i];
        if (!changed[i]) continue;
        in.changed_offsets[c++] = off;
        keys.clear();                                                                // :216-238 on the updated row
        for (int j = in.conn_offsets[k]; j < in.conn_offsets[k + 1]; ++j) {
            const int kk = in.conn_kf[j];
            if (in.kf_flags[kk] & 1) continue;                                       // :229
            keys.push_back(conn::key(kk == in.current ? counter[k] : in.conn_weight[j], kk));
        }
        if (!found_at[i] && cur_alive) keys.push_back(conn::key(counter[k], in.current));
        off += emit_ordered(keys, in.changed_kf + off, in.changed_weight + off);
    }
    in.changed_offsets[c] = off;
    return true;
}

int capacity_error(const char* entry, const tc2li_connections_problem* problems, int p) {
    const tc2li_connections_problem& in = problems[p];
    set_error("%s: problem %d needs room for %d counter, %d ordered and %d changed entries and has %d, %d and %d", entry, p,
              in.counts[TC2LI_CONNECTIONS_N_COUNTER], in.counts[TC2LI_CONNECTIONS_N_ORDERED], in.counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES],
              in.counter_capacity, in.ordered_capacity, in.changed_capacity);
    return TC2LI_ERR_CAPACITY;
}

bool fits(const tc2li_connections_problem& in, const int32_t* counts) {
    return counts[TC2LI_CONNECTIONS_N_COUNTER] <= in.counter_capacity && counts[TC2LI_CONNECTIONS_N_ORDERED] <= in.ordered_capacity &&
           counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] <= in.changed_capacity;
}

int check_covisibles(const char* entry, const int32_t* row_offsets, const int32_t* row_kf, const int32_t* row_weight, int n_rows, const uint8_t* bad,
                     int n_keyframes, const int32_t* out_offsets, const int32_t* out_kf, const int32_t* out_weight) {
    if (n_rows < 0 || n_keyframes < 0 || !row_offsets || !out_offsets) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    if (!ascending(row_offsets, n_rows)) {
        set_error("%s: row_offsets do not ascend from 0", entry);
        return TC2LI_ERR_INVALID;
    }
    if (row_offsets[n_rows] && (!row_kf || !row_weight || !bad || !out_kf || !out_weight)) {
        set_error("%s: null array", entry);
        return TC2LI_ERR_INVALID;
    }
    const char* rows = validate_rows(row_offsets, row_kf, n_rows, n_keyframes);
    if (rows[0]) {
        set_error("%s: %s", entry, rows);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

}  // namespace

// for tc2li_process_new_keyframe_batch (process_keyframe_device.hpp), which votes on the observation rows it has just written
const char* connections_what_is_wrong(const tc2li_connections_problem& in) { return validate(in); }
int host_connections(const char* entry, const tc2li_connections_problem* problems, int n_problems, bool write) {
    if (write)
        return size_then_write(n_problems, [&](int p, bool w) { return connections_one(problems[p], w); }, [&](int p) { return capacity_error(entry, problems, p); });
    std::vector<uint8_t> ok(n_problems, 1);
    tracking_pool().parallel_for(n_problems, [&](int p) { ok[p] = connections_one(problems[p], false); });
    for (int p = 0; p < n_problems; ++p)
        if (!ok[p]) return capacity_error(entry, problems, p);
    return n_problems;
}
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_connections_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_connections_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kConnLdsKeyframes; out[1] = kConnRankLanes; out[2] = kConnThreads;
    return 3;
}

extern "C" int tc2li_host_update_connections_batch(const tc2li_connections_problem* problems, int n_problems) {
    const char* entry = "tc2li_host_update_connections_batch";
    const int rc = validate_all(entry, problems, n_problems);
    if (rc < 0) return rc;
    return size_then_write(n_problems, [&](int p, bool write) { return connections_one(problems[p], write); },
                           [&](int p) { return capacity_error(entry, problems, p); });
}

extern "C" int tc2li_update_connections_batch(const tc2li_connections_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_update_connections_batch";
    const int rc = validate_all(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // where every problem's tables start in the concatenation
    std::vector<ConnProblemDev> dev(n_problems);
    size_t n_kf = 0, n_conn = 0, n_slots = 0, n_points = 0, n_obs = 0, n_hist = 0, n_counter = 0, n_items = 0, n_changed = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_connections_problem& in = problems[p];
        ConnProblemDev& d = dev[p];
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.conn_row_off = (int32_t)(n_kf + p); d.conn_off = (int32_t)n_conn;
        d.slot_off = (int32_t)n_slots; d.n_slots = in.n_slots;
        d.point_off = (int32_t)n_points; d.obs_row_off = (int32_t)(n_points + p); d.obs_off = (int32_t)n_obs;
        d.current = in.current;
        d.flags = (in.first_connection ? 1 : 0) | (in.is_init_kf ? 2 : 0);
        d.hist_off = in.n_keyframes > kConnLdsKeyframes ? (int32_t)n_hist : -1;
        d.counter_off = (int32_t)n_counter; d.counter_cap = in.counter_capacity;
        d.ordered_off = (int32_t)n_items; d.ordered_cap = in.ordered_capacity;
        d.changed_off = (int32_t)n_changed; d.changed_cap = in.changed_capacity;
        n_kf += in.n_keyframes; n_conn += in.conn_offsets[in.n_keyframes]; n_slots += in.n_slots; n_points += in.n_points;
        n_obs += in.obs_offsets[in.n_points];
        if (d.hist_off >= 0) n_hist += in.n_keyframes;
        n_counter += in.counter_capacity; n_items += in.ordered_capacity; n_changed += in.changed_capacity;
        if (std::max(std::max(std::max(n_kf + p, n_conn), std::max(n_slots, n_points + p)), std::max(std::max(n_obs, n_counter), std::max(n_items + p, n_changed))) >
            kMaxRows)
            return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    // one buffer: [inputs | outputs]; the upload is the first part, the download the second
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const size_t o_prob = io.take(np * sizeof(ConnProblemDev)), o_poi = io.take(n_items * 4), o_flags = io.take(n_kf), o_crow = io.take((n_kf + np) * 4),
                 o_ckf = io.take(n_conn * 4), o_cw = io.take(n_conn * 4), o_spt = io.take(n_slots * 4), o_pbad = io.take(n_points),
                 o_orow = io.take((n_points + np) * 4), o_okf = io.take(n_obs * 4);
    T.outputs_begin();
    const size_t o_counts = io.take(np * TC2LI_CONNECTIONS_COUNTS * 4), o_cnkf = io.take(n_counter * 4), o_cnw = io.take(n_counter * 4),
                 o_okfs = io.take(n_items * 4), o_ows = io.take(n_items * 4), o_tkf = io.take(n_items * 4), o_tch = io.take(n_items),
                 o_choff = io.take((n_items + np) * 4), o_chkf = io.take(n_changed * 4), o_chw = io.take(n_changed * 4);
    const size_t o_hist = work.take(n_hist * 4), o_tw = work.take(n_items * 4), o_ioff = work.take(n_items * 4), o_ifound = work.take(n_items);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceConnections>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, dev.data(), np, sizeof(ConnProblemDev));
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_connections_problem& in = problems[p];
        const ConnProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, nc = (size_t)in.conn_offsets[in.n_keyframes], npt = (size_t)in.n_points, no = (size_t)in.obs_offsets[in.n_points];
        int32_t* poi = T.host<int32_t>(o_poi) + d.ordered_off;
        for (int i = 0; i < in.ordered_capacity; ++i) poi[i] = p;
        io.put(o_flags, d.kf_off, in.kf_flags, nk, 1);
        io.put(o_crow, d.conn_row_off, in.conn_offsets, nk + 1, 4);
        io.put(o_ckf, d.conn_off, in.conn_kf, nc, 4); io.put(o_cw, d.conn_off, in.conn_weight, nc, 4);
        io.put(o_spt, d.slot_off, in.slot_point, in.n_slots, 4);
        io.put(o_pbad, d.point_off, in.point_bad, npt, 1);
        io.put(o_orow, d.obs_row_off, in.obs_offsets, npt + 1, 4);
        io.put(o_okf, d.obs_off, in.obs_kf, no, 4);
    });
    TC2LI_HIP_CHECK(T.upload(st));
    ConnBatch B{};
    B.n_problems = n_problems; B.n_items = (int)n_items;
    B.problems = T.dev<const ConnProblemDev>(o_prob); B.problem_of_item = T.dev<const int32_t>(o_poi);
    B.kf_flags = T.dev<const uint8_t>(o_flags); B.conn_offsets = T.dev<const int32_t>(o_crow); B.conn_kf = T.dev<const int32_t>(o_ckf);
    B.conn_weight = T.dev<const int32_t>(o_cw); B.slot_point = T.dev<const int32_t>(o_spt); B.point_bad = T.dev<const uint8_t>(o_pbad);
    B.obs_offsets = T.dev<const int32_t>(o_orow); B.obs_kf = T.dev<const int32_t>(o_okf);
    B.hist = T.dev_work<int32_t>(o_hist); B.touched_weight = T.dev_work<int32_t>(o_tw); B.item_off = T.dev_work<int32_t>(o_ioff);
    B.item_found = T.dev_work<uint8_t>(o_ifound);
    B.counts = T.dev<int32_t>(o_counts); B.counter_kf = T.dev<int32_t>(o_cnkf); B.counter_weight = T.dev<int32_t>(o_cnw);
    B.ordered_kf = T.dev<int32_t>(o_okfs); B.ordered_weight = T.dev<int32_t>(o_ows); B.touched_kf = T.dev<int32_t>(o_tkf);
    B.touched_changed = T.dev<uint8_t>(o_tch); B.changed_offsets = T.dev<int32_t>(o_choff); B.changed_kf = T.dev<int32_t>(o_chkf);
    B.changed_weight = T.dev<int32_t>(o_chw);
    launch_update_connections(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    const int short_of_room = copy_counts(problems, n_problems, T.host<const int32_t>(o_counts), TC2LI_CONNECTIONS_COUNTS, fits);
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_connections_problem& in = problems[p];
        const ConnProblemDev& D = dev[p];
        const int32_t* counts = in.counts;
        if (counts[TC2LI_CONNECTIONS_STATUS] == TC2LI_CONNECTIONS_UNCHANGED) return;
        const size_t nc = (size_t)counts[TC2LI_CONNECTIONS_N_COUNTER], no = (size_t)counts[TC2LI_CONNECTIONS_N_ORDERED];
        io.get(in.counter_kf, o_cnkf, D.counter_off, nc, 4); io.get(in.counter_weight, o_cnw, D.counter_off, nc, 4);
        io.get(in.ordered_kf, o_okfs, D.ordered_off, no, 4); io.get(in.ordered_weight, o_ows, D.ordered_off, no, 4);
        io.get(in.touched_kf, o_tkf, D.ordered_off, no, 4); io.get(in.touched_changed, o_tch, D.ordered_off, no, 1);
        io.get(in.changed_offsets, o_choff, (size_t)D.ordered_off + p, (size_t)counts[TC2LI_CONNECTIONS_N_CHANGED] + 1, 4);
        io.get(in.changed_kf, o_chkf, D.changed_off, (size_t)counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES], 4);
        io.get(in.changed_weight, o_chw, D.changed_off, (size_t)counts[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES], 4);
    });
    return n_problems;
}

extern "C" int tc2li_host_update_best_covisibles_batch(const int32_t* row_offsets, const int32_t* row_kf, const int32_t* row_weight, int n_rows,
                                                       const uint8_t* bad, int n_keyframes, int32_t* out_offsets, int32_t* out_kf, int32_t* out_weight) {
    const int rc = check_covisibles("tc2li_host_update_best_covisibles_batch", row_offsets, row_kf, row_weight, n_rows, bad, n_keyframes, out_offsets,
                                    out_kf, out_weight);
    if (rc < 0) return rc;
    std::vector<uint64_t> keys;
    int off = 0;
    for (int r = 0; r < n_rows; ++r) {
        out_offsets[r] = off;
        keys.clear();
        for (int j = row_offsets[r]; j < row_offsets[r + 1]; ++j)
            if (!bad[row_kf[j]]) keys.push_back(conn::key(row_weight[j], row_kf[j]));    // :229
        off += emit_ordered(keys, out_kf + off, out_weight + off);
    }
    out_offsets[n_rows] = off;
    return n_rows;
}

extern "C" int tc2li_update_best_covisibles_batch(const int32_t* row_offsets, const int32_t* row_kf, const int32_t* row_weight, int n_rows,
                                                  const uint8_t* bad, int n_keyframes, int32_t* out_offsets, int32_t* out_kf, int32_t* out_weight,
                                                  void* stream) {
    const int rc = check_covisibles("tc2li_update_best_covisibles_batch", row_offsets, row_kf, row_weight, n_rows, bad, n_keyframes, out_offsets, out_kf,
                                    out_weight);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    out_offsets[0] = 0;
    if (n_rows == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    const size_t nr = (size_t)n_rows, ne = (size_t)row_offsets[n_rows], nk = (size_t)n_keyframes;
    PackedTransfer T;
    Packer& io = T.io;
    const size_t o_row = io.take((nr + 1) * 4), o_kf = io.take(ne * 4), o_w = io.take(ne * 4), o_bad = io.take(nk);
    T.outputs_begin();
    const size_t o_count = io.take(nr * 4), o_okf = io.take(ne * 4), o_ow = io.take(ne * 4);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceCovisibles>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_row, 0, row_offsets, nr + 1, 4);
    io.put(o_kf, 0, row_kf, ne, 4); io.put(o_w, 0, row_weight, ne, 4);
    if (bad) io.put(o_bad, 0, bad, nk, 1);
    TC2LI_HIP_CHECK(T.upload(st));
    CovisBatch B{};
    B.n_rows = n_rows;
    B.row_offsets = T.dev<const int32_t>(o_row); B.row_kf = T.dev<const int32_t>(o_kf); B.row_weight = T.dev<const int32_t>(o_w);
    B.bad = T.dev<const uint8_t>(o_bad);
    B.out_count = T.dev<int32_t>(o_count); B.out_kf = T.dev<int32_t>(o_okf); B.out_weight = T.dev<int32_t>(o_ow);
    launch_update_best_covisibles(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    // the device wrote every list at its row's start; close the gaps the bad keyframes left
    const int32_t* count = T.host<const int32_t>(o_count);
    int at = 0;
    for (int r = 0; r < n_rows; ++r) {
        out_offsets[r] = at;
        io.get(out_kf + at, o_okf, row_offsets[r], (size_t)count[r], 4);
        io.get(out_weight + at, o_ow, row_offsets[r], (size_t)count[r], 4);
        at += count[r];
    }
    out_offsets[n_rows] = at;
    return n_rows;
}

// tc2li_process_new_keyframe_batch / tc2li_host_process_new_keyframe_batch / tc2li_process_new_keyframe_limits (include/tc2li_hip.h):
// LocalMapping::ProcessNewKeyFrame (SF/src/LocalMapping.cc:312-352) on the flat graph.  Here: the validation both entries share, the host
// twin (plain sequential C++ in the reference's order, the refresh at the slot's turn, one problem per worker), and the device entry: one
// packed upload, the launches of process_keyframe_kernels.hip and connections_kernels.hip on the rows the former wrote, one download, and
// the host twin for the problems that met the observation limit.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <new>
#include <vector>

#include "common.hpp"
#include "fuse_search.hpp"
#include "packed_batch.hpp"
#include "process_keyframe_device.hpp"

namespace tc2li {
namespace {

typedef tc2li_process_keyframe_problem Problem;

// "" or what is wrong with problem `in`; stored_n(slot) = the keypoints stored for a slot, -1: empty or out of range
template <class StoredN>
const char* what_is_wrong(const Problem& in, StoredN stored_n) {
    const tc2li_connections_problem& c = in.conn;
    const char* conn = connections_what_is_wrong(c);
    if (conn[0]) return conn;
    const int nk = c.n_keyframes, np = c.n_points, cur = c.current;
    const int n_obs = c.obs_offsets[np];
    if (!in.kf_slot || !in.centres || !in.counts) return "null kf_slot, centres or counts";
    if (np > 0 && (!in.positions || !in.point_nobs || !in.point_ref_kf || !in.point_ref_level_scale)) return "null point table";
    if (n_obs > 0 && !in.obs_index) return "null obs_index";
    if (in.associated_capacity < 0 || in.recent_capacity < 0 || in.obs_capacity < 0) return "negative capacity";
    if ((in.associated_capacity > 0 && (!in.associated_slot || !in.associated_point)) || (in.recent_capacity > 0 && !in.recent) ||
        (in.obs_capacity > 0 && (!in.obs_kf_out || !in.obs_index_out)))
        return "null list with a capacity";
    if (!(in.last_level_scale > 0)) return "last_level_scale must be positive";
    std::vector<int32_t> n_of;
    try {
        n_of.resize(nk);
    } catch (const std::bad_alloc&) {
        return "no memory for a table of n_keyframes entries";
    }
    for (int k = 0; k < nk; ++k) {
        if (in.kf_slot[k] < -1) return "kf_slot below -1";
        n_of[k] = in.kf_slot[k] < 0 ? -1 : stored_n(in.kf_slot[k]);
        if (in.kf_slot[k] >= 0 && n_of[k] < 0) return "a keyframe names a slot that is empty or out of range";
    }
    if (n_of[cur] < 0) return "the current keyframe needs a slot";
    if (n_of[cur] != c.n_slots) return "n_slots is not the stored keypoint count of the current keyframe";
    for (int p = 0; p < np; ++p)
        for (int o = c.obs_offsets[p]; o < c.obs_offsets[p + 1]; ++o) {
            const int kf = c.obs_kf[o];
            if (o > c.obs_offsets[p] && kf <= c.obs_kf[o - 1]) return "an observation row does not ascend strictly";
            if (in.obs_index[o] < 0 || (n_of[kf] >= 0 && in.obs_index[o] >= n_of[kf])) return "observation index out of range";
        }
    for (int i = 0; i < c.n_slots; ++i) {
        const int p = c.slot_point[i];
        if (p < 0) continue;
        bool in_current = false;
        for (int o = c.obs_offsets[p]; o < c.obs_offsets[p + 1]; ++o) {
            if (n_of[c.obs_kf[o]] < 0) return "an observer of a point of the slot row has no slot";
            in_current |= c.obs_kf[o] == cur;
        }
        if (!c.point_bad[p] && !in_current && (in.point_ref_kf[p] < 0 || in.point_ref_kf[p] >= nk)) return "point_ref_kf out of range";
    }
    return "";
}

int check_call(const char* entry, const Problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems > 0 && !problems)) {
        set_error("%s: invalid argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------
struct Result {
    int32_t counts[kPkCounts];
    std::vector<int32_t> a_slot, a_point, recent, nobs, obs_off, obs_kf, obs_idx, desc_kf, desc_idx;
    std::vector<uint8_t> refreshed;
    std::vector<float> normals, mn, mx;
};

// desc_of(kf): the descriptors of keyframe row kf; u_right: of the current keyframe
template <class DescOf>
void run_twin(const Problem& in, DescOf desc_of, const float* u_right, Result& r) {
    const tc2li_connections_problem& c = in.conn;
    const int np = c.n_points, cur = c.current;
    std::vector<std::vector<NbObs>> obs(np);
    for (int p = 0; p < np; ++p)
        for (int o = c.obs_offsets[p]; o < c.obs_offsets[p + 1]; ++o) obs[p].push_back(NbObs{c.obs_kf[o], in.obs_index[o]});
    if (np) r.nobs.assign(in.point_nobs, in.point_nobs + np);
    r.desc_kf.assign(np, -1); r.desc_idx.assign(np, -1);
    r.refreshed.assign(np, 0); r.normals.assign(3 * (size_t)np, 0.f); r.mn.assign(np, 0.f); r.mx.assign(np, 0.f);
    std::vector<uint32_t> d;
    std::vector<int> row_obs;
    for (int i = 0; i < c.n_slots; ++i) {                                    // :326
        const int p = c.slot_point[i];
        if (p < 0 || c.point_bad[p]) continue;                               // :329, :331
        std::vector<NbObs>& v = obs[p];
        auto at = v.begin();
        while (at != v.end() && at->kf < cur) ++at;
        if (at != v.end() && at->kf == cur) { r.recent.push_back(p); continue; }   // :333, :341
        v.insert(at, NbObs{cur, i});                                         // :335; MapPoint.cc:150-175
        r.nobs[p] += u_right[i] >= 0 ? 2 : 1;                                // MapPoint.cc:171-174
        r.a_slot.push_back(i); r.a_point.push_back(p);
        // :336, MapPoint.cc:435-503 in the order of k_map_points_refresh
        const int N = (int)v.size();
        const float* X = in.positions + 3 * (size_t)p;
        const float px = X[0], py = X[1], pz = X[2];
        float nx = 0, ny = 0, nz = 0;
        for (const NbObs& ob : v) {                                          // MapPoint.cc:456-475: no isBad() test
            const float* C = in.centres + 3 * (size_t)ob.kf;
            const float vx = px - C[0], vy = py - C[1], vz = pz - C[2];
            const float nr = sqrtf(vx * vx + vy * vy + vz * vz);
            nx = nx + vx / nr; ny = ny + vy / nr; nz = nz + vz / nr;
        }
        const float* R = in.centres + 3 * (size_t)in.point_ref_kf[p];
        const float rx = px - R[0], ry = py - R[1], rz = pz - R[2];
        const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
        r.mx[p] = dist * in.point_ref_level_scale[p];                        // MapPoint.cc:499
        r.mn[p] = r.mx[p] / in.last_level_scale;                             // MapPoint.cc:500
        r.normals[3 * (size_t)p] = nx / (float)N; r.normals[3 * (size_t)p + 1] = ny / (float)N; r.normals[3 * (size_t)p + 2] = nz / (float)N;
        r.refreshed[p] = 1;
        // :337, MapPoint.cc:338-412
        d.clear(); row_obs.clear();
        for (size_t o = 0; o < v.size(); ++o) {
            if (c.kf_flags[v[o].kf] & 1) continue;                           // MapPoint.cc:361
            const uint32_t* src = reinterpret_cast<const uint32_t*>(desc_of(v[o].kf)) + 8 * (size_t)v[o].idx;
            d.insert(d.end(), src, src + 8);
            row_obs.push_back((int)o);
        }
        const int M = (int)row_obs.size();
        if (M == 0) continue;                                                // MapPoint.cc:374
        int best_median = 0x7fffffff, best = 0;
        for (int k = 0; k < M; ++k) {
            const int m = row_median(d.data(), 8, M, k);                     // MapPoint.cc:397-399
            if (m < best_median) { best_median = m; best = k; }              // MapPoint.cc:401
        }
        r.desc_kf[p] = v[row_obs[best]].kf; r.desc_idx[p] = v[row_obs[best]].idx;
    }
    r.obs_off.assign(np + 1, 0);
    for (int p = 0; p < np; ++p) {
        for (const NbObs& ob : obs[p]) { r.obs_kf.push_back(ob.kf); r.obs_idx.push_back(ob.idx); }
        r.obs_off[p + 1] = (int32_t)r.obs_kf.size();
    }
    r.counts[kPkStatus] = TC2LI_PROCESS_KEYFRAME_ON_HOST; r.counts[kPkAssociated] = (int32_t)r.a_slot.size();
    r.counts[kPkRecent] = (int32_t)r.recent.size(); r.counts[kPkObs] = (int32_t)r.obs_kf.size();
}

// UpdateConnections (:348) of a problem on the end state r
tc2li_connections_problem on_end_state(const Problem& in, const Result& r) {
    tc2li_connections_problem c = in.conn;
    c.obs_offsets = r.obs_off.data(); c.obs_kf = r.obs_kf.data();
    return c;
}

bool fits(const Problem& in, const int32_t* counts) {
    return counts[kPkAssociated] <= in.associated_capacity && counts[kPkRecent] <= in.recent_capacity && counts[kPkObs] <= in.obs_capacity;
}
bool conn_fits(const tc2li_connections_problem& in) {
    const int32_t* c = in.counts;
    return c[TC2LI_CONNECTIONS_N_COUNTER] <= in.counter_capacity && c[TC2LI_CONNECTIONS_N_ORDERED] <= in.ordered_capacity &&
           c[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] <= in.changed_capacity;
}
int capacity_error(const char* entry, const Problem* problems, int p) {
    const int32_t *c = problems[p].counts, *k = problems[p].conn.counts;
    set_error("%s: problem %d needs room for %d associated, %d recent, %d observations, %d counter, %d ordered and %d changed entries", entry, p, c[kPkAssociated],
              c[kPkRecent], c[kPkObs], k[TC2LI_CONNECTIONS_N_COUNTER], k[TC2LI_CONNECTIONS_N_ORDERED], k[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES]);
    return TC2LI_ERR_CAPACITY;
}
int first_short_of_room(const Problem* problems, int n_problems) {
    for (int p = 0; p < n_problems; ++p)
        if (!fits(problems[p], problems[p].counts) || !conn_fits(problems[p].conn)) return p;
    return -1;
}
template <class T> void give(T* dst, const std::vector<T>& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T)); }
void write_result(const Problem& in, const Result& r) {
    give(in.associated_slot, r.a_slot); give(in.associated_point, r.a_point); give(in.recent, r.recent); give(in.point_nobs_out, r.nobs);
    give(in.obs_offsets_out, r.obs_off); give(in.obs_kf_out, r.obs_kf); give(in.obs_index_out, r.obs_idx); give(in.desc_kf, r.desc_kf);
    give(in.desc_index, r.desc_idx); give(in.refreshed, r.refreshed); give(in.normals_out, r.normals); give(in.min_distance_out, r.mn);
    give(in.max_distance_out, r.mx);
}

// the arrays of a store slot that the twin reads, copied to the host
struct HostSlot {
    std::vector<uint8_t> desc;
    std::vector<float> u_right;
};

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_process_new_keyframe_limits(int32_t* out, int capacity) {
    const int32_t v[4] = {kPkMaxObs, kNbMaxKeys, kPkThreads, kPkRefreshWaves};
    if (!out || capacity < 0) { set_error("tc2li_process_new_keyframe_limits: invalid argument"); return TC2LI_ERR_INVALID; }
    for (int i = 0; i < std::min(capacity, 4); ++i) out[i] = v[i];
    return 4;
}

extern "C" int tc2li_host_process_new_keyframe_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_process_keyframe_problem* problems,
                                                     int n_problems) {
    const char* entry = "tc2li_host_process_new_keyframe_batch";
    int rc = check_call(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (n_views < 0 || (n_views > 0 && !views)) { set_error("%s: invalid argument", entry); return TC2LI_ERR_INVALID; }
    for (int v = 0; v < n_views; ++v)
        if (views[v].n > 0 && (!views[v].descriptors || !views[v].u_right)) { set_error("%s: view %d: null descriptors or u_right", entry, v); return TC2LI_ERR_INVALID; }
    rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) {
        return what_is_wrong(problems[p], [&](int s) { return s < n_views ? std::max(views[s].n, -1) : -1; });
    }));
    if (rc < 0) return rc;
    if (n_problems == 0) return 0;
    std::vector<Result> results(n_problems);
    std::vector<tc2li_connections_problem> conn(n_problems);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const Problem& in = problems[p];
        run_twin(in, [&](int kf) { return views[in.kf_slot[kf]].descriptors; }, views[in.kf_slot[in.conn.current]].u_right, results[p]);
        memcpy(in.counts, results[p].counts, sizeof(results[p].counts));
        conn[p] = on_end_state(in, results[p]);
    });
    host_connections(entry, conn.data(), n_problems, false);                 // the sizes of every problem into conn.counts
    const int short_of_room = first_short_of_room(problems, n_problems);
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    rc = host_connections(entry, conn.data(), n_problems, true);
    if (rc < 0) return rc;
    tracking_pool().parallel_for(n_problems, [&](int p) { write_result(problems[p], results[p]); });
    return n_problems;
}

extern "C" int tc2li_process_new_keyframe_batch(tc2li_keyframe_store* store, const tc2li_process_keyframe_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_process_new_keyframe_batch";
    int rc = check_call(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (!store) { set_error("%s: invalid argument", entry); return TC2LI_ERR_INVALID; }
    // ---- every check before any allocation sized by the caller's counts: a row's slot is looked up in the store as it is now ----
    rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) {
        return what_is_wrong(problems[p], [&](int s) {
            NbKf d{};
            int32_t levels = 0;
            return keyframe_store_neighbors(store, s, &d, &levels) ? d.n : -1;
        });
    }));
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();

    // ---- where every problem's tables start in the concatenation ----
    const size_t np_ = (size_t)n_problems;
    std::vector<PkProblemDev> dev(n_problems);
    std::vector<ConnProblemDev> cdev(n_problems);
    size_t n_kf = 0, n_conn = 0, n_slots = 0, n_points = 0, n_obs = 0, n_obs_out = 0, n_list = 0, n_hist = 0, n_counter = 0, n_items = 0, n_changed = 0;
    for (int p = 0; p < n_problems; ++p) {
        const Problem& in = problems[p];
        const tc2li_connections_problem& c = in.conn;
        int occupied = 0;
        for (int i = 0; i < c.n_slots; ++i) occupied += c.slot_point[i] >= 0;
        const int obs = c.obs_offsets[c.n_points];
        PkProblemDev& D = dev[p];
        D = PkProblemDev{};
        D.n_kf = c.n_keyframes; D.n_slots = c.n_slots; D.n_points = c.n_points; D.current = c.current;
        D.kf_off = (int32_t)n_kf; D.slot_off = (int32_t)n_slots; D.point_off = (int32_t)n_points; D.point_row_off = (int32_t)(n_points + p);
        D.obs_off = (int32_t)n_obs; D.obs_out_off = (int32_t)n_obs_out; D.list_off = (int32_t)n_list; D.item_off = (int32_t)n_list;
        D.last_level_scale = in.last_level_scale;
        ConnProblemDev& d = cdev[p];
        d = ConnProblemDev{};
        d.kf_off = D.kf_off; d.n_kf = c.n_keyframes; d.conn_row_off = (int32_t)(n_kf + p); d.conn_off = (int32_t)n_conn;
        d.slot_off = D.slot_off; d.n_slots = c.n_slots; d.point_off = D.point_off; d.obs_row_off = D.point_row_off; d.obs_off = D.obs_out_off;
        d.current = c.current; d.flags = (c.first_connection ? 1 : 0) | (c.is_init_kf ? 2 : 0);
        d.hist_off = c.n_keyframes > kConnLdsKeyframes ? (int32_t)n_hist : -1;
        d.counter_off = (int32_t)n_counter; d.counter_cap = c.counter_capacity; d.ordered_off = (int32_t)n_items; d.ordered_cap = c.ordered_capacity;
        d.changed_off = (int32_t)n_changed; d.changed_cap = c.changed_capacity;
        n_kf += c.n_keyframes; n_conn += c.conn_offsets[c.n_keyframes]; n_slots += c.n_slots; n_points += c.n_points; n_obs += obs;
        n_obs_out += (size_t)obs + occupied; n_list += occupied;
        if (d.hist_off >= 0) n_hist += c.n_keyframes;
        n_counter += c.counter_capacity; n_items += c.ordered_capacity; n_changed += c.changed_capacity;
        if (std::max(std::max(std::max(n_kf + p + 1, n_conn), std::max(n_slots, 3 * n_points + p + 1)), std::max(std::max(n_obs_out, n_counter), std::max(n_items + p + 1, n_changed))) >
            kMaxRows)
            return too_many_rows(entry, p);
    }
    // the keyframe rows: descriptors of the store slot, the centre
    std::vector<PkKf> kfs;
    try {
        kfs.resize(n_kf);
    } catch (const std::bad_alloc&) {
        set_error("%s: no memory for %zu keyframe rows", entry, n_kf);
        return TC2LI_ERR_INVALID;
    }
    for (int p = 0; p < n_problems; ++p) {
        const Problem& in = problems[p];
        for (int k = 0; k < in.conn.n_keyframes; ++k) {
            PkKf& d = kfs[dev[p].kf_off + k];
            d = PkKf{};
            memcpy(d.centre, in.centres + 3 * (size_t)k, 12);
            if (in.kf_slot[k] < 0) continue;
            NbKf s{};
            int32_t levels = 0;
            if (!keyframe_store_neighbors(store, in.kf_slot[k], &s, &levels)) {   // erased since the check: another thread's doing
                set_error("%s: problem %d names slot %d, which is empty or out of range", entry, p, in.kf_slot[k]);
                return TC2LI_ERR_INVALID;
            }
            d.desc = s.desc;
            if (k == in.conn.current) dev[p].u_right = s.u_right;
        }
    }

    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const auto t_prob = io.take<PkProblemDev>(np_); const auto t_cprob = io.take<ConnProblemDev>(np_); const auto t_poi = io.take<int32_t>(n_items);
    const auto t_kfs = io.take<PkKf>(n_kf); const auto t_kflag = io.take<uint8_t>(n_kf); const auto t_crow = io.take<int32_t>(n_kf + np_);
    const auto t_ckf = io.take<int32_t>(n_conn); const auto t_cw = io.take<int32_t>(n_conn); const auto t_slot = io.take<int32_t>(n_slots);
    const auto t_pbad = io.take<uint8_t>(n_points); const auto t_pos = io.take<float>(3 * n_points); const auto t_nobs = io.take<int32_t>(n_points);
    const auto t_ref = io.take<int32_t>(n_points); const auto t_rscale = io.take<float>(n_points); const auto t_ooff = io.take<int32_t>(n_points + np_);
    const auto t_okf = io.take<int32_t>(n_obs); const auto t_oidx = io.take<int32_t>(n_obs);
    T.outputs_begin();
    const auto t_counts = io.take<int32_t>(np_ * kPkCounts); const auto t_aslot = io.take<int32_t>(n_list); const auto t_apoint = io.take<int32_t>(n_list);
    const auto t_recent = io.take<int32_t>(n_list); const auto t_nobs_out = io.take<int32_t>(n_points); const auto t_ooff_out = io.take<int32_t>(n_points + np_);
    const auto t_okf_out = io.take<int32_t>(n_obs_out); const auto t_oidx_out = io.take<int32_t>(n_obs_out); const auto t_dkf = io.take<int32_t>(n_points);
    const auto t_didx = io.take<int32_t>(n_points); const auto t_refreshed = io.take<uint8_t>(n_points); const auto t_normals = io.take<float>(3 * n_points);
    const auto t_mn = io.take<float>(n_points); const auto t_mx = io.take<float>(n_points);
    const auto t_ccounts = io.take<int32_t>(np_ * TC2LI_CONNECTIONS_COUNTS); const auto t_cnkf = io.take<int32_t>(n_counter); const auto t_cnw = io.take<int32_t>(n_counter);
    const auto t_orkf = io.take<int32_t>(n_items); const auto t_orw = io.take<int32_t>(n_items); const auto t_tkf = io.take<int32_t>(n_items);
    const auto t_tch = io.take<uint8_t>(n_items); const auto t_choff = io.take<int32_t>(n_items + np_); const auto t_chkf = io.take<int32_t>(n_changed);
    const auto t_chw = io.take<int32_t>(n_changed);
    const auto w_first = work.take<int32_t>(n_points); const auto w_hist = work.take<int32_t>(n_hist); const auto w_tw = work.take<int32_t>(n_items);
    const auto w_ioff = work.take<int32_t>(n_items); const auto w_ifound = work.take<uint8_t>(n_items);
    // the lock is held to the end: the results are read from the space's pinned block
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceProcessKeyframe>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(t_prob, 0, dev.data(), np_); io.put(t_cprob, 0, cdev.data(), np_); io.put(t_kfs, 0, kfs.data(), n_kf);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const Problem& in = problems[p];
        const tc2li_connections_problem& c = in.conn;
        const PkProblemDev& D = dev[p];
        const size_t nk = (size_t)c.n_keyframes, npt = (size_t)c.n_points, no = (size_t)c.obs_offsets[c.n_points], nc = (size_t)c.conn_offsets[c.n_keyframes];
        int32_t* poi = T.host(t_poi) + cdev[p].ordered_off;
        for (int i = 0; i < c.ordered_capacity; ++i) poi[i] = p;
        io.put(t_kflag, D.kf_off, c.kf_flags, nk); io.put(t_crow, cdev[p].conn_row_off, c.conn_offsets, nk + 1);
        io.put(t_ckf, cdev[p].conn_off, c.conn_kf, nc); io.put(t_cw, cdev[p].conn_off, c.conn_weight, nc);
        io.put(t_slot, D.slot_off, c.slot_point, (size_t)c.n_slots);
        io.put(t_ooff, D.point_row_off, c.obs_offsets, npt + 1);
        io.put(t_pbad, D.point_off, c.point_bad, npt); io.put(t_pos, 3 * (size_t)D.point_off, in.positions, 3 * npt); io.put(t_nobs, D.point_off, in.point_nobs, npt);
        io.put(t_ref, D.point_off, in.point_ref_kf, npt); io.put(t_rscale, D.point_off, in.point_ref_level_scale, npt);
        io.put(t_okf, D.obs_off, c.obs_kf, no); io.put(t_oidx, D.obs_off, in.obs_index, no);
    });
    // with tc2li_profile_enable(1) the two copies are bracketed by events like the launches: the report lists them by these names
    hipEvent_t up_a = nullptr, up_b = nullptr, down_a = nullptr, down_b = nullptr;
    const bool timed = prof::g_enabled.load(std::memory_order_relaxed) && prof::acquire("upload(process_new_keyframe)", &up_a, &up_b) &&
                       prof::acquire("download(process_new_keyframe)", &down_a, &down_b);
    if (timed) TC2LI_HIP_CHECK(hipEventRecord(up_a, st));
    TC2LI_HIP_CHECK(T.upload(st));
    if (timed) TC2LI_HIP_CHECK(hipEventRecord(up_b, st));
    PkBatch B{};
    B.n_problems = n_problems; B.n_items = (int)n_list;
    B.problems = T.dev(t_prob); B.kfs = T.dev(t_kfs); B.kf_flags = T.dev(t_kflag); B.slot_point = T.dev(t_slot); B.point_bad = T.dev(t_pbad);
    B.positions = T.dev(t_pos); B.nobs = T.dev(t_nobs); B.ref_kf = T.dev(t_ref); B.ref_scale = T.dev(t_rscale);
    B.obs_offsets = T.dev(t_ooff); B.obs_kf = T.dev(t_okf); B.obs_index = T.dev(t_oidx);
    B.first_slot = T.dev_work(w_first);
    B.counts = T.dev(t_counts); B.associated_slot = T.dev(t_aslot); B.associated_point = T.dev(t_apoint); B.recent = T.dev(t_recent);
    B.nobs_out = T.dev(t_nobs_out); B.obs_offsets_out = T.dev(t_ooff_out); B.obs_kf_out = T.dev(t_okf_out); B.obs_index_out = T.dev(t_oidx_out);
    B.desc_kf = T.dev(t_dkf); B.desc_index = T.dev(t_didx); B.refreshed = T.dev(t_refreshed); B.normals = T.dev(t_normals);
    B.min_dist = T.dev(t_mn); B.max_dist = T.dev(t_mx);
    launch_process_keyframe(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    // UpdateConnections (:348) on the rows k_pkf_associate wrote: they never cross the bus before the vote
    ConnBatch C{};
    C.n_problems = n_problems; C.n_items = (int)n_items;
    C.problems = T.dev(t_cprob); C.problem_of_item = T.dev(t_poi); C.kf_flags = T.dev(t_kflag); C.conn_offsets = T.dev(t_crow); C.conn_kf = T.dev(t_ckf);
    C.conn_weight = T.dev(t_cw); C.slot_point = T.dev(t_slot); C.point_bad = T.dev(t_pbad); C.obs_offsets = T.dev(t_ooff_out); C.obs_kf = T.dev(t_okf_out);
    C.hist = T.dev_work(w_hist); C.touched_weight = T.dev_work(w_tw); C.item_off = T.dev_work(w_ioff); C.item_found = T.dev_work(w_ifound);
    C.counts = T.dev(t_ccounts); C.counter_kf = T.dev(t_cnkf); C.counter_weight = T.dev(t_cnw); C.ordered_kf = T.dev(t_orkf); C.ordered_weight = T.dev(t_orw);
    C.touched_kf = T.dev(t_tkf); C.touched_changed = T.dev(t_tch); C.changed_offsets = T.dev(t_choff); C.changed_kf = T.dev(t_chkf); C.changed_weight = T.dev(t_chw);
    launch_update_connections(C, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    if (timed) TC2LI_HIP_CHECK(hipEventRecord(down_a, st));
    TC2LI_HIP_CHECK(T.download(T.down_from, io.off, st));
    if (timed) TC2LI_HIP_CHECK(hipEventRecord(down_b, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));

    // ---- the host twin for what met the observation limit: the arrays of the slots those problems name come down once ----
    std::vector<int> host_list;
    std::vector<uint8_t> on_host(n_problems, 0);
    for (int p = 0; p < n_problems; ++p) {
        const int32_t* c = T.host(t_counts) + kPkCounts * (size_t)p;
        if (c[kPkStatus] == TC2LI_PROCESS_KEYFRAME_ON_DEVICE) {
            memcpy(problems[p].counts, c, kPkCounts * 4);
            memcpy(problems[p].conn.counts, T.host(t_ccounts) + TC2LI_CONNECTIONS_COUNTS * (size_t)p, TC2LI_CONNECTIONS_COUNTS * 4);
        } else {
            on_host[p] = 1;
            host_list.push_back(p);
        }
    }
    std::vector<Result> results(n_problems);
    std::vector<tc2li_connections_problem> conn(host_list.size());
    if (!host_list.empty()) {
        std::map<int, HostSlot> slots;
        for (const int p : host_list)
            for (int k = 0; k < problems[p].conn.n_keyframes; ++k) {
                const int s = problems[p].kf_slot[k];
                if (s < 0 || slots.count(s)) continue;
                NbKf d{};
                int32_t levels = 0;
                if (!keyframe_store_neighbors(store, s, &d, &levels)) { set_error("%s: slot %d was erased during the call", entry, s); return TC2LI_ERR_INVALID; }
                HostSlot& h = slots[s];
                const size_t n = (size_t)d.n;
                h.desc.resize(std::max<size_t>(32 * n, 4)); h.u_right.resize(std::max<size_t>(n, 1));
                if (n) {
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.desc.data(), d.desc, 32 * n, hipMemcpyDeviceToHost, st));
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.u_right.data(), d.u_right, 4 * n, hipMemcpyDeviceToHost, st));
                }
            }
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
        tracking_pool().parallel_for((int)host_list.size(), [&](int i) {
            const int p = host_list[i];
            const Problem& in = problems[p];
            run_twin(in, [&](int kf) { return slots.find(in.kf_slot[kf])->second.desc.data(); }, slots.find(in.kf_slot[in.conn.current])->second.u_right.data(),
                     results[p]);
            memcpy(in.counts, results[p].counts, sizeof(results[p].counts));
            conn[i] = on_end_state(in, results[p]);
        });
        host_connections(entry, conn.data(), (int)conn.size(), false);
    }
    const int short_of_room = first_short_of_room(problems, n_problems);
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    // ---- every list fits: the results into the problems' arrays ----
    if (!host_list.empty()) {
        rc = host_connections(entry, conn.data(), (int)conn.size(), true);
        if (rc < 0) return rc;
    }
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const Problem& in = problems[p];
        if (on_host[p]) { write_result(in, results[p]); return; }
        const PkProblemDev& D = dev[p];
        const size_t npt = (size_t)in.conn.n_points;
        const int32_t* c = in.counts;
        if (in.associated_slot) io.get(in.associated_slot, t_aslot, D.list_off, (size_t)c[kPkAssociated]);
        if (in.associated_point) io.get(in.associated_point, t_apoint, D.list_off, (size_t)c[kPkAssociated]);
        if (in.recent) io.get(in.recent, t_recent, D.list_off, (size_t)c[kPkRecent]);
        if (in.point_nobs_out) io.get(in.point_nobs_out, t_nobs_out, D.point_off, npt);
        if (in.obs_offsets_out) io.get(in.obs_offsets_out, t_ooff_out, D.point_row_off, npt + 1);
        if (in.obs_kf_out) io.get(in.obs_kf_out, t_okf_out, D.obs_out_off, (size_t)c[kPkObs]);
        if (in.obs_index_out) io.get(in.obs_index_out, t_oidx_out, D.obs_out_off, (size_t)c[kPkObs]);
        if (in.desc_kf) io.get(in.desc_kf, t_dkf, D.point_off, npt);
        if (in.desc_index) io.get(in.desc_index, t_didx, D.point_off, npt);
        if (in.refreshed) io.get(in.refreshed, t_refreshed, D.point_off, npt);
        if (in.normals_out) io.get(in.normals_out, t_normals, 3 * (size_t)D.point_off, 3 * npt);
        if (in.min_distance_out) io.get(in.min_distance_out, t_mn, D.point_off, npt);
        if (in.max_distance_out) io.get(in.max_distance_out, t_mx, D.point_off, npt);
        const tc2li_connections_problem& k = in.conn;
        const ConnProblemDev& E = cdev[p];
        const int32_t* kc = k.counts;
        if (kc[TC2LI_CONNECTIONS_STATUS] == TC2LI_CONNECTIONS_UNCHANGED) return;
        const size_t nc = (size_t)kc[TC2LI_CONNECTIONS_N_COUNTER], no = (size_t)kc[TC2LI_CONNECTIONS_N_ORDERED], ne = (size_t)kc[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES];
        io.get(k.counter_kf, t_cnkf, E.counter_off, nc); io.get(k.counter_weight, t_cnw, E.counter_off, nc);
        io.get(k.ordered_kf, t_orkf, E.ordered_off, no); io.get(k.ordered_weight, t_orw, E.ordered_off, no);
        io.get(k.touched_kf, t_tkf, E.ordered_off, no); io.get(k.touched_changed, t_tch, E.ordered_off, no);
        io.get(k.changed_offsets, t_choff, (size_t)E.ordered_off + p, (size_t)kc[TC2LI_CONNECTIONS_N_CHANGED] + 1);
        io.get(k.changed_kf, t_chkf, E.changed_off, ne); io.get(k.changed_weight, t_chw, E.changed_off, ne);
    });
    return n_problems;
}

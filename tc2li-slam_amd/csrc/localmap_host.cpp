// tc2li_local_map_* (include/tc2li_hip.h): a device-resident mirror of the keyframe-graph pieces Tracking::UpdateLocalKeyFrames /
// UpdateLocalPoints read (SF/src/Tracking.cc:3296-3476), uploaded when the map changes, and the per-frame update on it.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "common.hpp"
#include "localmap_batch_device.hpp"
#include "localmap_device.hpp"
#include "packed_batch.hpp"

using namespace tc2li;

struct tc2li_local_map {
    std::mutex mu;
    int n_keyframes = 0, n_points = 0, total_matches = 0;
    bool has_graph = false;
    DevBuf<uint8_t> d_kf_bad, d_point_bad, d_marked, d_cleared;
    DevBuf<int32_t> d_covis_off, d_covis, d_child_off, d_children, d_parent, d_prev, d_match_off, d_matches, d_obs_off, d_obs_kf;
    DevBuf<int32_t> d_votes, d_kf_list, d_rev_base, d_header, d_first, d_block_counts, d_points, d_frame_points;
    PinnedBuf<int32_t> h_header;
    LocalMapDev dev{};
};

namespace {

// offsets [n + 1] start at 0, never decrease; the values they index lie in [lo, hi).  "" or what is wrong.
std::string csr_fault(const int32_t* off, const int32_t* val, int n, int lo, int hi, const char* what) {
    char msg[160];
    msg[0] = 0;
    if (!off) snprintf(msg, sizeof msg, "map graph: %s offsets are null", what);
    else if (off[0] != 0) snprintf(msg, sizeof msg, "map graph: %s offsets must start at 0", what);
    if (msg[0]) return msg;
    for (int i = 0; i < n; ++i) if (off[i + 1] < off[i]) { snprintf(msg, sizeof msg, "map graph: %s offsets decrease at %d", what, i); return msg; }
    if (off[n] > 0 && !val) { snprintf(msg, sizeof msg, "map graph: %s values are null", what); return msg; }
    for (int k = 0; k < off[n]; ++k) if (val[k] < lo || val[k] >= hi) { snprintf(msg, sizeof msg, "map graph: %s entry %d = %d out of range", what, k, val[k]); return msg; }
    return "";
}

// tc2li_local_map_set_graph's checks of a graph: "" or what is wrong.  Sets no error itself: it also runs on pool threads.
std::string graph_fault(const tc2li_map_graph* g) {
    if (!g || g->n_keyframes < 0 || g->n_points < 0) return "invalid argument";
    const int K = g->n_keyframes, P = g->n_points;
    if (K > 0 && (!g->kf_bad || !g->parent || !g->prev_kf)) return "map graph: null keyframe arrays";
    if (P > 0 && !g->point_bad) return "map graph: null point arrays";
    std::string f = csr_fault(g->covis_offsets, g->covis, K, 0, K, "covisibility");
    if (f.empty()) f = csr_fault(g->child_offsets, g->children, K, 0, K, "children");
    if (f.empty()) f = csr_fault(g->match_offsets, g->matches, K, -1, P, "matches");
    if (f.empty()) f = csr_fault(g->obs_offsets, g->obs_kf, P, 0, K, "observations");
    if (!f.empty()) return f;
    for (int k = 0; k < K; ++k)
        if (g->parent[k] < -1 || g->parent[k] >= K || g->prev_kf[k] < -1 || g->prev_kf[k] >= K) {
            char msg[96];
            snprintf(msg, sizeof msg, "map graph: parent / previous keyframe of %d out of range", k);
            return msg;
        }
    return "";
}

template <typename T>
hipError_t put(DevBuf<T>& d, const T* src, size_t n, hipStream_t st) {
    hipError_t e = d.ensure(n > 0 ? n : 1);
    if (e != hipSuccess || n == 0) return e;
    return hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, st);
}

// The copies of a validated graph into m's buffers on st, and the scratch of the single-map update; m->mu is held.  The mirror is
// adopted (graph_adopt) once the stream has been waited on: until then the caller's arrays are being read.
hipError_t graph_enqueue(tc2li_local_map* m, const tc2li_map_graph* g, hipStream_t st) {
    const int K = g->n_keyframes, P = g->n_points;
#define LM_TRY(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return e_; } while (0)
    LM_TRY(put(m->d_kf_bad, g->kf_bad, K, st)); LM_TRY(put(m->d_point_bad, g->point_bad, P, st));
    LM_TRY(put(m->d_covis_off, g->covis_offsets, (size_t)K + 1, st)); LM_TRY(put(m->d_covis, g->covis, g->covis_offsets[K], st));
    LM_TRY(put(m->d_child_off, g->child_offsets, (size_t)K + 1, st)); LM_TRY(put(m->d_children, g->children, g->child_offsets[K], st));
    LM_TRY(put(m->d_parent, g->parent, K, st)); LM_TRY(put(m->d_prev, g->prev_kf, K, st));
    LM_TRY(put(m->d_match_off, g->match_offsets, (size_t)K + 1, st)); LM_TRY(put(m->d_matches, g->matches, g->match_offsets[K], st));
    LM_TRY(put(m->d_obs_off, g->obs_offsets, (size_t)P + 1, st)); LM_TRY(put(m->d_obs_kf, g->obs_kf, g->obs_offsets[P], st));
    const size_t Kc = std::max(K, 1), Pc = std::max(P, 1);
    LM_TRY(m->d_votes.ensure(Kc)); LM_TRY(m->d_marked.ensure(Kc)); LM_TRY(m->d_kf_list.ensure(Kc));
    LM_TRY(m->d_rev_base.ensure(Kc + 1)); LM_TRY(m->d_header.ensure(4)); LM_TRY(m->d_first.ensure(Pc));
    LM_TRY(m->d_block_counts.ensure((size_t)g->match_offsets[K] / 256 + 2)); LM_TRY(m->d_points.ensure(Pc));
    LM_TRY(m->h_header.ensure(4));
#undef LM_TRY
    return hipSuccess;
}

void graph_adopt(tc2li_local_map* m, const tc2li_map_graph* g) {
    const int K = g->n_keyframes, P = g->n_points;
    m->total_matches = g->match_offsets[K];
    m->n_keyframes = K; m->n_points = P; m->has_graph = true;
    LocalMapDev& d = m->dev;
    d.n_keyframes = K; d.n_points = P; d.kf_bad = m->d_kf_bad.p; d.covis_off = m->d_covis_off.p; d.covis = m->d_covis.p;
    d.child_off = m->d_child_off.p; d.children = m->d_children.p; d.parent = m->d_parent.p; d.prev_kf = m->d_prev.p;
    d.match_off = m->d_match_off.p; d.matches = m->d_matches.p; d.point_bad = m->d_point_bad.p; d.obs_off = m->d_obs_off.p; d.obs_kf = m->d_obs_kf.p;
    d.votes = m->d_votes.p; d.marked = m->d_marked.p; d.kf_list = m->d_kf_list.p; d.rev_base = m->d_rev_base.p; d.header = m->d_header.p;
    d.first_pos = m->d_first.p; d.block_counts = m->d_block_counts.p; d.points = m->d_points.p;
}

}  // namespace

extern "C" {

int tc2li_local_map_create(tc2li_local_map** out) {
    if (!out) { set_error("tc2li_local_map_create: invalid argument"); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    *out = new tc2li_local_map();
    return TC2LI_OK;
}

void tc2li_local_map_destroy(tc2li_local_map* m) { delete m; }

int tc2li_local_map_set_graph(tc2li_local_map* m, const tc2li_map_graph* g, void* stream_) {
    if (!m || !g || g->n_keyframes < 0 || g->n_points < 0) { set_error("tc2li_local_map_set_graph: invalid argument"); return TC2LI_ERR_INVALID; }
    const std::string fault = graph_fault(g);
    if (!fault.empty()) { set_error("%s", fault.c_str()); return TC2LI_ERR_INVALID; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream_;
    std::lock_guard<std::mutex> lk(m->mu);
    TC2LI_HIP_CHECK(graph_enqueue(m, g, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));  // the caller's arrays may go away
    graph_adopt(m, g);
    return TC2LI_OK;
}

int tc2li_local_map_update(tc2li_local_map* m, const int32_t* frame_points, int n_frame_points, int temporal_last_kf,
                           int32_t* local_keyframes, int keyframe_capacity, int32_t* n_local_keyframes, int32_t* reference_kf,
                           int32_t* local_points, int point_capacity, int32_t* n_local_points, uint8_t* frame_point_cleared, void* stream_) {
    if (!m || n_frame_points < 0 || (n_frame_points > 0 && (!frame_points || !frame_point_cleared)) || !local_keyframes || !n_local_keyframes ||
        !reference_kf || !local_points || !n_local_points || keyframe_capacity < 0 || point_capacity < 0) {
        set_error("tc2li_local_map_update: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    std::lock_guard<std::mutex> lk(m->mu);
    if (!m->has_graph) { set_error("tc2li_local_map_update: no graph set"); return TC2LI_ERR_INVALID; }
    if (temporal_last_kf < -1 || temporal_last_kf >= m->n_keyframes) { set_error("tc2li_local_map_update: temporal_last_kf out of range"); return TC2LI_ERR_INVALID; }
    for (int i = 0; i < n_frame_points; ++i)
        if (frame_points[i] < -1 || frame_points[i] >= m->n_points) { set_error("frame point %d = %d out of range", i, frame_points[i]); return TC2LI_ERR_INVALID; }
    *n_local_keyframes = 0; *n_local_points = 0; *reference_kf = -1;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream_;
    const LocalMapDev& d = m->dev;
    const size_t K = m->n_keyframes, P = m->n_points;
    TC2LI_HIP_CHECK(m->d_frame_points.ensure(std::max(n_frame_points, 1))); TC2LI_HIP_CHECK(m->d_cleared.ensure(std::max(n_frame_points, 1)));
    if (K) { TC2LI_HIP_CHECK(hipMemsetAsync(d.votes, 0, K * sizeof(int32_t), st)); TC2LI_HIP_CHECK(hipMemsetAsync(d.marked, 0, K, st)); }
    if (P) TC2LI_HIP_CHECK(hipMemsetAsync(d.first_pos, 0x7f, P * sizeof(int32_t), st));  // 0x7f7f7f7f: beyond any position
    if (n_frame_points) TC2LI_HIP_CHECK(hipMemcpyAsync(m->d_frame_points.p, frame_points, n_frame_points * sizeof(int32_t), hipMemcpyHostToDevice, st));
    launch_local_map_votes(d, m->d_frame_points.p, n_frame_points, m->d_cleared.p, st);
    launch_local_map_keyframes(d, temporal_last_kf, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(m->h_header.p, d.header, 3 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));  // the grid of the point kernels is the length of the concatenated match lists
    const int n_local = m->h_header.p[0], total = m->h_header.p[1];
    *reference_kf = m->h_header.p[2];
    if (n_local > keyframe_capacity) { set_error("%d local keyframes, capacity %d", n_local, keyframe_capacity); return TC2LI_ERR_CAPACITY; }
    int n_pts = 0;
    if (total > 0) {
        launch_local_map_points(d, n_local, total, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipMemcpyAsync(m->h_header.p + 3, d.header + 3, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(hipStreamSynchronize(st));
        n_pts = m->h_header.p[3];
        if (n_pts > point_capacity) { set_error("%d local points, capacity %d", n_pts, point_capacity); return TC2LI_ERR_CAPACITY; }
    }
    if (n_local) TC2LI_HIP_CHECK(hipMemcpyAsync(local_keyframes, d.kf_list, n_local * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (n_pts) TC2LI_HIP_CHECK(hipMemcpyAsync(local_points, d.points, n_pts * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (n_frame_points) TC2LI_HIP_CHECK(hipMemcpyAsync(frame_point_cleared, m->d_cleared.p, n_frame_points, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    *n_local_keyframes = n_local;
    *n_local_points = n_pts;
    return n_pts;
}

const int32_t* tc2li_local_map_device_points(const tc2li_local_map* m) { return m ? m->dev.points : nullptr; }

}  // extern "C"

// ---- UpdateLocalMap for many sequences in one call (include/tc2li_hip.h "tc2li_local_map_update_batch") ----------------------------------
namespace {

typedef tc2li_local_map_update_problem LmProblem;

// the first failure in item order as "<entry>: <noun> <i>: <what>"; fault_of(i) runs on the tracking pool and returns "" or what is wrong
template <class FaultOf>
int refuse_first(const char* entry, const char* noun, int n, FaultOf fault_of) {
    std::vector<std::string> fault(n);
    tracking_pool().parallel_for(n, [&](int i) { fault[i] = fault_of(i); });
    for (int i = 0; i < n; ++i)
        if (!fault[i].empty()) {
            set_error("%s: %s %d: %s", entry, noun, i, fault[i].c_str());
            return TC2LI_ERR_INVALID;
        }
    return 0;
}

// what does not depend on the graph
const char* problem_fault(const LmProblem& in, bool device) {
    if (device ? !in.map : !in.graph) return device ? "null map" : "null graph";
    if (!in.counts) return "null counts";
    if (in.n_frame_points < 0) return "negative n_frame_points";
    if (in.keyframe_capacity < 0 || in.point_capacity < 0) return "negative capacity";
    if (in.n_frame_points && (!in.frame_points || !in.frame_point_cleared)) return "null frame_points or frame_point_cleared";
    if ((in.keyframe_capacity && !in.local_keyframes) || (in.point_capacity && !in.local_points)) return "null local_keyframes or local_points";
    return "";
}

// the frame against a graph of n_keyframes and n_points
const char* frame_fault(const LmProblem& in, int n_keyframes, int n_points) {
    if (in.temporal_last_kf < -1 || in.temporal_last_kf >= n_keyframes) return "temporal_last_kf out of range";
    for (int i = 0; i < in.n_frame_points; ++i)
        if (in.frame_points[i] < -1 || in.frame_points[i] >= n_points) return "a frame point is out of range";
    return "";
}

bool fits(const LmProblem& in, const int32_t* counts) {
    return counts[TC2LI_LOCAL_MAP_N_KEYFRAMES] <= in.keyframe_capacity && counts[TC2LI_LOCAL_MAP_N_POINTS] <= in.point_capacity;
}

int capacity_error(const char* entry, const LmProblem* problems, int p) {
    const LmProblem& in = problems[p];
    set_error("%s: problem %d needs room for %d local keyframes and %d local points and has %d and %d", entry, p, in.counts[TC2LI_LOCAL_MAP_N_KEYFRAMES],
              in.counts[TC2LI_LOCAL_MAP_N_POINTS], in.keyframe_capacity, in.point_capacity);
    return TC2LI_ERR_CAPACITY;
}

struct LocalMapLists {
    std::vector<int32_t> keyframes, points;
    std::vector<uint8_t> cleared;
    int32_t counts[TC2LI_LOCAL_MAP_COUNTS];
};

// Tracking::UpdateLocalKeyFrames + UpdateLocalPoints on the graph itself, in the reference's order of steps
void walk_local_map(const tc2li_map_graph& g, const LmProblem& in, LocalMapLists& out) {
    const int K = g.n_keyframes;
    std::vector<int32_t> votes(K, 0);
    std::vector<uint8_t> marked(K, 0), seen(g.n_points, 0);
    out.cleared.assign(in.n_frame_points, 0);
    int n_cleared = 0;
    for (int i = 0; i < in.n_frame_points; ++i) {                                       // :3329-3347
        const int p = in.frame_points[i];
        if (p < 0) continue;
        if (g.point_bad[p]) { out.cleared[i] = 1; ++n_cleared; continue; }              // :3345
        for (int k = g.obs_offsets[p]; k < g.obs_offsets[p + 1]; ++k) ++votes[g.obs_kf[k]];
    }
    std::vector<int32_t>& list = out.keyframes;
    int most = 0, reference = -1;
    for (int kf = 0; kf < K; ++kf) {                                                    // :3382-3397
        if (!votes[kf] || g.kf_bad[kf]) continue;
        if (votes[kf] > most) { most = votes[kf]; reference = kf; }
        list.push_back(kf);
        marked[kf] = 1;
    }
    const size_t n_voted = list.size();
    auto push = [&](int kf) { list.push_back(kf); marked[kf] = 1; };
    for (size_t j = 0; j < n_voted; ++j) {                                              // :3400-3451: the voted keyframes only
        if (list.size() > 80) break;                                                    // :3404
        const int kf = list[j];
        const int ce = std::min(g.covis_offsets[kf + 1], g.covis_offsets[kf] + 10);     // GetBestCovisibilityKeyFrames(10)
        for (int k = g.covis_offsets[kf]; k < ce; ++k)
            if (!g.kf_bad[g.covis[k]] && !marked[g.covis[k]]) { push(g.covis[k]); break; }
        for (int k = g.child_offsets[kf]; k < g.child_offsets[kf + 1]; ++k)
            if (!g.kf_bad[g.children[k]] && !marked[g.children[k]]) { push(g.children[k]); break; }
        const int par = g.parent[kf];
        if (par >= 0 && !marked[par]) { push(par); break; }                             // :3441-3450: no isBad(), and the break leaves the loop
    }
    if (in.temporal_last_kf >= 0 && list.size() < 80) {                                 // :3453-3469
        int t = in.temporal_last_kf;
        for (int i = 0; i < 20 && t >= 0; ++i)
            if (!marked[t]) { push(t); t = g.prev_kf[t]; }                              // a step only after a push
    }
    for (size_t j = list.size(); j-- > 0;) {                                            // :3296-3323: keyframes backwards, slots forwards
        const int kf = list[j];
        for (int k = g.match_offsets[kf]; k < g.match_offsets[kf + 1]; ++k) {
            const int p = g.matches[k];
            if (p < 0 || seen[p] || g.point_bad[p]) continue;
            out.points.push_back(p);
            seen[p] = 1;
        }
    }
    std::fill(out.counts, out.counts + TC2LI_LOCAL_MAP_COUNTS, 0);
    out.counts[TC2LI_LOCAL_MAP_N_KEYFRAMES] = (int32_t)list.size();
    out.counts[TC2LI_LOCAL_MAP_N_VOTED] = (int32_t)n_voted;
    out.counts[TC2LI_LOCAL_MAP_REFERENCE_KF] = reference;
    out.counts[TC2LI_LOCAL_MAP_N_POINTS] = (int32_t)out.points.size();
    out.counts[TC2LI_LOCAL_MAP_N_CLEARED] = n_cleared;
}

template <class T>
void copy_out(T* dst, const T* src, size_t n) {
    if (n) memcpy(dst, src, n * sizeof(T));
}

// the problem that names a map an earlier problem named, or -1; *first = that earlier problem
template <class MapOf>
int second_use(int n, MapOf map_of, int* first) {
    std::vector<int> order(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return map_of(a) != map_of(b) ? std::less<const void*>()(map_of(a), map_of(b)) : a < b; });
    int found = -1;
    for (int i = 1; i < n; ++i)
        if (map_of(order[i]) == map_of(order[i - 1]) && (found < 0 || order[i] < found)) { found = order[i]; *first = order[i - 1]; }
    return found;
}

// the mutexes of the maps, taken in address order (two calls that share maps cannot wait for each other in a ring)
struct MapLocks {
    std::vector<std::unique_lock<std::mutex>> held;
    template <class MapOf>
    MapLocks(int n, MapOf map_of) {
        std::vector<tc2li_local_map*> maps(n);
        for (int i = 0; i < n; ++i) maps[i] = map_of(i);
        std::sort(maps.begin(), maps.end(), std::less<tc2li_local_map*>());
        for (tc2li_local_map* m : maps) held.emplace_back(m->mu);
    }
};

// the lists of a device call come down into pinned memory of the size that was found
struct LocalMapBatchSpace : PackedSpace {
    PinnedBuf<int32_t> h_lists;
};

}  // namespace

extern "C" {

int tc2li_local_map_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_local_map_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kLmbLdsKeyframes; out[1] = kLmbPointGroups; out[2] = kLmbThreads;
    return 3;
}

int tc2li_host_local_map_update_batch(const tc2li_local_map_update_problem* problems, int n_problems) {
    const char* entry = "tc2li_host_local_map_update_batch";
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    const int rc = refuse_first(entry, "problem", n_problems, [&](int p) -> std::string {
        const LmProblem& in = problems[p];
        const char* f = problem_fault(in, false);
        if (f[0]) return f;
        std::string g = graph_fault(in.graph);
        if (!g.empty()) return g;
        return frame_fault(in, in.graph->n_keyframes, in.graph->n_points);
    });
    if (rc < 0) return rc;
    std::vector<LocalMapLists> lists(n_problems);
    tracking_pool().parallel_for(n_problems, [&](int p) { walk_local_map(*problems[p].graph, problems[p], lists[p]); });
    int short_of_room = -1;
    for (int p = 0; p < n_problems; ++p) {
        memcpy(problems[p].counts, lists[p].counts, sizeof lists[p].counts);
        if (short_of_room < 0 && !fits(problems[p], lists[p].counts)) short_of_room = p;
    }
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const LmProblem& in = problems[p];
        copy_out(in.local_keyframes, lists[p].keyframes.data(), lists[p].keyframes.size());
        copy_out(in.local_points, lists[p].points.data(), lists[p].points.size());
        copy_out(in.frame_point_cleared, lists[p].cleared.data(), lists[p].cleared.size());
    });
    return n_problems;
}

int tc2li_local_map_update_batch(const tc2li_local_map_update_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_local_map_update_batch";
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    int rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) { return problem_fault(problems[p], true); }));
    if (rc < 0) return rc;
    int first = -1;
    const int second = second_use(n_problems, [&](int p) { return problems[p].map; }, &first);
    if (second >= 0) {
        set_error("%s: problem %d: names the map of problem %d; the two would share its place in the batch", entry, second, first);
        return TC2LI_ERR_INVALID;
    }
    MapLocks locks(n_problems, [&](int p) { return problems[p].map; });
    rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) {
        const tc2li_local_map* m = problems[p].map;
        return m->has_graph ? frame_fault(problems[p], m->n_keyframes, m->n_points) : "the map has no graph";
    }));
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // where every problem's rows start in the batch's tables
    std::vector<LmbProblem> dev(n_problems);
    size_t n_fp = 0, n_keys = 0, n_votes = 0, n_kf = 0, n_lists = 0;
    for (int p = 0; p < n_problems; ++p) {
        const LmProblem& in = problems[p];
        const tc2li_local_map* m = in.map;
        LmbProblem& d = dev[p];
        memset(&d, 0, sizeof d);
        d.map = m->dev;
        d.fp_off = (int32_t)n_fp; d.n_fp = in.n_frame_points; d.temporal_last_kf = in.temporal_last_kf;
        d.key_off = (int32_t)n_keys;
        d.vote_off = m->n_keyframes > kLmbLdsKeyframes ? (int32_t)n_votes : -1;
        d.list_off = (int32_t)n_kf;
        n_fp += in.n_frame_points; n_keys += m->n_points; n_kf += m->n_keyframes;
        if (d.vote_off >= 0) n_votes += m->n_keyframes;
        n_lists += (size_t)m->n_keyframes + std::min(m->n_points, m->total_matches);   // a list never holds a keyframe or a point twice
        if (std::max(std::max(n_fp, n_keys), std::max(n_kf + p + 1, n_lists)) > kMaxRows) return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    // one buffer [inputs | counts, where the lists start, cleared flags]; the work buffer starts with what the kernels expect zeroed
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const Table<LmbProblem> t_prob = io.take<LmbProblem>(np);
    const Table<int32_t> t_fp = io.take<int32_t>(n_fp);
    T.outputs_begin();
    const Table<int32_t> t_counts = io.take<int32_t>(np * TC2LI_LOCAL_MAP_COUNTS), t_seg = io.take<int32_t>(np + 1);
    const Table<uint8_t> t_cleared = io.take<uint8_t>(n_fp);
    const Table<int32_t> t_keys = work.take<int32_t>(n_keys), t_votes = work.take<int32_t>(n_votes);
    const Table<uint8_t> t_marks = work.take<uint8_t>(n_votes);
    const size_t zeroed = work.off;
    const Table<int32_t> t_kfl = work.take<int32_t>(n_kf), t_rev = work.take<int32_t>(n_kf + np), t_info = work.take<int32_t>(2 * np),
                         t_bcount = work.take<int32_t>(np * kLmbPointGroups), t_bbase = work.take<int32_t>(np * kLmbPointGroups),
                         t_lists = work.take<int32_t>(n_lists);
    LocalMapBatchSpace& S = shutdown_owned<LocalMapBatchSpace, kSpaceLocalMap>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(t_prob, 0, dev.data(), np);
    tracking_pool().parallel_for(n_problems, [&](int p) { io.put(t_fp, dev[p].fp_off, problems[p].frame_points, problems[p].n_frame_points); });
    TC2LI_HIP_CHECK(T.upload(st));
    TC2LI_HIP_CHECK(T.zero_work(zeroed, st));
    LmbBatch B{};
    B.n_problems = n_problems;
    B.problems = T.dev(t_prob); B.frame_points = T.dev(t_fp);
    B.keys = T.dev_work(t_keys); B.votes = T.dev_work(t_votes); B.marks = T.dev_work(t_marks);
    B.kf_list = T.dev_work(t_kfl); B.rev_base = T.dev_work(t_rev); B.info = T.dev_work(t_info);
    B.block_counts = T.dev_work(t_bcount); B.block_base = T.dev_work(t_bbase); B.lists = T.dev_work(t_lists);
    B.counts = T.dev(t_counts); B.seg = T.dev(t_seg); B.cleared = T.dev(t_cleared);
    launch_local_map_batch(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));   // the sizes: what the second download is as long as
    const int short_of_room = copy_counts(problems, n_problems, T.host(t_counts), TC2LI_LOCAL_MAP_COUNTS, fits);
    if (short_of_room >= 0) return capacity_error(entry, problems, short_of_room);
    const int32_t* seg = T.host(t_seg);
    const size_t n_found = (size_t)seg[n_problems];
    if (n_found > n_lists) {
        set_error("%s: the lists hold %zu entries, more than the %zu the graphs allow", entry, n_found, n_lists);
        return TC2LI_ERR_HIP;
    }
    if (n_found) {
        TC2LI_HIP_CHECK(S.h_lists.ensure(n_found));
        TC2LI_HIP_CHECK(hipMemcpyAsync(S.h_lists.p, B.lists, n_found * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
    }
    const int32_t* found = S.h_lists.p;
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const LmProblem& in = problems[p];
        const size_t nk = (size_t)in.counts[TC2LI_LOCAL_MAP_N_KEYFRAMES], npts = (size_t)in.counts[TC2LI_LOCAL_MAP_N_POINTS];
        copy_out(in.local_keyframes, found + seg[p], nk);
        copy_out(in.local_points, found + seg[p] + nk, npts);
        io.get(in.frame_point_cleared, t_cleared, dev[p].fp_off, in.n_frame_points);
    });
    return n_problems;
}

int tc2li_local_map_set_graph_batch(tc2li_local_map* const* maps, const tc2li_map_graph* graphs, int n_maps, void* stream) {
    const char* entry = "tc2li_local_map_set_graph_batch";
    if (n_maps < 0 || (n_maps && (!maps || !graphs))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    const int rc = refuse_first(entry, "map", n_maps, [&](int i) -> std::string { return maps[i] ? graph_fault(&graphs[i]) : std::string("null map"); });
    if (rc < 0) return rc;
    int first = -1;
    const int second = second_use(n_maps, [&](int i) { return maps[i]; }, &first);
    if (second >= 0) {
        set_error("%s: map %d: is map %d again", entry, second, first);
        return TC2LI_ERR_INVALID;
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_maps == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    MapLocks locks(n_maps, [&](int i) { return maps[i]; });
    for (int i = 0; i < n_maps; ++i) TC2LI_HIP_CHECK(graph_enqueue(maps[i], &graphs[i], st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));  // one wait for all: the caller's arrays may go away
    for (int i = 0; i < n_maps; ++i) graph_adopt(maps[i], &graphs[i]);
    return n_maps;
}

}  // extern "C"

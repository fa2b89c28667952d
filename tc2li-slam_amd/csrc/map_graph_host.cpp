// tc2li_map_graph_* / tc2li_host_map_graph_apply (include/tc2li_hip.h "the map graph resident on the device"): the slab and its layout,
// the host's mirror of per-row metadata (row counts, the store slot and the slot row of every keyframe row, the observation total -- no
// table), the check of an edit log against it, the log's way to the device (map_graph_kernels.hip) and the plain sequential twin that
// defines the result.  MgLease (map_graph_host.hpp) is how a gather reads the graph (ba_window_host.cpp).
// tc2li_map_graph_*connections* (tc2li_hip.h "the covisibility graph on the resident map graph"): the two CSRs of the connections in an
// allocation of their own, their mirror (generation, rows covered, entries), the check of tables set from the host, the records of an
// update or an erase for connections_kernels.hip, and the two host twins.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <utility>
#include <vector>

#include "common.hpp"
#include "map_graph_host.hpp"
#include "packed_batch.hpp"
#include "window_gather_host.hpp"

using namespace tc2li;

namespace {

struct SeqMeta {
    bool set = false;
    int generation = 0;                      // the observation CSR that is current
    int n_kf = 0, n_pt = 0, n_obs = 0;
    int applies = -1;
    int64_t apply_bytes = 0, gather_bytes = 0;
    std::vector<int32_t> store_slot;         // [n_kf]
    std::vector<int32_t> n_keys;             // [n_kf] the most keypoints the row's store slot held at a set or an apply: every resident obs_index is below it
    std::vector<int32_t> slot_off{0};        // [n_kf + 1] slot_offsets
    // the connections (tc2li_map_graph_connections_*): the generation of both CSRs that is current, the keyframe rows their offsets
    // cover (the rows appended since are empty), their entries
    int conn_generation = 0, conn_rows = 0, n_weight = 0, n_ordered = 0;
    int conn_updates = 0;
    int64_t conn_bytes = 0;
    void clear_connections() { conn_generation = conn_rows = n_weight = n_ordered = conn_updates = 0; conn_bytes = 0; }
};

}  // namespace

struct tc2li_map_graph_handle {
    tc2li_keyframe_store* store = nullptr;
    int n_seq = 0;
    int32_t cap[TC2LI_MAP_GRAPH_CAPACITIES] = {0, 0, 0, 0};
    uint8_t* slab = nullptr;
    MgTables T{};
    std::vector<SeqMeta> seq;
    std::mutex mu;                           // one call at a time on a graph
    PinnedBuf<uint8_t> h_up;                 // what a call stages: the tables of a set, the records, edits and values of an apply
    PinnedBuf<CopyTask> tasks;
    DevBuf<uint8_t> d_up;
    DevBuf<int32_t> d_totals;
    PinnedBuf<int32_t> h_totals;
    // a commit: [records | the erase logs the device writes] and [totals | status words]; its own, because the logs of host-path windows
    // go through the apply's buffers in the same call
    PinnedBuf<uint8_t> h_commit;
    DevBuf<uint8_t> d_commit;
    DevBuf<int32_t> d_commit_words;
    PinnedBuf<int32_t> h_commit_words;
    // the connections: their own allocation, made by the reserve; the records, scratch and words of an update or an erase
    uint8_t* conn_slab = nullptr;
    MgConnTables C{};
    PinnedBuf<MgConnDev> h_conn;
    DevBuf<MgConnDev> d_conn;
    DevBuf<uint8_t> d_conn_scratch;
    DevBuf<int32_t> d_conn_words;
    PinnedBuf<int32_t> h_conn_words;
};

namespace {

// ---- the check of a log ----------------------------------------------------------------------------------------------------------------
// The sizes a log meets and what they are after it.  store_slot / slot_off: of the rows resident now.
struct LogSizes {
    int n_kf, n_pt, n_obs;
    const int32_t* store_slot;
    const int32_t* slot_off;
};
struct LogAfter {
    int n_kf = 0, n_pt = 0, n_slot = 0, n_adds = 0;
    std::vector<int32_t> new_store_slot, new_slots;   // of the rows the log appends
};

bool is_byte(double v) { return v >= 0 && v <= 255 && v == std::floor(v); }

// 0, or the code with *what set.  The first edit in log order that fails decides; the observation bound comes after all edits.
// store_n: the keypoints of every store slot (-1: empty), or NULL for the host twin, which has no store.
int check_log(const LogSizes& m, const tc2li_map_graph_edit* edits, int n_edits, const double* values, int n_values, const int32_t* cap,
              const std::vector<int32_t>* store_n, LogAfter* r, const char** what) {
    r->n_kf = m.n_kf; r->n_pt = m.n_pt; r->n_slot = m.slot_off[m.n_kf]; r->n_adds = 0;
    auto fail = [&](int code, const char* w) { *what = w; return code; };
    auto has_values = [&](int32_t off, int count) { return off >= 0 && (int64_t)off + count <= n_values; };
    auto slots_of = [&](int row) { return row < m.n_kf ? m.slot_off[row + 1] - m.slot_off[row] : r->new_slots[row - m.n_kf]; };
    auto store_slot_of = [&](int row) { return row < m.n_kf ? m.store_slot[row] : r->new_store_slot[row - m.n_kf]; };
    if (n_edits < 0 || n_values < 0 || (n_edits && !edits) || (n_values && !values)) return fail(TC2LI_ERR_INVALID, "null or negative log");
    for (int e = 0; e < n_edits; ++e) {
        const tc2li_map_graph_edit& ed = edits[e];
        switch (ed.op) {
            case TC2LI_MAP_GRAPH_ADD_KEYFRAME: {
                if (ed.a < 0 || (store_n && (ed.a >= (int)store_n->size() || (*store_n)[ed.a] < 0))) return fail(TC2LI_ERR_INVALID, "a store slot is empty or out of range");
                if (ed.b < 0) return fail(TC2LI_ERR_INVALID, "a negative slot count");
                if (!has_values(ed.c, 9)) return fail(TC2LI_ERR_INVALID, "a values offset out of range");
                const double id = values[ed.c];
                if (!(std::fabs(id) <= 9007199254740992.0) || id != std::floor(id) || !is_byte(values[ed.c + 1])) return fail(TC2LI_ERR_INVALID, "a keyframe id or flags that is no integer");
                if (r->n_kf + 1 > cap[TC2LI_MAP_GRAPH_KEYFRAMES]) return fail(TC2LI_ERR_CAPACITY, "keyframe rows beyond the capacity");
                if ((int64_t)r->n_slot + ed.b > cap[TC2LI_MAP_GRAPH_SLOTS]) return fail(TC2LI_ERR_CAPACITY, "slot entries beyond the capacity");
                r->new_store_slot.push_back(ed.a); r->new_slots.push_back(ed.b);
                ++r->n_kf; r->n_slot += ed.b;
                break;
            }
            case TC2LI_MAP_GRAPH_SET_KEYFRAME_FLAGS:
                if (ed.a < 0 || ed.a >= r->n_kf) return fail(TC2LI_ERR_INVALID, "a keyframe row out of range or named before its append");
                if (ed.b < 0 || ed.b > 255) return fail(TC2LI_ERR_INVALID, "flags outside a byte");
                break;
            case TC2LI_MAP_GRAPH_SET_POSE:
                if (ed.a < 0 || ed.a >= r->n_kf) return fail(TC2LI_ERR_INVALID, "a keyframe row out of range or named before its append");
                if (!has_values(ed.b, 7)) return fail(TC2LI_ERR_INVALID, "a values offset out of range");
                break;
            case TC2LI_MAP_GRAPH_ADD_POINT:
                if (ed.a < 0 || ed.a > 255) return fail(TC2LI_ERR_INVALID, "flags outside a byte");
                if (!has_values(ed.b, 3)) return fail(TC2LI_ERR_INVALID, "a values offset out of range");
                if (r->n_pt + 1 > cap[TC2LI_MAP_GRAPH_POINTS]) return fail(TC2LI_ERR_CAPACITY, "point rows beyond the capacity");
                ++r->n_pt;
                break;
            case TC2LI_MAP_GRAPH_SET_POINT_FLAGS:
                if (ed.a < 0 || ed.a >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point row out of range or named before its append");
                if (ed.b < 0 || ed.b > 255) return fail(TC2LI_ERR_INVALID, "flags outside a byte");
                break;
            case TC2LI_MAP_GRAPH_SET_POSITION:
                if (ed.a < 0 || ed.a >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point row out of range or named before its append");
                if (!has_values(ed.b, 3)) return fail(TC2LI_ERR_INVALID, "a values offset out of range");
                break;
            case TC2LI_MAP_GRAPH_SET_SLOT:
                if (ed.a < 0 || ed.a >= r->n_kf) return fail(TC2LI_ERR_INVALID, "a keyframe row out of range or named before its append");
                if (ed.b < 0 || ed.b >= slots_of(ed.a)) return fail(TC2LI_ERR_INVALID, "a slot out of range");
                if (ed.c < -1 || ed.c >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point below -1, out of range or named before its append");
                break;
            case TC2LI_MAP_GRAPH_ADD_OBSERVATION:
                if (ed.a < 0 || ed.a >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point row out of range or named before its append");
                if (ed.b < 0 || ed.b >= r->n_kf) return fail(TC2LI_ERR_INVALID, "a keyframe row out of range or named before its append");
                if (ed.c < -1 || (store_n && ed.c >= (*store_n)[store_slot_of(ed.b)])) return fail(TC2LI_ERR_INVALID, "an observation index outside the keypoints of the observer's slot");
                ++r->n_adds;
                break;
            case TC2LI_MAP_GRAPH_ERASE_OBSERVATION:
                if (ed.a < 0 || ed.a >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point row out of range or named before its append");
                if (ed.b < 0 || ed.b >= r->n_kf) return fail(TC2LI_ERR_INVALID, "a keyframe row out of range or named before its append");
                break;
            case TC2LI_MAP_GRAPH_CLEAR_OBSERVATIONS:
                if (ed.a < 0 || ed.a >= r->n_pt) return fail(TC2LI_ERR_INVALID, "a point row out of range or named before its append");
                break;
            default: return fail(TC2LI_ERR_INVALID, "an unknown op");
        }
    }
    // the host cannot know whether an ADD grows a row: conservative, and exact to state
    if ((int64_t)m.n_obs + r->n_adds > cap[TC2LI_MAP_GRAPH_OBSERVATIONS]) return fail(TC2LI_ERR_CAPACITY, "observation entries resident + ADD_OBSERVATION edits beyond the capacity");
    return 0;
}

const char* tables_fault(const tc2li_map_graph_tables& t) {
    if (t.n_keyframes < 0 || t.n_points < 0) return "negative size";
    if (!t.slot_offsets || !t.obs_offsets) return "null slot_offsets or obs_offsets";
    if ((t.n_keyframes && (!t.kf_slot || !t.kf_id || !t.kf_flags || !t.poses7)) || (t.n_points && (!t.point_flags || !t.positions)))
        return "null kf_slot, kf_id, kf_flags, poses7, point_flags or positions";
    return "";
}

bool sequence_ok(const tc2li_map_graph_handle* g, int s) { return s >= 0 && s < g->n_seq; }

MgSequenceView view_of(const tc2li_map_graph_handle* g, int s) {
    const SeqMeta& m = g->seq[s];
    MgSequenceView v{};
    v.n_kf = m.n_kf; v.n_points = m.n_pt; v.n_slot = m.slot_off[m.n_kf]; v.n_obs = m.n_obs;
    v.t_kf = s * g->cap[0]; v.t_slot = s * g->cap[1]; v.t_point = s * g->cap[2];
    v.t_obs = (2 * s + m.generation) * g->cap[3];
    v.slot_row = s * (g->cap[0] + 1); v.obs_row = (2 * s + m.generation) * (g->cap[2] + 1);
    v.kf_store_slot = m.store_slot.data(); v.kf_keys = m.n_keys.data();
    v.ord_row = (2 * s + m.conn_generation) * (g->cap[0] + 1); v.conn_rows = m.conn_rows; v.n_ordered = m.n_ordered;
    return v;
}

}  // namespace

// ---- handle ----------------------------------------------------------------------------------------------------------------------------
extern "C" int tc2li_map_graph_limits(int32_t* out, int capacity) {
    if (!out || capacity < 6) {
        set_error("tc2li_map_graph_limits: room for 6 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kMgLdsRow; out[1] = kMgThreads; out[2] = kMgThreads; out[3] = (int32_t)sizeof(MgApplyDev); out[4] = (int32_t)sizeof(BawProblemDev); out[5] = (int32_t)kMgMaxWalk;
    return 6;
}

extern "C" int tc2li_map_graph_create(tc2li_keyframe_store* store, int n_sequences, const int32_t* capacities, tc2li_map_graph_handle** out) {
    const char* me = "tc2li_map_graph_create";
    if (!out || !store || !capacities || n_sequences < 1) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    *out = nullptr;
    for (int c = 0; c < TC2LI_MAP_GRAPH_CAPACITIES; ++c)
        if (capacities[c] < 1 || 2 * (int64_t)n_sequences * ((int64_t)capacities[c] + 1) > (int64_t)kMaxRows) {
            set_error("%s: a capacity below 1, or a table of all sequences beyond 2^31 rows", me);
            return TC2LI_ERR_INVALID;
        }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    std::unique_ptr<tc2li_map_graph_handle> G(new tc2li_map_graph_handle());
    G->store = store; G->n_seq = n_sequences;
    memcpy(G->cap, capacities, sizeof(G->cap));
    const size_t S = (size_t)n_sequences, K = (size_t)capacities[0], L = (size_t)capacities[1], P = (size_t)capacities[2], O = (size_t)capacities[3];
    Packer slab;
    const size_t o_slot = slab.take(S * K * 4), o_id = slab.take(S * K * 8), o_flags = slab.take(S * K), o_pose = slab.take(S * K * 56);
    const size_t o_srow = slab.take(S * (K + 1) * 4), o_spt = slab.take(S * L * 4), o_pflags = slab.take(S * P), o_pos = slab.take(S * P * 24);
    const size_t o_orow = slab.take(2 * S * (P + 1) * 4), o_okf = slab.take(2 * S * O * 4), o_oidx = slab.take(2 * S * O * 4);
    const size_t o_head = slab.take(S * P * 4), o_last = slab.take(S * P * 4), o_len = slab.take(S * P * 4), o_stage = slab.take(S * P * 4);
    const size_t o_touched = slab.take(S * P * 4), o_skf = slab.take(S * O * 4), o_sidx = slab.take(S * O * 4);
    TC2LI_HIP_CHECK(hipMalloc((void**)&G->slab, slab.off));
    uint8_t* b = G->slab;
    MgTables& T = G->T;
    T.kf_slot = (int32_t*)(b + o_slot); T.kf_id = (int64_t*)(b + o_id); T.kf_flags = b + o_flags; T.poses7 = (double*)(b + o_pose);
    T.slot_offsets = (int32_t*)(b + o_srow); T.slot_point = (int32_t*)(b + o_spt); T.point_flags = b + o_pflags; T.positions = (double*)(b + o_pos);
    T.obs_offsets = (int32_t*)(b + o_orow); T.obs_kf = (int32_t*)(b + o_okf); T.obs_index = (int32_t*)(b + o_oidx);
    T.pt_head = (int32_t*)(b + o_head); T.pt_last = (int32_t*)(b + o_last); T.pt_len = (int32_t*)(b + o_len); T.pt_stage = (int32_t*)(b + o_stage);
    T.touched = (int32_t*)(b + o_touched); T.stage_kf = (int32_t*)(b + o_skf); T.stage_index = (int32_t*)(b + o_sidx);
    T.cap_kf = capacities[0]; T.cap_slot = capacities[1]; T.cap_pt = capacities[2]; T.cap_obs = capacities[3];
    G->seq.assign(S, SeqMeta{});
    *out = G.release();
    return 0;
}

extern "C" int tc2li_map_graph_destroy(tc2li_map_graph_handle* g) {
    if (!g) return 0;
    if (g->slab) (void)hipFree(g->slab);
    if (g->conn_slab) (void)hipFree(g->conn_slab);
    delete g;
    return 0;
}

extern "C" int tc2li_map_graph_info(tc2li_map_graph_handle* g, int sequence, int64_t* out, int capacity) {
    if (!g || !sequence_ok(g, sequence) || !out || capacity < TC2LI_MAP_GRAPH_INFO_FIELDS) { set_error("tc2li_map_graph_info: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    const SeqMeta& m = g->seq[sequence];
    out[TC2LI_MAP_GRAPH_INFO_KEYFRAMES] = m.n_kf; out[TC2LI_MAP_GRAPH_INFO_POINTS] = m.n_pt; out[TC2LI_MAP_GRAPH_INFO_SLOTS] = m.slot_off[m.n_kf];
    out[TC2LI_MAP_GRAPH_INFO_OBSERVATIONS] = m.n_obs; out[TC2LI_MAP_GRAPH_INFO_APPLIES] = m.applies;
    out[TC2LI_MAP_GRAPH_INFO_APPLY_BYTES] = m.apply_bytes; out[TC2LI_MAP_GRAPH_INFO_GATHER_BYTES] = m.gather_bytes;
    return TC2LI_MAP_GRAPH_INFO_FIELDS;
}

// ---- set -------------------------------------------------------------------------------------------------------------------------------
extern "C" int tc2li_map_graph_set_batch(tc2li_map_graph_handle* g, const int32_t* sequences, const tc2li_map_graph_tables* tables, int n, void* stream) {
    const char* me = "tc2li_map_graph_set_batch";
    if (!g || n < 0 || (n && (!sequences || !tables))) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(g->mu);
    SlotTable slots;
    BawStore where{};
    slot_table_from_store(g->store, &slots, &where);
    std::vector<uint8_t> named(g->n_seq, 0);
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_tables& t = tables[i];
        if (!sequence_ok(g, sequences[i]) || named[sequences[i]]) { set_error("%s: sequence %d out of range or named twice", me, sequences[i]); return TC2LI_ERR_INVALID; }
        named[sequences[i]] = 1;
        const char* what = tables_fault(t);
        if (!what[0]) what = validate_graph(t, slots, INT_MAX, [](int) { return ""; }, [] { return ""; });
        if (what[0]) { set_error("%s: sequence %d: %s", me, sequences[i], what); return TC2LI_ERR_INVALID; }
        const int n_slot = t.slot_offsets[t.n_keyframes], n_obs = t.obs_offsets[t.n_points];
        if (t.n_keyframes > g->cap[0] || n_slot > g->cap[1] || t.n_points > g->cap[2] || n_obs > g->cap[3]) {
            set_error("%s: sequence %d has %d keyframes, %d slots, %d points and %d observations; the capacities are %d, %d, %d and %d", me, sequences[i],
                      t.n_keyframes, n_slot, t.n_points, n_obs, g->cap[0], g->cap[1], g->cap[2], g->cap[3]);
            return TC2LI_ERR_CAPACITY;
        }
        bytes += 16 * 11 + (size_t)t.n_keyframes * (4 + 8 + 1 + 56 + 4) + 4 + (size_t)n_slot * 4 + (size_t)t.n_points * (1 + 24 + 4) + 4 + (size_t)n_obs * 8;
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    TC2LI_HIP_CHECK(g->h_up.ensure(bytes));
    TC2LI_HIP_CHECK(g->tasks.ensure(11 * (size_t)n));
    size_t at = 0, n_tasks = 0, max_bytes = 0;
    auto stage = [&](void* dst, const void* src, size_t b) {
        if (!b) return;
        memcpy(g->h_up.p + at, src, b);
        g->tasks.p[n_tasks++] = CopyTask{dst, g->h_up.p + at, b};
        max_bytes = std::max(max_bytes, b);
        at += (b + 15) & ~(size_t)15;
    };
    const MgTables& T = g->T;
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_tables& t = tables[i];
        const size_t s = (size_t)sequences[i], nk = (size_t)t.n_keyframes, np = (size_t)t.n_points;
        const size_t n_slot = (size_t)t.slot_offsets[nk], n_obs = (size_t)t.obs_offsets[np];
        stage(T.kf_slot + s * T.cap_kf, t.kf_slot, nk * 4); stage(T.kf_id + s * T.cap_kf, t.kf_id, nk * 8); stage(T.kf_flags + s * T.cap_kf, t.kf_flags, nk);
        stage(T.poses7 + s * T.cap_kf * 7, t.poses7, nk * 56); stage(T.slot_offsets + s * ((size_t)T.cap_kf + 1), t.slot_offsets, (nk + 1) * 4);
        stage(T.slot_point + s * T.cap_slot, t.slot_point, n_slot * 4); stage(T.point_flags + s * T.cap_pt, t.point_flags, np);
        stage(T.positions + s * T.cap_pt * 3, t.positions, np * 24);
        stage(T.obs_offsets + 2 * s * ((size_t)T.cap_pt + 1), t.obs_offsets, (np + 1) * 4);   // generation 0
        stage(T.obs_kf + 2 * s * T.cap_obs, t.obs_kf, n_obs * 4); stage(T.obs_index + 2 * s * T.cap_obs, t.obs_index, n_obs * 4);
    }
    launch_copy_tasks(g->tasks.p, (int)n_tasks, max_bytes, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(stream_wait_blocking(st));   // resident on return: a gather on any stream may follow
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_tables& t = tables[i];
        SeqMeta& m = g->seq[sequences[i]];
        m.set = true; m.generation = 0; m.n_kf = t.n_keyframes; m.n_pt = t.n_points; m.n_obs = t.obs_offsets[t.n_points];
        m.applies = 0; m.apply_bytes = 0; m.gather_bytes = 0;
        m.clear_connections();
        m.store_slot.assign(t.kf_slot, t.kf_slot + t.n_keyframes);
        m.n_keys.resize(t.n_keyframes);
        for (int k = 0; k < t.n_keyframes; ++k) m.n_keys[k] = slots.n[t.kf_slot[k]];
        m.slot_off.assign(t.slot_offsets, t.slot_offsets + t.n_keyframes + 1);
    }
    return n;
}

// ---- apply -----------------------------------------------------------------------------------------------------------------------------
namespace {
// the caller holds g->mu
int apply_locked(const char* me, tc2li_map_graph_handle* g, const tc2li_map_graph_delta* deltas, int n, void* stream) {
    SlotTable slots;
    BawStore where{};
    slot_table_from_store(g->store, &slots, &where);
    // ---- every check before any device work: a refused call leaves the graph as it was ----
    std::vector<uint8_t> named(g->n_seq, 0);
    std::vector<LogAfter> after(n);
    size_t n_edits = 0, n_values = 0;
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_delta& d = deltas[i];
        if (!sequence_ok(g, d.sequence) || named[d.sequence]) { set_error("%s: sequence %d out of range or named twice", me, d.sequence); return TC2LI_ERR_INVALID; }
        named[d.sequence] = 1;
        const SeqMeta& m = g->seq[d.sequence];
        if (!m.set) { set_error("%s: sequence %d was never set", me, d.sequence); return TC2LI_ERR_INVALID; }
        const LogSizes sizes{m.n_kf, m.n_pt, m.n_obs, m.store_slot.data(), m.slot_off.data()};
        const char* what = "";
        const int rc = check_log(sizes, d.edits, d.n_edits, d.values, d.n_values, g->cap, &slots.n, &after[i], &what);
        if (rc < 0) { set_error("%s: sequence %d: %s", me, d.sequence, what); return rc; }
        // what the workgroup of this log will read to find every touched row's edits (map_graph_device.hpp, kMgMaxWalk)
        std::vector<int32_t> first(after[i].n_pt, -1), last(after[i].n_pt, -1);
        for (int e = 0; e < d.n_edits; ++e) {
            const int op = d.edits[e].op;
            if (op != TC2LI_MAP_GRAPH_ADD_OBSERVATION && op != TC2LI_MAP_GRAPH_ERASE_OBSERVATION && op != TC2LI_MAP_GRAPH_CLEAR_OBSERVATIONS) continue;
            if (first[d.edits[e].a] < 0) first[d.edits[e].a] = e;
            last[d.edits[e].a] = e;
        }
        int64_t walk = 0;
        for (int p = 0; p < after[i].n_pt; ++p) walk += first[p] < 0 ? 0 : last[p] - first[p] + 1;
        if (walk > kMgMaxWalk) {
            set_error("%s: sequence %d: the observation edits of single points lie %lld log entries apart in sum, the limit is %lld; split the log or keep a point's edits together", me,
                      d.sequence, (long long)walk, (long long)kMgMaxWalk);
            return TC2LI_ERR_CAPACITY;
        }
        n_edits += (size_t)d.n_edits; n_values += (size_t)d.n_values;
        if (n_edits > kMaxRows || n_values > kMaxRows) return too_many_rows(me, i);
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // ---- one upload: [records | edits | values], nothing else ----
    const size_t o_edits = (size_t)n * sizeof(MgApplyDev), o_values = o_edits + n_edits * sizeof(tc2li_map_graph_edit), bytes = o_values + n_values * 8;
    TC2LI_HIP_CHECK(g->h_up.ensure(bytes)); TC2LI_HIP_CHECK(g->d_up.ensure(bytes));
    TC2LI_HIP_CHECK(g->d_totals.ensure(n)); TC2LI_HIP_CHECK(g->h_totals.ensure(n));
    MgApplyDev* rec = reinterpret_cast<MgApplyDev*>(g->h_up.p);
    size_t e_at = 0, v_at = 0;
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_delta& d = deltas[i];
        const SeqMeta& m = g->seq[d.sequence];
        MgApplyDev r{};
        r.sequence = d.sequence; r.generation = m.generation; r.n_kf = m.n_kf; r.n_points = m.n_pt; r.n_slot = m.slot_off[m.n_kf]; r.n_obs = m.n_obs;
        r.edit_off = (int32_t)e_at; r.n_edits = d.n_edits; r.value_off = (int32_t)v_at; r.n_points_new = after[i].n_pt;
        rec[i] = r;
        if (d.n_edits) memcpy(g->h_up.p + o_edits + e_at * sizeof(tc2li_map_graph_edit), d.edits, (size_t)d.n_edits * sizeof(tc2li_map_graph_edit));
        if (d.n_values) memcpy(g->h_up.p + o_values + v_at * 8, d.values, (size_t)d.n_values * 8);
        e_at += (size_t)d.n_edits; v_at += (size_t)d.n_values;
    }
    TC2LI_HIP_CHECK(hipMemcpyAsync(g->d_up.p, g->h_up.p, bytes, hipMemcpyHostToDevice, st));
    MgApplyBatch B{};
    B.T = g->T; B.n = n; B.deltas = reinterpret_cast<const MgApplyDev*>(g->d_up.p);
    B.edits = reinterpret_cast<const tc2li_map_graph_edit*>(g->d_up.p + o_edits); B.values = reinterpret_cast<const double*>(g->d_up.p + o_values);
    B.totals = g->d_totals.p;
    launch_map_graph_apply(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(g->h_totals.p, g->d_totals.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));   // 4 bytes per sequence
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_delta& d = deltas[i];
        SeqMeta& m = g->seq[d.sequence];
        const LogAfter& a = after[i];
        m.generation ^= 1; m.n_kf = a.n_kf; m.n_pt = a.n_pt; m.n_obs = g->h_totals.p[i];
        m.store_slot.insert(m.store_slot.end(), a.new_store_slot.begin(), a.new_store_slot.end());
        m.n_keys.resize(m.store_slot.size(), 0);
        for (size_t k = 0; k < m.store_slot.size(); ++k) m.n_keys[k] = std::max(m.n_keys[k], slots.n[m.store_slot[k]]);   // what this log's indices were checked against
        for (int32_t s : a.new_slots) m.slot_off.push_back(m.slot_off.back() + s);
        ++m.applies;
        m.apply_bytes = (int64_t)(sizeof(MgApplyDev) + (size_t)d.n_edits * sizeof(tc2li_map_graph_edit) + (size_t)d.n_values * 8);
    }
    return n;
}
}  // namespace

extern "C" int tc2li_map_graph_apply_batch(tc2li_map_graph_handle* g, const tc2li_map_graph_delta* deltas, int n, void* stream) {
    const char* me = "tc2li_map_graph_apply_batch";
    if (!g || n < 0 || (n && !deltas)) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(g->mu);
    return apply_locked(me, g, deltas, n, stream);
}

// ---- download --------------------------------------------------------------------------------------------------------------------------
namespace {
// the caller holds g->mu
int download_locked(const char* me, tc2li_map_graph_handle* g, int sequence, tc2li_map_graph_tables* out, const int32_t* capacities, int32_t* counts) {
    const SeqMeta& m = g->seq[sequence];
    const MgSequenceView v = view_of(g, sequence);
    counts[0] = v.n_kf; counts[1] = v.n_slot; counts[2] = v.n_points; counts[3] = v.n_obs;
    for (int c = 0; c < 4; ++c)
        if (capacities[c] < counts[c]) { set_error("%s: the arrays are too small", me); return TC2LI_ERR_CAPACITY; }
    if (!out->slot_offsets || !out->obs_offsets || (v.n_kf && (!out->kf_slot || !out->kf_id || !out->kf_flags || !out->poses7)) || (v.n_slot && !out->slot_point) ||
        (v.n_points && (!out->point_flags || !out->positions)) || (v.n_obs && (!out->obs_kf || !out->obs_index))) {
        set_error("%s: null array", me);
        return TC2LI_ERR_INVALID;
    }
    out->n_keyframes = v.n_kf; out->n_points = v.n_points;
    if (!m.set) { out->slot_offsets[0] = 0; out->obs_offsets[0] = 0; return 0; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const MgTables& T = g->T;
    auto get = [](void* dst, const void* src, size_t b) { return b ? hipMemcpy(dst, src, b, hipMemcpyDeviceToHost) : hipSuccess; };
    const size_t nk = (size_t)v.n_kf, np = (size_t)v.n_points;
    TC2LI_HIP_CHECK(get(out->kf_slot, T.kf_slot + v.t_kf, nk * 4)); TC2LI_HIP_CHECK(get(out->kf_id, T.kf_id + v.t_kf, nk * 8));
    TC2LI_HIP_CHECK(get(out->kf_flags, T.kf_flags + v.t_kf, nk)); TC2LI_HIP_CHECK(get(out->poses7, T.poses7 + (size_t)v.t_kf * 7, nk * 56));
    TC2LI_HIP_CHECK(get(out->slot_offsets, T.slot_offsets + v.slot_row, (nk + 1) * 4)); TC2LI_HIP_CHECK(get(out->slot_point, T.slot_point + v.t_slot, (size_t)v.n_slot * 4));
    TC2LI_HIP_CHECK(get(out->point_flags, T.point_flags + v.t_point, np)); TC2LI_HIP_CHECK(get(out->positions, T.positions + (size_t)v.t_point * 3, np * 24));
    TC2LI_HIP_CHECK(get(out->obs_offsets, T.obs_offsets + v.obs_row, (np + 1) * 4)); TC2LI_HIP_CHECK(get(out->obs_kf, T.obs_kf + v.t_obs, (size_t)v.n_obs * 4));
    TC2LI_HIP_CHECK(get(out->obs_index, T.obs_index + v.t_obs, (size_t)v.n_obs * 4));
    return 0;
}
}  // namespace

extern "C" int tc2li_map_graph_download(tc2li_map_graph_handle* g, int sequence, tc2li_map_graph_tables* out, const int32_t* capacities, int32_t* counts) {
    const char* me = "tc2li_map_graph_download";
    if (!g || !sequence_ok(g, sequence) || !out || !capacities || !counts) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    return download_locked(me, g, sequence, out, capacities, counts);
}

// ---- the connections -------------------------------------------------------------------------------------------------------------------
namespace {

// "" or what tc2li_map_graph_set_connections_batch refuses; rows: the keyframe rows the sequence has
const char* connections_fault(const tc2li_map_graph_connections& c, int rows) {
    if (c.n_keyframes < 0 || c.n_keyframes > rows) return "n_keyframes negative or beyond the sequence's keyframe rows";
    if (!c.conn_offsets || !c.ord_offsets) return "null conn_offsets or ord_offsets";
    if (!ascending(c.conn_offsets, c.n_keyframes) || !ascending(c.ord_offsets, c.n_keyframes)) return "offsets do not ascend from 0";
    const int nk = c.n_keyframes, nw = c.conn_offsets[nk], no = c.ord_offsets[nk];
    if ((nw && (!c.conn_kf || !c.conn_weight)) || (no && (!c.ord_kf || !c.ord_weight))) return "null conn_kf, conn_weight, ord_kf or ord_weight";
    for (int r = 0; r < nk; ++r)
        for (int j = c.conn_offsets[r]; j < c.conn_offsets[r + 1]; ++j) {
            if (c.conn_kf[j] < 0 || c.conn_kf[j] >= nk) return "a keyframe of a weight row is out of range";
            if (j > c.conn_offsets[r] && c.conn_kf[j] <= c.conn_kf[j - 1]) return "a weight row does not ascend strictly by keyframe";
            if (c.conn_kf[j] == r) return "a weight row names its own keyframe";
        }
    std::vector<int32_t> seen(nk, -1);
    for (int r = 0; r < nk; ++r)
        for (int j = c.ord_offsets[r]; j < c.ord_offsets[r + 1]; ++j) {
            const int k = c.ord_kf[j];
            if (k < 0 || k >= nk) return "a keyframe of an ordered row is out of range";
            if (k == r) return "an ordered row names its own keyframe";
            if (seen[k] == r) return "an ordered row names a keyframe twice";
            seen[k] = r;
        }
    return "";
}

bool reserved(const char* me, const tc2li_map_graph_handle* g) {
    if (g && g->conn_slab) return true;
    set_error("%s: null graph, or tc2li_map_graph_connections_reserve was not called", me);
    return false;
}

// The state of the host twins: a keyframe's weights in map order and its lists.
struct HostConnections {
    std::vector<std::vector<std::pair<int32_t, int32_t>>> weights, ordered;   // (keyframe, weight)
    void read(const tc2li_map_graph_connections& c, int rows) {
        weights.assign(rows, {}); ordered.assign(rows, {});
        for (int r = 0; r < c.n_keyframes; ++r) {
            for (int j = c.conn_offsets[r]; j < c.conn_offsets[r + 1]; ++j) weights[r].emplace_back(c.conn_kf[j], c.conn_weight[j]);
            for (int j = c.ord_offsets[r]; j < c.ord_offsets[r + 1]; ++j) ordered[r].emplace_back(c.ord_kf[j], c.ord_weight[j]);
        }
    }
    // KeyFrame::UpdateBestCovisibles (:216-238) of row k
    void best_covisibles(int k, const uint8_t* kf_flags) {
        std::vector<uint64_t> keys;
        for (const auto& e : weights[k])
            if (!(kf_flags[e.first] & 1)) keys.push_back(conn::key(e.second, e.first));   // :229
        std::sort(keys.begin(), keys.end());                                               // :224
        ordered[k].clear();
        for (size_t i = keys.size(); i-- > 0;) ordered[k].emplace_back(conn::key_kf(keys[i]), conn::key_weight(keys[i]));   // :231-232
    }
    // 0, or TC2LI_ERR_*; sizes is written either way
    int write(const char* me, tc2li_map_graph_connections* out, const int32_t* capacities, int32_t* sizes) const {
        size_t nw = 0, no = 0;
        for (const auto& r : weights) nw += r.size();
        for (const auto& r : ordered) no += r.size();
        sizes[0] = (int32_t)nw; sizes[1] = (int32_t)no;
        if ((int64_t)nw > capacities[0] || (int64_t)no > capacities[1]) {
            set_error("%s: %zu weight and %zu ordered entries, the capacities are %d and %d", me, nw, no, capacities[0], capacities[1]);
            return TC2LI_ERR_CAPACITY;
        }
        if (!out->conn_offsets || !out->ord_offsets || (nw && (!out->conn_kf || !out->conn_weight)) || (no && (!out->ord_kf || !out->ord_weight))) {
            set_error("%s: null output array", me);
            return TC2LI_ERR_INVALID;
        }
        int32_t a = 0, b = 0;
        for (size_t r = 0; r < weights.size(); ++r) {
            out->conn_offsets[r] = a; out->ord_offsets[r] = b;
            for (const auto& e : weights[r]) { out->conn_kf[a] = e.first; out->conn_weight[a++] = e.second; }
            for (const auto& e : ordered[r]) { out->ord_kf[b] = e.first; out->ord_weight[b++] = e.second; }
        }
        out->conn_offsets[weights.size()] = a; out->ord_offsets[weights.size()] = b;
        out->n_keyframes = (int32_t)weights.size();
        return 0;
    }
};

// what both twins check of their inputs
int twin_check(const char* me, const tc2li_map_graph_tables* t, const tc2li_map_graph_connections* in, int row, const tc2li_map_graph_connections* out,
               const int32_t* capacities, const int32_t* sizes) {
    if (!t || !in || !out || !capacities || !sizes) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    const char* what = tables_fault(*t);
    if (!what[0] && (!ascending(t->slot_offsets, t->n_keyframes) || !ascending(t->obs_offsets, t->n_points))) what = "offsets do not ascend from 0";
    if (!what[0]) {
        const int n_slot = t->slot_offsets[t->n_keyframes], n_obs = t->obs_offsets[t->n_points];
        if ((n_slot && !t->slot_point) || (n_obs && !t->obs_kf)) what = "null slot_point or obs_kf";
        for (int i = 0; !what[0] && i < n_slot; ++i)
            if (t->slot_point[i] < -1 || t->slot_point[i] >= t->n_points) what = "slot_point out of range";
        for (int i = 0; !what[0] && i < n_obs; ++i)
            if (t->obs_kf[i] < 0 || t->obs_kf[i] >= t->n_keyframes) what = "obs_kf out of range";
    }
    if (!what[0]) what = connections_fault(*in, t->n_keyframes);
    if (!what[0] && (row < 0 || row >= t->n_keyframes)) what = "the keyframe row is out of range";
    if (what[0]) { set_error("%s: %s", me, what); return TC2LI_ERR_INVALID; }
    return 0;
}

}  // namespace

extern "C" int tc2li_host_map_graph_update_connections(const tc2li_map_graph_tables* t, const tc2li_map_graph_connections* in, int32_t current,
                                                       int first_connection, int64_t init_kf_id, tc2li_map_graph_connections* out,
                                                       const int32_t* capacities, int32_t* sizes, int32_t* counts) {
    const char* me = "tc2li_host_map_graph_update_connections";
    if (!counts) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    int rc = twin_check(me, t, in, current, out, capacities, sizes);
    if (rc < 0) return rc;
    const int nk = t->n_keyframes, np = t->n_points;
    HostConnections H;
    H.read(*in, nk);
    // the call as a tc2li_connections_problem: the table above "Inputs" in the header
    std::vector<int32_t> conn_off(nk + 1, 0), conn_kf, conn_weight;
    for (int r = 0; r < nk; ++r) {
        for (const auto& e : H.weights[r]) { conn_kf.push_back(e.first); conn_weight.push_back(e.second); }
        conn_off[r + 1] = (int32_t)conn_kf.size();
    }
    std::vector<uint8_t> point_bad(np + 1, 0);
    for (int p = 0; p < np; ++p) point_bad[p] = t->point_flags[p] & 1;
    const size_t room = conn_kf.size() + (size_t)nk + 1;
    std::vector<int32_t> counter_kf(nk + 1), counter_weight(nk + 1), ordered_kf(nk + 1), ordered_weight(nk + 1), touched_kf(nk + 1), changed_off(nk + 2),
        changed_kf(room), changed_weight(room);
    std::vector<uint8_t> touched_changed(nk + 1);
    tc2li_connections_problem pr{};
    pr.kf_flags = t->kf_flags; pr.conn_offsets = conn_off.data(); pr.conn_kf = conn_kf.data(); pr.conn_weight = conn_weight.data();
    pr.slot_point = t->slot_point + t->slot_offsets[current]; pr.n_slots = t->slot_offsets[current + 1] - t->slot_offsets[current];
    pr.point_bad = point_bad.data(); pr.obs_offsets = t->obs_offsets; pr.obs_kf = t->obs_kf;
    pr.counts = counts; pr.counter_kf = counter_kf.data(); pr.counter_weight = counter_weight.data(); pr.ordered_kf = ordered_kf.data();
    pr.ordered_weight = ordered_weight.data(); pr.touched_kf = touched_kf.data(); pr.touched_changed = touched_changed.data();
    pr.changed_offsets = changed_off.data(); pr.changed_kf = changed_kf.data(); pr.changed_weight = changed_weight.data();
    pr.n_keyframes = nk; pr.n_points = np; pr.current = current;
    pr.counter_capacity = nk; pr.ordered_capacity = nk; pr.changed_capacity = (int32_t)room - 1;
    pr.first_connection = first_connection ? 1 : 0; pr.is_init_kf = t->kf_id[current] == init_kf_id ? 1 : 0;
    rc = tc2li_host_update_connections_batch(&pr, 1);
    if (rc < 0) return rc;
    if (counts[TC2LI_CONNECTIONS_STATUS] == TC2LI_CONNECTIONS_UPDATED) {
        auto& own = H.weights[current];
        own.clear();                                                                                       // :473
        for (int i = 0; i < counts[TC2LI_CONNECTIONS_N_COUNTER]; ++i) own.emplace_back(counter_kf[i], counter_weight[i]);
        H.ordered[current].clear();                                                                        // :474-475
        for (int i = 0; i < counts[TC2LI_CONNECTIONS_N_ORDERED]; ++i) H.ordered[current].emplace_back(ordered_kf[i], ordered_weight[i]);
        for (int i = 0, c = 0; i < counts[TC2LI_CONNECTIONS_N_ORDERED]; ++i) {                             // AddConnection (:201-214)
            const int k = touched_kf[i];
            const int32_t* w = std::lower_bound(counter_kf.data(), counter_kf.data() + counts[TC2LI_CONNECTIONS_N_COUNTER], k);
            const int32_t weight = counter_weight[w - counter_kf.data()];
            auto& row = H.weights[k];
            auto it = std::lower_bound(row.begin(), row.end(), current, [](const std::pair<int32_t, int32_t>& x, int32_t v) { return x.first < v; });
            if (it != row.end() && it->first == current) it->second = weight;
            else row.insert(it, std::make_pair(current, weight));
            if (!touched_changed[i]) continue;                                                             // :209-210
            H.ordered[k].clear();
            for (int j = changed_off[c]; j < changed_off[c + 1]; ++j) H.ordered[k].emplace_back(changed_kf[j], changed_weight[j]);
            ++c;
        }
    }
    rc = H.write(me, out, capacities, sizes);
    return rc < 0 ? rc : counts[TC2LI_CONNECTIONS_STATUS];
}

extern "C" int tc2li_host_map_graph_erase_connections(const tc2li_map_graph_tables* t, const tc2li_map_graph_connections* in, int32_t row,
                                                      tc2li_map_graph_connections* out, const int32_t* capacities, int32_t* sizes) {
    const char* me = "tc2li_host_map_graph_erase_connections";
    const int rc = twin_check(me, t, in, row, out, capacities, sizes);
    if (rc < 0) return rc;
    HostConnections H;
    H.read(*in, t->n_keyframes);
    for (const auto& e : H.weights[row]) {                                                                 // :600-603
        auto& theirs = H.weights[e.first];
        auto it = std::lower_bound(theirs.begin(), theirs.end(), row, [](const std::pair<int32_t, int32_t>& x, int32_t v) { return x.first < v; });
        if (it == theirs.end() || it->first != row) continue;                                              // :703: bUpdate stays false
        theirs.erase(it);                                                                                  // :705
        H.best_covisibles(e.first, t->kf_flags);                                                           // :710-711
    }
    H.weights[row].clear();                                                                                // :617
    H.ordered[row].clear();                                                                                // :618
    return H.write(me, out, capacities, sizes);
}

extern "C" int tc2li_map_graph_connections_limits(int32_t* out, int capacity) {
    if (!out || capacity < 2) { set_error("tc2li_map_graph_connections_limits: room for 2 values is needed"); return TC2LI_ERR_INVALID; }
    out[0] = (int32_t)sizeof(MgConnDev); out[1] = kMgcStatusWords * 4;
    return 2;
}

extern "C" int tc2li_map_graph_connections_reserve(tc2li_map_graph_handle* g, int entries) {
    const char* me = "tc2li_map_graph_connections_reserve";
    if (!g) { set_error("%s: null graph", me); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    if (g->conn_slab) { set_error("%s: called twice", me); return TC2LI_ERR_INVALID; }
    if (entries < 1 || 2 * (int64_t)g->n_seq * ((int64_t)entries + 1) > (int64_t)kMaxRows) {
        set_error("%s: a capacity below 1, or tables of all sequences beyond 2^31 entries", me);
        return TC2LI_ERR_INVALID;
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const size_t S = (size_t)g->n_seq, K = (size_t)g->cap[0], E = (size_t)entries;
    Packer slab;
    const size_t o_wrow = slab.take(2 * S * (K + 1) * 4), o_wkf = slab.take(2 * S * E * 4), o_ww = slab.take(2 * S * E * 4);
    const size_t o_orow = slab.take(2 * S * (K + 1) * 4), o_okf = slab.take(2 * S * E * 4), o_ow = slab.take(2 * S * E * 4);
    TC2LI_HIP_CHECK(hipMalloc((void**)&g->conn_slab, slab.off));
    uint8_t* b = g->conn_slab;
    MgConnTables& C = g->C;
    C.conn_offsets = (int32_t*)(b + o_wrow); C.conn_kf = (int32_t*)(b + o_wkf); C.conn_weight = (int32_t*)(b + o_ww);
    C.ord_offsets = (int32_t*)(b + o_orow); C.ord_kf = (int32_t*)(b + o_okf); C.ord_weight = (int32_t*)(b + o_ow);
    C.cap_e = entries;
    for (SeqMeta& m : g->seq) m.clear_connections();
    return 0;
}

extern "C" int tc2li_map_graph_connections_info(tc2li_map_graph_handle* g, int sequence, int64_t* out, int capacity) {
    const char* me = "tc2li_map_graph_connections_info";
    if (!reserved(me, g)) return TC2LI_ERR_INVALID;
    if (!sequence_ok(g, sequence) || !out || capacity < TC2LI_MAP_GRAPH_CONNECTIONS_INFO_FIELDS) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    const SeqMeta& m = g->seq[sequence];
    out[TC2LI_MAP_GRAPH_CONNECTIONS_WEIGHT_ENTRIES] = m.n_weight; out[TC2LI_MAP_GRAPH_CONNECTIONS_ORDERED_ENTRIES] = m.n_ordered;
    out[TC2LI_MAP_GRAPH_CONNECTIONS_UPDATES] = m.conn_updates; out[TC2LI_MAP_GRAPH_CONNECTIONS_UPDATE_BYTES] = m.conn_bytes;
    return TC2LI_MAP_GRAPH_CONNECTIONS_INFO_FIELDS;
}

extern "C" int tc2li_map_graph_set_connections_batch(tc2li_map_graph_handle* g, const int32_t* sequences, const tc2li_map_graph_connections* tables, int n,
                                                     void* stream) {
    const char* me = "tc2li_map_graph_set_connections_batch";
    if (!reserved(me, g)) return TC2LI_ERR_INVALID;
    if (n < 0 || (n && (!sequences || !tables))) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(g->mu);
    std::vector<uint8_t> named(g->n_seq, 0);
    size_t bytes = 0;
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_connections& c = tables[i];
        if (!sequence_ok(g, sequences[i]) || named[sequences[i]] || !g->seq[sequences[i]].set) {
            set_error("%s: sequence %d out of range, never set or named twice", me, sequences[i]);
            return TC2LI_ERR_INVALID;
        }
        named[sequences[i]] = 1;
        const char* what = connections_fault(c, g->seq[sequences[i]].n_kf);
        if (what[0]) { set_error("%s: sequence %d: %s", me, sequences[i], what); return TC2LI_ERR_INVALID; }
        const int nw = c.conn_offsets[c.n_keyframes], no = c.ord_offsets[c.n_keyframes];
        if (nw > g->C.cap_e || no > g->C.cap_e) {
            set_error("%s: sequence %d has %d weight and %d ordered entries; the reserve is %d", me, sequences[i], nw, no, g->C.cap_e);
            return TC2LI_ERR_CAPACITY;
        }
        bytes += 16 * 6 + 2 * ((size_t)c.n_keyframes + 1) * 4 + 2 * ((size_t)nw + (size_t)no) * 4;
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    TC2LI_HIP_CHECK(g->h_up.ensure(bytes));
    TC2LI_HIP_CHECK(g->tasks.ensure(6 * (size_t)n));
    size_t at = 0, n_tasks = 0, max_bytes = 0;
    auto stage = [&](void* dst, const void* src, size_t b) {
        if (!b) return;
        memcpy(g->h_up.p + at, src, b);
        g->tasks.p[n_tasks++] = CopyTask{dst, g->h_up.p + at, b};
        max_bytes = std::max(max_bytes, b);
        at += (b + 15) & ~(size_t)15;
    };
    const MgConnTables& C = g->C;
    const size_t rows = (size_t)g->cap[0] + 1, E = (size_t)C.cap_e;
    for (int i = 0; i < n; ++i) {                                                    // into generation 0
        const tc2li_map_graph_connections& c = tables[i];
        const size_t s = (size_t)sequences[i], nk = (size_t)c.n_keyframes, nw = (size_t)c.conn_offsets[nk], no = (size_t)c.ord_offsets[nk];
        stage(C.conn_offsets + 2 * s * rows, c.conn_offsets, (nk + 1) * 4); stage(C.conn_kf + 2 * s * E, c.conn_kf, nw * 4); stage(C.conn_weight + 2 * s * E, c.conn_weight, nw * 4);
        stage(C.ord_offsets + 2 * s * rows, c.ord_offsets, (nk + 1) * 4); stage(C.ord_kf + 2 * s * E, c.ord_kf, no * 4); stage(C.ord_weight + 2 * s * E, c.ord_weight, no * 4);
    }
    launch_copy_tasks(g->tasks.p, (int)n_tasks, max_bytes, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    for (int i = 0; i < n; ++i) {
        const tc2li_map_graph_connections& c = tables[i];
        SeqMeta& m = g->seq[sequences[i]];
        m.clear_connections();
        m.conn_rows = c.n_keyframes; m.n_weight = c.conn_offsets[c.n_keyframes]; m.n_ordered = c.ord_offsets[c.n_keyframes];
    }
    return n;
}

extern "C" int tc2li_map_graph_download_connections(tc2li_map_graph_handle* g, int sequence, tc2li_map_graph_connections* out, const int32_t* capacities,
                                                    int32_t* counts) {
    const char* me = "tc2li_map_graph_download_connections";
    if (!reserved(me, g)) return TC2LI_ERR_INVALID;
    if (!sequence_ok(g, sequence) || !out || !capacities || !counts) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(g->mu);
    const SeqMeta& m = g->seq[sequence];
    counts[0] = m.n_weight; counts[1] = m.n_ordered;
    if (capacities[0] < counts[0] || capacities[1] < counts[1]) { set_error("%s: the arrays are too small", me); return TC2LI_ERR_CAPACITY; }
    if (!out->conn_offsets || !out->ord_offsets || (m.n_weight && (!out->conn_kf || !out->conn_weight)) || (m.n_ordered && (!out->ord_kf || !out->ord_weight))) {
        set_error("%s: null array", me);
        return TC2LI_ERR_INVALID;
    }
    out->n_keyframes = m.n_kf;
    if (m.conn_rows > 0 || m.n_weight || m.n_ordered) {
        if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
        const MgConnTables& C = g->C;
        const size_t gen = 2 * (size_t)sequence + m.conn_generation, rows = (size_t)g->cap[0] + 1, E = (size_t)C.cap_e;
        auto get = [](void* dst, const void* src, size_t b) { return b ? hipMemcpy(dst, src, b, hipMemcpyDeviceToHost) : hipSuccess; };
        TC2LI_HIP_CHECK(get(out->conn_offsets, C.conn_offsets + gen * rows, ((size_t)m.conn_rows + 1) * 4));
        TC2LI_HIP_CHECK(get(out->ord_offsets, C.ord_offsets + gen * rows, ((size_t)m.conn_rows + 1) * 4));
        TC2LI_HIP_CHECK(get(out->conn_kf, C.conn_kf + gen * E, (size_t)m.n_weight * 4)); TC2LI_HIP_CHECK(get(out->conn_weight, C.conn_weight + gen * E, (size_t)m.n_weight * 4));
        TC2LI_HIP_CHECK(get(out->ord_kf, C.ord_kf + gen * E, (size_t)m.n_ordered * 4)); TC2LI_HIP_CHECK(get(out->ord_weight, C.ord_weight + gen * E, (size_t)m.n_ordered * 4));
    }
    for (int k = m.conn_rows; k <= m.n_kf; ++k) { out->conn_offsets[k] = m.n_weight; out->ord_offsets[k] = m.n_ordered; }   // the rows appended since: empty
    return 0;
}

namespace {
// An update (first_connection / init_kf_id given) or an erase of the connections; the caller has checked the plain arguments.
int connections_call(const char* me, tc2li_map_graph_handle* g, const int32_t* sequences, const int32_t* rows, const uint8_t* first_connection,
                     const int64_t* init_kf_id, int n, int32_t* counts_out, int mode, void* stream) {
    std::lock_guard<std::mutex> lk(g->mu);
    if (n > 65535) { set_error("%s: at most 65535 sequences in one call", me); return TC2LI_ERR_INVALID; }
    std::vector<uint8_t> named(g->n_seq, 0);
    int max_kf = 0;
    for (int i = 0; i < n; ++i) {
        if (!sequence_ok(g, sequences[i]) || named[sequences[i]] || !g->seq[sequences[i]].set) {
            set_error("%s: sequence %d out of range, never set or named twice", me, sequences[i]);
            return TC2LI_ERR_INVALID;
        }
        named[sequences[i]] = 1;
        const SeqMeta& m = g->seq[sequences[i]];
        if (rows[i] < 0 || rows[i] >= m.n_kf) { set_error("%s: sequence %d: keyframe row %d is out of range", me, sequences[i], rows[i]); return TC2LI_ERR_INVALID; }
        max_kf = std::max(max_kf, m.n_kf);
    }
    const size_t N = (size_t)n, K = (size_t)g->cap[0], E = (size_t)g->C.cap_e;
    if (N * (E + K + 1) > kMaxRows) return too_many_rows(me, n - 1);
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // scratch that can hold the largest lists of every sequence: nothing in it outlives the call
    Packer work;
    const size_t o_prob = work.take(N * sizeof(ConnProblemDev)), o_cnkf = work.take(N * K * 4), o_cnw = work.take(N * K * 4), o_okf = work.take(N * K * 4),
                 o_ow = work.take(N * K * 4), o_tkf = work.take(N * K * 4), o_tw = work.take(N * K * 4), o_ioff = work.take(N * K * 4),
                 o_tch = work.take(N * K), o_ifound = work.take(N * K), o_choff = work.take((N * K + N) * 4), o_chkf = work.take(N * (E + K) * 4),
                 o_chw = work.take(N * (E + K) * 4), o_rowof = work.take(2 * N * K * 4), o_hist = work.take(g->cap[0] > kConnLdsKeyframes ? N * K * 4 : 0);
    const size_t words = N * (TC2LI_CONNECTIONS_COUNTS + kMgcStatusWords);
    TC2LI_HIP_CHECK(g->h_conn.ensure(N)); TC2LI_HIP_CHECK(g->d_conn.ensure(N)); TC2LI_HIP_CHECK(g->d_conn_scratch.ensure(work.off));
    TC2LI_HIP_CHECK(g->d_conn_words.ensure(words)); TC2LI_HIP_CHECK(g->h_conn_words.ensure(words));
    for (int i = 0; i < n; ++i) {
        const SeqMeta& m = g->seq[sequences[i]];
        MgConnDev r{};
        r.sequence = sequences[i]; r.obs_generation = m.generation; r.conn_generation = m.conn_generation; r.n_kf = m.n_kf; r.conn_rows = m.conn_rows;
        r.current = rows[i]; r.slot_begin = m.slot_off[rows[i]]; r.n_slots = m.slot_off[rows[i] + 1] - m.slot_off[rows[i]];
        r.init_kf_id = init_kf_id ? init_kf_id[i] : 0; r.first_connection = first_connection ? first_connection[i] : 0; r.mode = mode;
        g->h_conn.p[i] = r;
    }
    TC2LI_HIP_CHECK(hipMemcpyAsync(g->d_conn.p, g->h_conn.p, N * sizeof(MgConnDev), hipMemcpyHostToDevice, st));   // all that goes up
    uint8_t* w = g->d_conn_scratch.p;
    MgConnBatch M{};
    M.T = g->T; M.C = g->C; M.n = n; M.max_kf = max_kf; M.records = g->d_conn.p;
    M.problems = reinterpret_cast<ConnProblemDev*>(w + o_prob);
    M.row_of = reinterpret_cast<int32_t*>(w + o_rowof);
    M.status = g->d_conn_words.p + N * TC2LI_CONNECTIONS_COUNTS;
    ConnBatch& B = M.B;
    B.n_problems = n; B.n_items = 0; B.problems = M.problems; B.problem_of_item = nullptr;
    B.kf_flags = g->T.kf_flags; B.conn_offsets = g->C.conn_offsets; B.conn_kf = g->C.conn_kf; B.conn_weight = g->C.conn_weight;
    B.slot_point = g->T.slot_point; B.point_bad = g->T.point_flags; B.obs_offsets = g->T.obs_offsets; B.obs_kf = g->T.obs_kf;
    B.hist = reinterpret_cast<int32_t*>(w + o_hist); B.touched_weight = reinterpret_cast<int32_t*>(w + o_tw); B.item_off = reinterpret_cast<int32_t*>(w + o_ioff);
    B.item_found = w + o_ifound;
    B.counts = g->d_conn_words.p; B.counter_kf = reinterpret_cast<int32_t*>(w + o_cnkf); B.counter_weight = reinterpret_cast<int32_t*>(w + o_cnw);
    B.ordered_kf = reinterpret_cast<int32_t*>(w + o_okf); B.ordered_weight = reinterpret_cast<int32_t*>(w + o_ow); B.touched_kf = reinterpret_cast<int32_t*>(w + o_tkf);
    B.touched_changed = w + o_tch; B.changed_offsets = reinterpret_cast<int32_t*>(w + o_choff); B.changed_kf = reinterpret_cast<int32_t*>(w + o_chkf);
    B.changed_weight = reinterpret_cast<int32_t*>(w + o_chw);
    launch_map_graph_connections(M, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(g->h_conn_words.p, g->d_conn_words.p, words * 4, hipMemcpyDeviceToHost, st));   // the counts blocks and the status words
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    const int32_t* counts = g->h_conn_words.p;
    const int32_t* status = counts + N * TC2LI_CONNECTIONS_COUNTS;
    int short_of_room = -1;
    for (int i = 0; i < n; ++i) {
        g->seq[sequences[i]].conn_rows = g->seq[sequences[i]].n_kf;                  // the first kernel gave the appended rows their offsets
        if (!status[(size_t)i * kMgcStatusWords] && short_of_room < 0) short_of_room = i;
    }
    for (int i = 0; i < n; ++i) {
        const int32_t* c = counts + (size_t)i * TC2LI_CONNECTIONS_COUNTS;
        const int32_t* s = status + (size_t)i * kMgcStatusWords;
        if (counts_out) {
            int32_t* o = counts_out + (size_t)i * TC2LI_CONNECTIONS_COUNTS;
            memcpy(o, c, TC2LI_CONNECTIONS_COUNTS * 4);
            if (mode == kMgcErase) o[TC2LI_CONNECTIONS_N_ORDERED] = o[TC2LI_CONNECTIONS_N_CHANGED] = o[TC2LI_CONNECTIONS_N_CHANGED_ENTRIES] = 0;
            o[6] = short_of_room >= 0 ? s[1] : 0; o[7] = short_of_room >= 0 ? s[2] : 0;
        }
        if (short_of_room >= 0) continue;
        SeqMeta& m = g->seq[sequences[i]];
        if (c[TC2LI_CONNECTIONS_STATUS] == TC2LI_CONNECTIONS_UPDATED) { m.conn_generation ^= 1; m.n_weight = s[1]; m.n_ordered = s[2]; }
        ++m.conn_updates;
        m.conn_bytes = (int64_t)sizeof(MgConnDev);
    }
    if (short_of_room >= 0) {
        const int32_t* s = status + (size_t)short_of_room * kMgcStatusWords;
        set_error("%s: sequence %d would hold %d weight and %d ordered entries, the reserve is %d; no sequence was changed", me, sequences[short_of_room],
                  s[1], s[2], g->C.cap_e);
        return TC2LI_ERR_CAPACITY;
    }
    return n;
}
}  // namespace

extern "C" int tc2li_map_graph_update_connections_batch(tc2li_map_graph_handle* g, const int32_t* sequences, const int32_t* current_rows,
                                                        const uint8_t* first_connection, const int64_t* init_kf_id, int n, int32_t* counts_out,
                                                        void* stream) {
    const char* me = "tc2li_map_graph_update_connections_batch";
    if (!reserved(me, g)) return TC2LI_ERR_INVALID;
    if (n < 0 || (n && (!sequences || !current_rows || !first_connection || !init_kf_id || !counts_out))) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    return connections_call(me, g, sequences, current_rows, first_connection, init_kf_id, n, counts_out, kMgcUpdate, stream);
}

extern "C" int tc2li_map_graph_erase_connections_batch(tc2li_map_graph_handle* g, const int32_t* sequences, const int32_t* rows, int n, void* stream) {
    const char* me = "tc2li_map_graph_erase_connections_batch";
    if (!reserved(me, g)) return TC2LI_ERR_INVALID;
    if (n < 0 || (n && (!sequences || !rows))) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    return connections_call(me, g, sequences, rows, nullptr, nullptr, n, nullptr, kMgcErase, stream);
}

// ---- what a gather reads ---------------------------------------------------------------------------------------------------------------
int tc2li::MgLease::acquire(const char* entry, tc2li_map_graph_handle* g, tc2li_keyframe_store* store, const int32_t* sequences_, int n_) {
    if (!g || n_ < 0 || (n_ && !sequences_)) { set_error("%s: null graph or sequences", entry); return TC2LI_ERR_INVALID; }
    if (store != g->store) { set_error("%s: the graph was created on another keyframe store", entry); return TC2LI_ERR_INVALID; }
    g->mu.lock();
    graph = g; sequences = sequences_; n = n_;
    T = g->T; C = g->C;
    seq.resize(n);
    for (int p = 0; p < n; ++p) {
        if (!sequence_ok(g, sequences[p]) || !g->seq[sequences[p]].set) { set_error("%s: problem %d names sequence %d, which is out of range or was never set", entry, p, sequences[p]); return TC2LI_ERR_INVALID; }
        seq[p] = view_of(g, sequences[p]);
    }
    return 0;
}
tc2li::MgLease::~MgLease() {
    if (!graph) return;
    if (uploaded >= 0)
        for (int p = 0; p < n; ++p) graph->seq[sequences[p]].gather_bytes = uploaded;
    graph->mu.unlock();
}

// ---- the commit of solved windows ------------------------------------------------------------------------------------------------------
int tc2li::map_graph_read(const char* entry, const MgLease& lease, int sequence, MgHostTables* out) {
    tc2li_map_graph_handle* g = lease.graph;
    const SeqMeta& m = g->seq[sequence];
    const int32_t caps[4] = {m.n_kf, m.slot_off[m.n_kf], m.n_pt, m.n_obs};
    const size_t nk = (size_t)caps[0], ns = (size_t)caps[1], np = (size_t)caps[2], no = (size_t)caps[3];
    out->kf_slot.assign(nk + 1, 0); out->kf_id.assign(nk + 1, 0); out->kf_flags.assign(nk + 1, 0); out->poses7.assign(7 * nk + 1, 0.0);
    out->slot_offsets.assign(nk + 1, 0); out->slot_point.assign(ns + 1, 0); out->point_flags.assign(np + 1, 0); out->positions.assign(3 * np + 1, 0.0);
    out->obs_offsets.assign(np + 1, 0); out->obs_kf.assign(no + 1, 0); out->obs_index.assign(no + 1, 0);
    tc2li_map_graph_tables& t = out->tables;
    t.kf_slot = out->kf_slot.data(); t.kf_id = out->kf_id.data(); t.kf_flags = out->kf_flags.data(); t.poses7 = out->poses7.data();
    t.slot_offsets = out->slot_offsets.data(); t.slot_point = out->slot_point.data(); t.point_flags = out->point_flags.data(); t.positions = out->positions.data();
    t.obs_offsets = out->obs_offsets.data(); t.obs_kf = out->obs_kf.data(); t.obs_index = out->obs_index.data();
    int32_t counts[4];
    return download_locked(entry, g, sequence, &t, caps, counts);
}

int tc2li::map_graph_commit(const char* entry, const MgLease& lease, const MgCommitSource& src, const std::vector<MgCommitWindow>& wins,
                            const tc2li_map_graph_delta* host_logs, int n_host_logs, uint32_t flags, hipStream_t st) {
    tc2li_map_graph_handle* g = lease.graph;
    const int n = (int)wins.size();
    std::vector<int> order;                  // the windows with erase pairs first: their records are the apply kernels' batch
    for (int k = 0; k < n; ++k) if (wins[k].n_erase > 0) order.push_back(k);
    const int n_erasing = (int)order.size();
    for (int k = 0; k < n; ++k) if (wins[k].n_erase <= 0) order.push_back(k);
    // what k_mg_apply will read to find every touched row's edits (kMgMaxWalk): pair i erases its observation with edit 2 i + 1, and the
    // pairs of a point are together within the monocular and within the stereo stretch, so a point has at most two stretches
    size_t n_edits = 0;
    int max_rows = 0;
    for (int k = 0; k < n_erasing; ++k) {
        const MgCommitWindow& w = wins[order[k]];
        std::vector<int32_t> first(w.n_points, -1), last(w.n_points, -1);
        for (int i = 0; i < w.n_erase; ++i) {
            const int pt = w.erase_point[i];
            if (pt < 0 || pt >= w.n_points) { set_error("%s: sequence %d: an erase pair names a point outside the window", entry, w.sequence); return TC2LI_ERR_INVALID; }
            if (first[pt] < 0) first[pt] = 2 * i + 1;
            last[pt] = 2 * i + 1;
        }
        int64_t walk = 0;
        for (int p = 0; p < w.n_points; ++p) walk += first[p] < 0 ? 0 : last[p] - first[p] + 1;
        if (walk > kMgMaxWalk) {
            set_error("%s: sequence %d: the erase pairs of single points lie %lld log entries apart in sum, the limit is %lld; solve without the commit and split the log", entry,
                      w.sequence, (long long)walk, (long long)kMgMaxWalk);
            return TC2LI_ERR_CAPACITY;
        }
        n_edits += 2 * (size_t)w.n_erase;
        if (n_edits > kMaxRows) return too_many_rows(entry, order[k]);
    }
    MgCommitBatch C{};
    if (n) {
        if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
        const size_t o_edits = (size_t)n * sizeof(MgApplyDev), bytes = o_edits + n_edits * sizeof(tc2li_map_graph_edit);
        TC2LI_HIP_CHECK(g->h_commit.ensure(o_edits)); TC2LI_HIP_CHECK(g->d_commit.ensure(bytes));
        TC2LI_HIP_CHECK(g->d_commit_words.ensure(2 * (size_t)n)); TC2LI_HIP_CHECK(g->h_commit_words.ensure(2 * (size_t)n));
        MgApplyDev* rec = reinterpret_cast<MgApplyDev*>(g->h_commit.p);
        size_t e_at = 0;
        for (int k = 0; k < n; ++k) {
            const MgCommitWindow& w = wins[order[k]];
            const SeqMeta& m = g->seq[w.sequence];
            MgApplyDev r{};
            r.sequence = w.sequence; r.generation = m.generation; r.n_kf = m.n_kf; r.n_points = m.n_pt; r.n_slot = m.slot_off[m.n_kf]; r.n_obs = m.n_obs;
            r.edit_off = (int32_t)e_at; r.n_edits = 2 * std::max(w.n_erase, 0); r.value_off = 0; r.n_points_new = m.n_pt;
            r.pad_[kMgcPoseOff] = w.pose_off; r.pad_[kMgcPointOff] = w.point_off; r.pad_[kMgcPoses] = w.n_poses; r.pad_[kMgcPoints] = w.n_points;
            r.pad_[kMgcEraseAt] = w.erase_at; r.pad_[kMgcEraseCap] = w.erase_cap;
            rec[k] = r;
            e_at += (size_t)r.n_edits;
            max_rows = std::max(max_rows, w.n_poses + w.n_points);
        }
        TC2LI_HIP_CHECK(hipMemcpyAsync(g->d_commit.p, g->h_commit.p, o_edits, hipMemcpyHostToDevice, st));   // all that goes up: 64 bytes per sequence
        C.T = g->T; C.n = n; C.n_erasing = n_erasing; C.max_rows = max_rows; C.flags = flags;
        C.records = reinterpret_cast<const MgApplyDev*>(g->d_commit.p);
        C.pose_row = src.pose_row; C.fixed = src.fixed; C.poses7 = src.poses7; C.point_row = src.point_row; C.points3 = src.points3; C.erase = src.erase;
        C.edits = reinterpret_cast<tc2li_map_graph_edit*>(g->d_commit.p + o_edits);
        C.status = g->d_commit_words.p + n;
        if (n_erasing) {   // the erase logs first: they read the tables and write none, and the host sees whether every pair was resolved
            launch_map_graph_commit_erase_log(C, st);
            TC2LI_HIP_CHECK(hipGetLastError());
            TC2LI_HIP_CHECK(hipMemcpyAsync(g->h_commit_words.p + n, C.status, (size_t)n_erasing * 4, hipMemcpyDeviceToHost, st));
            TC2LI_HIP_CHECK(stream_wait_blocking(st));
            for (int k = 0; k < n_erasing; ++k)
                if (g->h_commit_words.p[n + k]) {
                    set_error("%s: sequence %d: an erase pair names a keyframe that is not in the point's observation row", entry,
                              wins[order[k]].sequence);
                    return TC2LI_ERR_INVALID;
                }
        }
    }
    // the logs of the windows finished on the host: checked as any log before anything is written
    if (n_host_logs > 0) {
        const int rc = apply_locked(entry, g, host_logs, n_host_logs, st);
        if (rc < 0) return rc;
    }
    if (!n) return 0;
    launch_map_graph_commit_scatter(C, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    if (n_erasing) {   // a window without erase pairs keeps its observation CSR and its generation
        MgApplyBatch A{};
        A.T = g->T; A.n = n_erasing; A.deltas = C.records; A.edits = C.edits; A.values = nullptr; A.totals = g->d_commit_words.p;
        launch_map_graph_apply(A, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipMemcpyAsync(g->h_commit_words.p, g->d_commit_words.p, (size_t)n_erasing * 4, hipMemcpyDeviceToHost, st));
    }
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    for (int k = 0; k < n; ++k) {
        SeqMeta& m = g->seq[wins[order[k]].sequence];
        if (k < n_erasing) { m.generation ^= 1; m.n_obs = g->h_commit_words.p[k]; }
        ++m.applies;
        m.apply_bytes = (int64_t)sizeof(MgApplyDev);
    }
    return 0;
}

// the host's statement of the step: it defines what map_graph_commit leaves
extern "C" int tc2li_host_ba_window_commit_log(const tc2li_map_graph_tables* t, const tc2li_ba_window_solve_problem* q, int32_t result, uint32_t flags,
                                               tc2li_map_graph_edit* edits, int edit_capacity, double* values, int value_capacity, int32_t* n_edits_out,
                                               int32_t* n_values_out) {
    const char* me = "tc2li_host_ba_window_commit_log";
    if (!t || !q || !n_values_out || edit_capacity < 0 || value_capacity < 0 || !q->window.counts) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    if (flags & ~(uint32_t)TC2LI_BA_COMMIT_POSITIONS_F32) { set_error("%s: unknown flag bits", me); return TC2LI_ERR_INVALID; }
    if (!q->n_erase) { set_error("%s: n_erase is NULL: the commit is defined by the outlier rule", me); return TC2LI_ERR_INVALID; }
    const tc2li_ba_window_problem& w = q->window;
    if (w.counts[TC2LI_BA_WINDOW_STATUS] != TC2LI_BA_WINDOW_OK || result < 0) {   // ABORTED, refused or failed: nothing to recover
        if (n_edits_out) *n_edits_out = 0;
        *n_values_out = 0;
        return 0;
    }
    const char* what = tables_fault(*t);
    if (!what[0] && (!ascending(t->slot_offsets, t->n_keyframes) || !ascending(t->obs_offsets, t->n_points))) what = "offsets do not ascend from 0";
    if (what[0]) { set_error("%s: %s", me, what); return TC2LI_ERR_INVALID; }
    const int n_poses = w.counts[TC2LI_BA_WINDOW_N_POSES], n_points = w.counts[TC2LI_BA_WINDOW_N_POINTS], n_erase = *q->n_erase;
    if (n_poses < 0 || n_points < 0 || n_erase < 0 || (n_poses && (!w.pose_row || !w.fixed || !w.poses7_out)) || (n_points && (!w.point_row || !w.points3_out)) ||
        (n_erase && (!q->erase_pose || !q->erase_point)) || (t->obs_offsets[t->n_points] && (!t->obs_kf || !t->obs_index))) {
        set_error("%s: negative count or null array", me);
        return TC2LI_ERR_INVALID;
    }
    int n_free = 0;
    for (int i = 0; i < n_poses; ++i) {
        if (w.pose_row[i] < 0 || w.pose_row[i] >= t->n_keyframes) { set_error("%s: pose_row[%d] is outside the tables", me, i); return TC2LI_ERR_INVALID; }
        n_free += w.fixed[i] ? 0 : 1;
    }
    for (int j = 0; j < n_points; ++j)
        if (w.point_row[j] < 0 || w.point_row[j] >= t->n_points) { set_error("%s: point_row[%d] is outside the tables", me, j); return TC2LI_ERR_INVALID; }
    int64_t need_edits = 2 * (int64_t)n_erase + n_free + n_points;   // (fewer where a keyframe row holds no slot to clear: known after the look-up)
    const int64_t need_values = 7 * (int64_t)n_free + 3 * (int64_t)n_points;
    if (need_edits > INT_MAX || need_values > INT_MAX) { set_error("%s: the log is beyond 2^31 entries", me); return TC2LI_ERR_INVALID; }
    if (n_erase > q->erase_capacity) {
        if (n_edits_out) *n_edits_out = (int32_t)need_edits;
        *n_values_out = (int32_t)need_values;
        set_error("%s: %d erase pairs and erase_capacity %d: the lists are cut", me, n_erase, q->erase_capacity);
        return TC2LI_ERR_CAPACITY;
    }
    std::vector<int32_t> index(n_erase, 0);
    for (int i = 0; i < n_erase; ++i) {
        const int ep = q->erase_pose[i], et = q->erase_point[i];
        if (ep < 0 || ep >= n_poses || et < 0 || et >= n_points) { set_error("%s: erase pair %d is outside the counts", me, i); return TC2LI_ERR_INVALID; }
        const int kf = w.pose_row[ep], pt = w.point_row[et];
        const int32_t *b = t->obs_kf + t->obs_offsets[pt], *e = t->obs_kf + t->obs_offsets[pt + 1];
        const int32_t* it = std::lower_bound(b, e, kf);
        if (it == e || *it != kf) { set_error("%s: erase pair %d: keyframe row %d is not in the observation row of point %d", me, i, kf, pt); return TC2LI_ERR_INVALID; }
        index[i] = t->obs_index[it - t->obs_kf];                                            // GetIndexInKeyFrame (KeyFrame::EraseMapPointMatch(MapPoint*))
        if (index[i] < 0 || index[i] >= t->slot_offsets[kf + 1] - t->slot_offsets[kf]) { index[i] = -1; --need_edits; }   // the row's matches are not resident: no slot to clear
    }
    if (n_edits_out) *n_edits_out = (int32_t)need_edits;
    *n_values_out = (int32_t)need_values;
    if (need_edits > edit_capacity || need_values > value_capacity) {
        set_error("%s: the log has %lld edits and %lld values, the arrays hold %d and %d", me, (long long)need_edits, (long long)need_values, edit_capacity, value_capacity);
        return TC2LI_ERR_CAPACITY;
    }
    if ((need_edits && !edits) || (need_values && !values)) { set_error("%s: null edits or values", me); return TC2LI_ERR_INVALID; }
    int e_at = 0, v_at = 0;
    for (int i = 0; i < n_erase; ++i) {                                                     // OptimizerWithLidar.cc:457-463
        const int kf = w.pose_row[q->erase_pose[i]], pt = w.point_row[q->erase_point[i]];
        if (index[i] >= 0) edits[e_at++] = tc2li_map_graph_edit{TC2LI_MAP_GRAPH_SET_SLOT, kf, index[i], -1};
        edits[e_at++] = tc2li_map_graph_edit{TC2LI_MAP_GRAPH_ERASE_OBSERVATION, pt, kf, 0};
    }
    for (int i = 0; i < n_poses; ++i) {                                                     // :468-475
        if (w.fixed[i]) continue;
        edits[e_at++] = tc2li_map_graph_edit{TC2LI_MAP_GRAPH_SET_POSE, w.pose_row[i], v_at, 0};
        memcpy(values + v_at, w.poses7_out + 7 * (size_t)i, 7 * sizeof(double));
        v_at += 7;
    }
    for (int j = 0; j < n_points; ++j) {                                                    // :478-484
        edits[e_at++] = tc2li_map_graph_edit{TC2LI_MAP_GRAPH_SET_POSITION, w.point_row[j], v_at, 0};
        for (int c = 0; c < 3; ++c) {
            const double x = w.points3_out[3 * (size_t)j + c];
            values[v_at++] = (flags & TC2LI_BA_COMMIT_POSITIONS_F32) ? (double)(float)x : x;   // cast<float>() (:482)
        }
    }
    return e_at;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------
extern "C" int tc2li_host_map_graph_apply(const tc2li_map_graph_tables* in, const tc2li_map_graph_edit* edits, int n_edits, const double* values,
                                          int n_values, tc2li_map_graph_tables* out, const int32_t* capacities, int32_t* counts) {
    const char* me = "tc2li_host_map_graph_apply";
    if (!in || !out || !capacities || !counts) { set_error("%s: invalid argument", me); return TC2LI_ERR_INVALID; }
    const char* what = tables_fault(*in);
    if (!what[0] && (!ascending(in->slot_offsets, in->n_keyframes) || !ascending(in->obs_offsets, in->n_points))) what = "offsets do not ascend from 0";
    if (what[0]) { set_error("%s: %s", me, what); return TC2LI_ERR_INVALID; }
    const int n_kf = in->n_keyframes, n_pt = in->n_points, n_slot = in->slot_offsets[n_kf], n_obs = in->obs_offsets[n_pt];
    if ((n_slot && !in->slot_point) || (n_obs && (!in->obs_kf || !in->obs_index))) { set_error("%s: null slot_point, obs_kf or obs_index", me); return TC2LI_ERR_INVALID; }
    if (n_kf > capacities[0] || n_slot > capacities[1] || n_pt > capacities[2] || n_obs > capacities[3]) { set_error("%s: the tables are beyond the capacities", me); return TC2LI_ERR_CAPACITY; }
    LogAfter after;
    const LogSizes sizes{n_kf, n_pt, n_obs, in->kf_slot, in->slot_offsets};
    const int rc = check_log(sizes, edits, n_edits, values, n_values, capacities, nullptr, &after, &what);
    if (rc < 0) { set_error("%s: %s", me, what); return rc; }
    // the state, then the log one edit after the other
    std::vector<int32_t> kf_slot(in->kf_slot, in->kf_slot + n_kf), slot_off(in->slot_offsets, in->slot_offsets + n_kf + 1), slot_point(in->slot_point, in->slot_point + n_slot);
    std::vector<int64_t> kf_id(in->kf_id, in->kf_id + n_kf);
    std::vector<uint8_t> kf_flags(in->kf_flags, in->kf_flags + n_kf), point_flags(in->point_flags, in->point_flags + n_pt);
    std::vector<double> poses7(in->poses7, in->poses7 + 7 * (size_t)n_kf), positions(in->positions, in->positions + 3 * (size_t)n_pt);
    std::vector<std::vector<std::pair<int32_t, int32_t>>> obs(n_pt);
    for (int p = 0; p < n_pt; ++p)
        for (int o = in->obs_offsets[p]; o < in->obs_offsets[p + 1]; ++o) obs[p].emplace_back(in->obs_kf[o], in->obs_index[o]);
    for (int e = 0; e < n_edits; ++e) {
        const tc2li_map_graph_edit& ed = edits[e];
        switch (ed.op) {
            case TC2LI_MAP_GRAPH_ADD_KEYFRAME: {                                          // new KeyFrame (Tracking.cc:3078)
                const double* v = values + ed.c;
                kf_slot.push_back(ed.a); kf_id.push_back((int64_t)v[0]); kf_flags.push_back((uint8_t)(int)v[1]);
                poses7.insert(poses7.end(), v + 2, v + 9);
                slot_point.insert(slot_point.end(), (size_t)ed.b, -1);
                slot_off.push_back(slot_off.back() + ed.b);
                break;
            }
            case TC2LI_MAP_GRAPH_SET_KEYFRAME_FLAGS: kf_flags[ed.a] = (uint8_t)ed.b; break;          // KeyFrame.cc:585
            case TC2LI_MAP_GRAPH_SET_POSE: std::copy(values + ed.b, values + ed.b + 7, poses7.begin() + 7 * (size_t)ed.a); break;   // KeyFrame.cc:121
            case TC2LI_MAP_GRAPH_ADD_POINT:                                                          // new MapPoint
                point_flags.push_back((uint8_t)ed.a);
                positions.insert(positions.end(), values + ed.b, values + ed.b + 3);
                obs.emplace_back();
                break;
            case TC2LI_MAP_GRAPH_SET_POINT_FLAGS: point_flags[ed.a] = (uint8_t)ed.b; break;          // MapPoint.cc:225
            case TC2LI_MAP_GRAPH_SET_POSITION: std::copy(values + ed.b, values + ed.b + 3, positions.begin() + 3 * (size_t)ed.a); break;
            case TC2LI_MAP_GRAPH_SET_SLOT: slot_point[slot_off[ed.a] + ed.b] = ed.c; break;          // KeyFrame.cc:309-340
            case TC2LI_MAP_GRAPH_ADD_OBSERVATION: {                                                  // MapPoint.cc:150-175
                auto& row = obs[ed.a];
                auto it = std::lower_bound(row.begin(), row.end(), ed.b, [](const std::pair<int32_t, int32_t>& x, int32_t k) { return x.first < k; });
                if (it != row.end() && it->first == ed.b) it->second = ed.c;                         // mObservations[pKF] = indexes (:155-169)
                else row.insert(it, std::make_pair(ed.b, ed.c));
                break;
            }
            case TC2LI_MAP_GRAPH_ERASE_OBSERVATION: {                                                // MapPoint.cc:177-210
                auto& row = obs[ed.a];
                auto it = std::lower_bound(row.begin(), row.end(), ed.b, [](const std::pair<int32_t, int32_t>& x, int32_t k) { return x.first < k; });
                if (it != row.end() && it->first == ed.b) row.erase(it);                             // absent: nothing (:182)
                break;
            }
            default: obs[ed.a].clear(); break;                                                       // mObservations.clear()
        }
    }
    size_t total = 0;
    for (const auto& row : obs) total += row.size();
    counts[0] = (int32_t)kf_slot.size(); counts[1] = slot_off.back(); counts[2] = (int32_t)point_flags.size(); counts[3] = (int32_t)total;
    const size_t nk = kf_slot.size(), np = point_flags.size();
    if (!out->slot_offsets || !out->obs_offsets || (nk && (!out->kf_slot || !out->kf_id || !out->kf_flags || !out->poses7)) || (slot_point.size() && !out->slot_point) ||
        (np && (!out->point_flags || !out->positions)) || (total && (!out->obs_kf || !out->obs_index))) {
        set_error("%s: null output array", me);
        return TC2LI_ERR_INVALID;
    }
    auto put = [](void* dst, const void* src, size_t b) { if (b) memcpy(dst, src, b); };
    put(out->kf_slot, kf_slot.data(), nk * 4); put(out->kf_id, kf_id.data(), nk * 8); put(out->kf_flags, kf_flags.data(), nk); put(out->poses7, poses7.data(), nk * 56);
    put(out->slot_offsets, slot_off.data(), (nk + 1) * 4); put(out->slot_point, slot_point.data(), slot_point.size() * 4);
    put(out->point_flags, point_flags.data(), np); put(out->positions, positions.data(), np * 24);
    int32_t o = 0;
    for (size_t p = 0; p < np; ++p) {
        out->obs_offsets[p] = o;
        for (const auto& kv : obs[p]) { out->obs_kf[o] = kv.first; out->obs_index[o++] = kv.second; }
    }
    out->obs_offsets[np] = o;
    out->n_keyframes = (int32_t)nk; out->n_points = (int32_t)np;
    return 0;
}

// The device-resident keyframe store and the batch entries of local mapping's geometric front half (include/tc2li_hip.h):
//   tc2li_keyframe_store_*             what a keyframe never changes after creation crosses the bus once, when the keyframe is made
//   tc2li_create_new_map_points_batch  LocalMapping::CreateNewMapPoints (SF/src/LocalMapping.cc:402-726) for many keyframes
//   tc2li_fuse_search_batch            the ORBmatcher::Fuse searches of SearchInNeighbors (:728-837) for many (keyframe, point list) items
// A batch call uploads one packed block (tables, poses and pair constants, has_point / points), launches a fixed number of kernels
// over tables of (problem, neighbour) pairs or items, downloads one block and waits once.  The kernels run the device functions of
// the single-keyframe entries (mapping_kernels.hip); the host constants come from mapping_host.hpp, so the results are the same bits.
//
// The slab, allocated once:   cell_start [max_keyframes][kCellsPlus1] | items [max_keyframes][max_keypoints] | put tables | slots
// and a slot at fixed offsets: keys | descriptors | u_right | depth | match keys (x, y, octave) | fv_node | fv_offset | fv_index
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "ba_window_device.hpp"
#include "common.hpp"
#include "mapping_device.hpp"
#include "mapping_host.hpp"
#include "matcher_device.hpp"
#include "neighbors_device.hpp"
#include "packed_batch.hpp"

using namespace tc2li;
using namespace tc2li::mapping_host;

static_assert(sizeof(tc2li_new_map_point) == 32, "ABI layout");
static_assert(sizeof(tc2li_map_point) == 68, "ABI layout");
static_assert(kNewPointsMaxKeys >= kMaxMatchKeys, "k_new_points_compact holds one entry per keypoint of a slot");

namespace {

inline size_t a16(size_t v) { return (v + 15) & ~(size_t)15; }

struct SlotInfo {
    int32_t n = -1, n_nodes = -1, n_entries = 0, n_levels = 0;  // n < 0: empty; n_levels: 1 + the highest octave among the keypoints
    float bounds[4] = {0, 0, 0, 0};
};

}  // namespace

struct tc2li_keyframe_store {
    int max_kf = 0, max_kp = 0;
    uint8_t* slab = nullptr;
    size_t o_cells = 0, o_items = 0, o_tab = 0, o_slots = 0, stride = 0;              // regions of the slab
    size_t s_keys = 0, s_desc = 0, s_ur = 0, s_depth = 0, s_mkeys = 0, s_node = 0, s_off = 0, s_idx = 0;  // arrays of a slot
    std::vector<SlotInfo> info;
    std::mutex info_mu;  // the table above: held for a look or an update, never across device work
    std::mutex put_mu;   // one put_batch at a time: the staging arena and the put tables
    PinnedBuf<uint8_t> arena;
    PinnedBuf<CopyTask> tasks;

    uint8_t* slot(int s) const { return slab + o_slots + (size_t)s * stride; }
    int32_t* cell_start(int s) const { return reinterpret_cast<int32_t*>(slab + o_cells) + (size_t)s * kCellsPlus1; }
    uint16_t* items(int s) const { return reinterpret_cast<uint16_t*>(slab + o_items) + (size_t)s * max_kp; }
    KfDev view(int s, const SlotInfo& si) const {  // pose, has_point and the pair constants are the caller's
        KfDev d{};
        uint8_t* b = slot(s);
        d.n = si.n; d.n_nodes = si.n_nodes;
        d.keys = reinterpret_cast<const float*>(b + s_keys); d.desc = b + s_desc;
        d.u_right = reinterpret_cast<const float*>(b + s_ur); d.depth = reinterpret_cast<const float*>(b + s_depth);
        d.fv_node = reinterpret_cast<const int32_t*>(b + s_node); d.fv_off = reinterpret_cast<const int32_t*>(b + s_off);
        d.fv_idx = reinterpret_cast<const int32_t*>(b + s_idx);
        return d;
    }
};

namespace {

// Work space of one batch call: taken from a free list for the length of the call, so concurrent callers never share one and none
// waits for another (the list's lock covers the take and the return only).
struct BatchSpace {
    DevBuf<uint8_t> d_in, d_work, d_out;
    PinnedBuf<uint8_t> h_in, h_out;
};
struct SpacePool {
    std::mutex mu;
    std::vector<std::unique_ptr<BatchSpace>> free;
};
struct SpaceLease {
    std::unique_ptr<BatchSpace> s;
    SpaceLease() {
        SpacePool& P = shutdown_owned<SpacePool>();
        std::lock_guard<std::mutex> lk(P.mu);
        if (!P.free.empty()) { s = std::move(P.free.back()); P.free.pop_back(); }
        else s.reset(new BatchSpace());
    }
    ~SpaceLease() {
        SpacePool& P = shutdown_owned<SpacePool>();
        std::lock_guard<std::mutex> lk(P.mu);
        P.free.push_back(std::move(s));
    }
};

bool slot_in_range(const tc2li_keyframe_store* S, int s) { return s >= 0 && s < S->max_kf; }

}  // namespace

extern "C" int tc2li_keyframe_store_create(int max_keyframes, int max_keypoints, tc2li_keyframe_store** out) {
    if (!out || max_keyframes < 1 || max_keypoints < 1 || (int64_t)max_keyframes * max_keypoints > 0x7fffffffLL) {
        set_error("tc2li_keyframe_store_create: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    *out = nullptr;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    std::unique_ptr<tc2li_keyframe_store> S(new tc2li_keyframe_store());
    S->max_kf = max_keyframes; S->max_kp = max_keypoints;
    const size_t K = (size_t)max_keypoints, F = (size_t)max_keyframes;
    Packer slot, slab;
    S->s_keys = slot.take(K * sizeof(tc2li_keypoint)); S->s_desc = slot.take(32 * K); S->s_ur = slot.take(4 * K); S->s_depth = slot.take(4 * K);
    S->s_mkeys = slot.take(K * sizeof(MatchKey)); S->s_node = slot.take(4 * K); S->s_off = slot.take(4 * (K + 1)); S->s_idx = slot.take(4 * K);
    S->stride = slot.off;
    S->o_cells = slab.take(F * kCellsPlus1 * sizeof(int32_t)); S->o_items = slab.take(F * K * sizeof(uint16_t));
    S->o_tab = slab.take(F * (a16(sizeof(MatchFrameDev)) + 8)); S->o_slots = slab.take(F * S->stride);
    TC2LI_HIP_CHECK(hipMalloc((void**)&S->slab, slab.off));
    S->info.assign(F, SlotInfo{});
    *out = S.release();
    return 0;
}

extern "C" int tc2li_keyframe_store_destroy(tc2li_keyframe_store* S) {
    if (!S) return 0;
    if (S->slab) (void)hipFree(S->slab);
    delete S;
    return 0;
}

extern "C" int tc2li_keyframe_store_erase(tc2li_keyframe_store* S, int slot) {
    if (!S || !slot_in_range(S, slot)) { set_error("tc2li_keyframe_store_erase: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(S->info_mu);
    S->info[slot] = SlotInfo{};
    return 0;
}

extern "C" int tc2li_keyframe_store_info(tc2li_keyframe_store* S, int slot, int32_t* n_keypoints, int32_t* n_nodes) {
    if (!S || !slot_in_range(S, slot)) { set_error("tc2li_keyframe_store_info: invalid argument"); return TC2LI_ERR_INVALID; }
    std::lock_guard<std::mutex> lk(S->info_mu);
    if (n_keypoints) *n_keypoints = S->info[slot].n < 0 ? -1 : S->info[slot].n;
    if (n_nodes) *n_nodes = S->info[slot].n < 0 ? -1 : S->info[slot].n_nodes;
    return 0;
}

// what tc2li_ba_window_batch reads of the store (ba_window_host.cpp)
int tc2li::keyframe_store_slots(const tc2li_keyframe_store* S) { return S->max_kf; }
void tc2li::keyframe_store_baw(tc2li_keyframe_store* S, BawStore* where, int32_t* n_keypoints, int32_t* n_levels, int capacity) {
    *where = BawStore{S->slab + S->o_slots, S->stride, S->s_keys, S->s_ur};
    std::lock_guard<std::mutex> lk(S->info_mu);
    for (int s = 0; s < capacity && s < S->max_kf; ++s) { n_keypoints[s] = S->info[s].n < 0 ? -1 : S->info[s].n; n_levels[s] = S->info[s].n_levels; }
}

// what tc2li_search_in_neighbors_batch reads of the store (neighbors_host.cpp)
bool tc2li::keyframe_store_neighbors(tc2li_keyframe_store* S, int s, NbKf* out, int32_t* n_levels) {
    if (!slot_in_range(S, s)) return false;
    std::lock_guard<std::mutex> lk(S->info_mu);
    const SlotInfo& si = S->info[s];
    if (si.n < 0) return false;
    const KfDev d = S->view(s, si);
    out->keys = d.keys; out->desc = d.desc; out->u_right = d.u_right; out->cell_start = S->cell_start(s); out->items = S->items(s);
    out->n = si.n;
    memcpy(out->bounds, si.bounds, 16);
    *n_levels = si.n_levels;
    return true;
}

extern "C" int tc2li_keyframe_store_put_batch(tc2li_keyframe_store* S, int n, const int32_t* slots, const tc2li_keyframe_view* views,
                                              const float* bounds4, int n_levels, void* stream_) {
    if (!S || n < 0 || (n > 0 && (!slots || !views || !bounds4)) || n_levels < 1) { set_error("tc2li_keyframe_store_put_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    if (n == 0) return 0;
    // ---- every check before any device work: a refused call leaves the store as it was ----
    std::vector<uint8_t> named(S->max_kf, 0);
    std::vector<SlotInfo> fresh(n);
    static const uint8_t dummy = 0;
    size_t arena_bytes = a16((size_t)n * sizeof(MatchFrameDev)) + a16((size_t)n * 8);
    for (int k = 0; k < n; ++k) {
        if (!slot_in_range(S, slots[k])) { set_error("tc2li_keyframe_store_put_batch: slot %d out of range", slots[k]); return TC2LI_ERR_INVALID; }
        if (named[slots[k]]) { set_error("tc2li_keyframe_store_put_batch: slot %d named twice", slots[k]); return TC2LI_ERR_INVALID; }
        named[slots[k]] = 1;
        tc2li_keyframe_view v = views[k];
        v.has_point = &dummy;  // not stored: has_point and the pose are inputs of every search
        const int rc = check_view(&v, "tc2li_keyframe_store_put_batch");
        if (rc < 0) return rc;
        const int entries = v.n_nodes > 0 ? v.fv_offset[v.n_nodes] : 0;
        if (v.n > S->max_kp || v.n > kMaxMatchKeys || v.n_nodes > S->max_kp || entries > S->max_kp) {
            set_error("tc2li_keyframe_store_put_batch: keyframe with %d keypoints, %d nodes, %d entries; a slot holds %d (feature grid: %d)", v.n, v.n_nodes,
                      entries, S->max_kp, kMaxMatchKeys);
            return TC2LI_ERR_CAPACITY;
        }
        const float* b = bounds4 + 4 * (size_t)k;
        if (!(b[1] > b[0]) || !(b[3] > b[2])) { set_error("tc2li_keyframe_store_put_batch: empty image bounds"); return TC2LI_ERR_INVALID; }
        int top = 0;
        for (int i = 0; i < v.n; ++i) {
            if (v.keys[i].octave < 0 || v.keys[i].octave >= n_levels) { set_error("tc2li_keyframe_store_put_batch: keypoint octave out of range"); return TC2LI_ERR_INVALID; }
            top = std::max(top, v.keys[i].octave + 1);
        }
        fresh[k].n = v.n; fresh[k].n_nodes = v.n_nodes; fresh[k].n_entries = entries; fresh[k].n_levels = top;
        memcpy(fresh[k].bounds, b, 16);
        arena_bytes += a16((size_t)v.n * sizeof(tc2li_keypoint)) + a16(32 * (size_t)v.n) + 2 * a16(4 * (size_t)v.n) + a16((size_t)v.n * sizeof(MatchKey)) +
                       a16(4 * (size_t)v.n_nodes) + a16(4 * ((size_t)v.n_nodes + 1)) + a16(4 * (size_t)entries);
    }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    std::lock_guard<std::mutex> put_lock(S->put_mu);
    TC2LI_HIP_CHECK(S->arena.ensure(arena_bytes));
    TC2LI_HIP_CHECK(S->tasks.ensure(8 * (size_t)n + 1));
    // ---- one staging arena: the grid tables first, then every array of every keyframe ----
    uint8_t* A = S->arena.p;
    size_t at = 0, n_tasks = 0, max_bytes = 0;
    auto stage = [&](void* dst, const void* src, size_t bytes) -> uint8_t* {
        uint8_t* h = A + at;
        if (src && bytes) memcpy(h, src, bytes);
        if (bytes) { S->tasks.p[n_tasks++] = CopyTask{dst, h, bytes}; max_bytes = std::max(max_bytes, bytes); }
        at += a16(bytes);
        return h;
    };
    uint8_t* d_tab = S->slab + S->o_tab;
    MatchFrameDev* d_frames = reinterpret_cast<MatchFrameDev*>(d_tab);
    int32_t* d_key_base = reinterpret_cast<int32_t*>(d_tab + a16((size_t)n * sizeof(MatchFrameDev)));
    int32_t* d_cell_row = d_key_base + n;
    MatchFrameDev* h_frames = reinterpret_cast<MatchFrameDev*>(stage(d_frames, nullptr, a16((size_t)n * sizeof(MatchFrameDev)) + (size_t)n * 8));
    int32_t* h_key_base = reinterpret_cast<int32_t*>(reinterpret_cast<uint8_t*>(h_frames) + a16((size_t)n * sizeof(MatchFrameDev)));
    int32_t* h_cell_row = h_key_base + n;
    for (int k = 0; k < n; ++k) {
        const tc2li_keyframe_view& v = views[k];
        const SlotInfo& si = fresh[k];
        uint8_t* b = S->slot(slots[k]);
        stage(b + S->s_keys, v.keys, (size_t)v.n * sizeof(tc2li_keypoint));
        stage(b + S->s_desc, v.descriptors, 32 * (size_t)v.n);
        stage(b + S->s_ur, v.u_right, 4 * (size_t)v.n);
        stage(b + S->s_depth, v.depth, 4 * (size_t)v.n);
        MatchKey* mk = reinterpret_cast<MatchKey*>(stage(b + S->s_mkeys, nullptr, (size_t)v.n * sizeof(MatchKey)));
        for (int i = 0; i < v.n; ++i) mk[i] = MatchKey{v.keys[i].x, v.keys[i].y, v.keys[i].octave};
        stage(b + S->s_node, v.fv_node, 4 * (size_t)v.n_nodes);
        int32_t* off = reinterpret_cast<int32_t*>(stage(b + S->s_off, nullptr, 4 * ((size_t)v.n_nodes + 1)));
        if (v.n_nodes > 0) memcpy(off, v.fv_offset, 4 * ((size_t)v.n_nodes + 1)); else off[0] = 0;
        stage(b + S->s_idx, v.fv_index, 4 * (size_t)si.n_entries);
        h_frames[k] = MatchFrameDev{reinterpret_cast<const MatchKey*>(b + S->s_mkeys), b + S->s_desc, reinterpret_cast<const float*>(b + S->s_ur), nullptr, nullptr,
                                    v.n, 0, 0, 0, si.bounds[0], si.bounds[1], si.bounds[2], si.bounds[3]};
        h_key_base[k] = (int32_t)((size_t)slots[k] * S->max_kp);
        h_cell_row[k] = slots[k];
    }
    // ---- one copy of the arena into the slots, one grid launch over the n keyframes ----
    launch_copy_tasks(S->tasks.p, (int)n_tasks, max_bytes, st);
    MatchLists L{};
    L.cell_start = reinterpret_cast<int32_t*>(S->slab + S->o_cells);
    L.items = reinterpret_cast<uint16_t*>(S->slab + S->o_items);
    L.key_base = d_key_base; L.cell_row = d_cell_row;
    launch_match_grid(d_frames, n, L, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));  // resident on return: a search on any stream may follow
    std::lock_guard<std::mutex> lk(S->info_mu);
    for (int k = 0; k < n; ++k) S->info[slots[k]] = fresh[k];
    return 0;
}

extern "C" int tc2li_create_new_map_points_batch(tc2li_keyframe_store* S, const tc2li_new_points_problem* problems, int n_problems,
                                                 const tc2li_camera* cam, float mb, const float* scale_factors, const float* level_sigma2,
                                                 int n_levels, float scale_factor, tc2li_new_map_point* points, const int32_t* point_offsets,
                                                 int32_t* n_points, void* stream_) {
    const char* me = "tc2li_create_new_map_points_batch";
    if (!S || n_problems < 0 || (n_problems > 0 && (!problems || !n_points)) || !cam || !scale_factors || !level_sigma2 || n_levels < 1 || !point_offsets) {
        set_error("%s: invalid argument", me);
        return TC2LI_ERR_INVALID;
    }
    if (n_problems == 0) return 0;
    if (point_offsets[0] < 0) { set_error("%s: negative point offset", me); return TC2LI_ERR_INVALID; }
    for (int p = 0; p < n_problems; ++p)
        if (point_offsets[p + 1] < point_offsets[p]) { set_error("%s: point offsets not ascending", me); return TC2LI_ERR_INVALID; }
    const size_t n_records = (size_t)(point_offsets[n_problems] - point_offsets[0]);
    if (n_records > 0 && !points) { set_error("%s: null points", me); return TC2LI_ERR_INVALID; }
    // ---- the slots every problem names, as they are now ----
    size_t n_pairs = 0, n_slots = 0, hp_bytes = 0;
    std::vector<SlotInfo> kf_info;  // per problem: current, then the neighbours
    {
        std::lock_guard<std::mutex> lk(S->info_mu);
        for (int p = 0; p < n_problems; ++p) {
            const tc2li_new_points_problem& P = problems[p];
            if (P.n_neighbours < 0 || (P.n_neighbours > 0 && !P.neighbours) || !P.poses7 || !P.has_point) { set_error("%s: problem %d: invalid argument", me, p); return TC2LI_ERR_INVALID; }
            for (int k = 0; k <= P.n_neighbours; ++k) {
                const int s = k == 0 ? P.current : P.neighbours[k - 1];
                if (!slot_in_range(S, s) || S->info[s].n < 0) { set_error("%s: problem %d names slot %d, which is empty or out of range", me, p, s); return TC2LI_ERR_INVALID; }
                const SlotInfo& si = S->info[s];
                if (si.n_levels > n_levels) { set_error("%s: slot %d holds octave %d, the tables have %d levels", me, s, si.n_levels - 1, n_levels); return TC2LI_ERR_INVALID; }
                if (si.n > 0 && !P.has_point[k]) { set_error("%s: problem %d: null has_point", me, p); return TC2LI_ERR_INVALID; }
                kf_info.push_back(si);
                hp_bytes += a16((size_t)si.n);
            }
            n_pairs += (size_t)P.n_neighbours;
            n_slots += (size_t)P.n_neighbours * (size_t)kf_info[kf_info.size() - 1 - P.n_neighbours].n;
        }
    }
    if (n_pairs > 0x7fffffffULL / 12 || n_slots > 0x7fffffffULL) { set_error("%s: batch too large", me); return TC2LI_ERR_CAPACITY; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    SpaceLease lease;
    BatchSpace& W = *lease.s;
    // ---- layout of the one upload, the work arrays and the one download ----
    Packer in, work, out;
    const size_t i_prob = in.take((size_t)n_problems * sizeof(MappingDev)), i_out = in.take((size_t)n_problems * sizeof(NewPointsOut));
    const size_t i_neigh = in.take(n_pairs * sizeof(KfDev)), i_pair = in.take(n_pairs * sizeof(PairRef));
    const size_t i_scale = in.take(4 * (size_t)n_levels), i_sigma = in.take(4 * (size_t)n_levels), i_hp = in.take(hp_bytes);
    const size_t w_match = work.take(4 * n_slots), w_ok = work.take(n_slots), w_x3D = work.take(12 * n_slots), w_cnt = work.take(4 * n_pairs);
    const size_t r_count = out.take(4 * (size_t)n_problems), r_rec = out.take(32 * n_records);
    const size_t in_bytes = in.off, work_bytes = work.off, out_bytes = out.off;
    TC2LI_HIP_CHECK(W.d_in.ensure(in_bytes)); TC2LI_HIP_CHECK(W.h_in.ensure(in_bytes)); TC2LI_HIP_CHECK(W.d_work.ensure(work_bytes));
    TC2LI_HIP_CHECK(W.d_out.ensure(out_bytes)); TC2LI_HIP_CHECK(W.h_out.ensure(out_bytes));
    uint8_t *H = W.h_in.p, *D = W.d_in.p;
    MappingDev* h_prob = reinterpret_cast<MappingDev*>(H + i_prob);
    NewPointsOut* h_out = reinterpret_cast<NewPointsOut*>(H + i_out);
    KfDev* h_neigh = reinterpret_cast<KfDev*>(H + i_neigh);
    PairRef* h_pair = reinterpret_cast<PairRef*>(H + i_pair);
    memcpy(H + i_scale, scale_factors, 4 * (size_t)n_levels);
    memcpy(H + i_sigma, level_sigma2, 4 * (size_t)n_levels);
    size_t pair = 0, slot = 0, hp = 0, kf = 0;
    int max_entries = 0, max_keys = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_new_points_problem& P = problems[p];
        auto resident = [&](int k) {  // keyframe k of the problem: the store's arrays, this call's pose and has_point
            const SlotInfo& si = kf_info[kf + k];
            KfDev d = S->view(k == 0 ? P.current : P.neighbours[k - 1], si);
            if (si.n > 0) memcpy(H + i_hp + hp, P.has_point[k], (size_t)si.n);
            d.has_point = D + i_hp + hp;
            hp += a16((size_t)si.n);
            set_pose(d, P.poses7 + 7 * (size_t)k);
            return d;
        };
        MappingDev m{};
        m.cur = resident(0);
        for (int j = 0; j < P.n_neighbours; ++j) {
            KfDev& k2 = h_neigh[pair + j];
            k2 = resident(1 + j);
            pair_constants(m.cur, k2, cam);
            k2.skip = baseline(m.cur, k2) < mb ? 1 : 0;  // LocalMapping.cc:456-460 (stereo / RGB-D branch)
            h_pair[pair + j] = PairRef{p, j};
        }
        m.neigh = reinterpret_cast<const KfDev*>(D + i_neigh) + pair; m.n_neigh = P.n_neighbours; m.n_levels = n_levels;
        m.fx = (float)cam->fx; m.fy = (float)cam->fy; m.cx = (float)cam->cx; m.cy = (float)cam->cy; m.mb = mb; m.mbf = (float)cam->bf;
        m.ratio_factor = 1.5f * scale_factor; m.th_far = P.th_far_points;
        m.inertial = P.inertial; m.far_points = P.far_points; m.only_stereo = 0; m.coarse = P.coarse;
        m.scale_factors = reinterpret_cast<const float*>(D + i_scale); m.level_sigma2 = reinterpret_cast<const float*>(D + i_sigma);
        m.match = reinterpret_cast<int32_t*>(W.d_work.p + w_match) + slot; m.ok = W.d_work.p + w_ok + slot;
        m.x3D = reinterpret_cast<float*>(W.d_work.p + w_x3D) + 3 * slot;
        h_prob[p] = m;
        h_out[p] = NewPointsOut{(int32_t)pair, point_offsets[p] - point_offsets[0], point_offsets[p + 1] - point_offsets[p], 0};
        if (P.n_neighbours > 0) { max_entries = std::max(max_entries, kf_info[kf].n_entries); max_keys = std::max(max_keys, m.cur.n); }
        pair += (size_t)P.n_neighbours; slot += (size_t)P.n_neighbours * (size_t)m.cur.n; kf += 1 + (size_t)P.n_neighbours;
    }
    TC2LI_HIP_CHECK(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, st));
    if (n_slots) {
        TC2LI_HIP_CHECK(hipMemsetAsync(W.d_work.p + w_match, 0xff, 4 * n_slots, st));
        TC2LI_HIP_CHECK(hipMemsetAsync(W.d_work.p + w_ok, 0, n_slots, st));
    }
    launch_new_points_batch(reinterpret_cast<const MappingDev*>(D + i_prob), n_problems, reinterpret_cast<const PairRef*>(D + i_pair), (int)n_pairs,
                            max_entries, max_keys, reinterpret_cast<const NewPointsOut*>(D + i_out), reinterpret_cast<int32_t*>(W.d_work.p + w_cnt),
                            reinterpret_cast<int32_t*>(W.d_out.p + r_count), W.d_out.p + r_rec, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(W.h_out.p, W.d_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    const int32_t* counts = reinterpret_cast<const int32_t*>(W.h_out.p + r_count);
    long total = 0;
    int short_of = -1;
    for (int p = 0; p < n_problems; ++p) {
        n_points[p] = counts[p];
        const int room = point_offsets[p + 1] - point_offsets[p];
        if (counts[p] > room && short_of < 0) short_of = p;
        const int keep = std::min(counts[p], room);
        if (keep > 0) memcpy(points + point_offsets[p], W.h_out.p + r_rec + 32 * (size_t)(point_offsets[p] - point_offsets[0]), 32 * (size_t)keep);
        total += keep;
    }
    if (short_of >= 0) {
        set_error("%s: problem %d creates %d points, room for %d", me, short_of, counts[short_of], point_offsets[short_of + 1] - point_offsets[short_of]);
        return TC2LI_ERR_CAPACITY;
    }
    return (int)std::min<long>(total, 0x7fffffffL);
}

extern "C" int tc2li_fuse_search_batch(tc2li_keyframe_store* S, const tc2li_fuse_item* items, int n_items, const float cam4[4], float bf,
                                       const float* scale_factors, const float* inv_level_sigma2, int n_levels, float log_scale_factor,
                                       const tc2li_map_point* points, int n_points_total, const uint8_t* valid, int n_valid_total,
                                       int32_t* best_idx, int32_t* best_dist, int32_t* n_fused, void* stream_) {
    const char* me = "tc2li_fuse_search_batch";
    if (!S || n_items < 0 || (n_items > 0 && (!items || !n_fused)) || !cam4 || !scale_factors || !inv_level_sigma2 || n_levels < 1 || n_points_total < 0 ||
        n_valid_total < 0 || (n_points_total > 0 && !points) || (n_valid_total > 0 && (!valid || !best_idx)) || !(log_scale_factor > 0)) {
        set_error("%s: invalid argument", me);
        return TC2LI_ERR_INVALID;
    }
    if (n_items == 0) return 0;
    std::vector<SlotInfo> info(n_items);
    int max_points = 0;
    {
        std::lock_guard<std::mutex> lk(S->info_mu);
        for (int k = 0; k < n_items; ++k) {
            const tc2li_fuse_item& it = items[k];
            if (!slot_in_range(S, it.keyframe) || S->info[it.keyframe].n < 0) { set_error("%s: item %d names slot %d, which is empty or out of range", me, k, it.keyframe); return TC2LI_ERR_INVALID; }
            if (it.n_points < 0 || it.first_point < 0 || it.first_valid < 0 || (int64_t)it.first_point + it.n_points > n_points_total ||
                (int64_t)it.first_valid + it.n_points > n_valid_total) {
                set_error("%s: item %d: point range outside the arrays", me, k);
                return TC2LI_ERR_INVALID;
            }
            info[k] = S->info[it.keyframe];
            if (info[k].n_levels > n_levels) { set_error("%s: slot %d holds octave %d, the tables have %d levels", me, it.keyframe, info[k].n_levels - 1, n_levels); return TC2LI_ERR_INVALID; }
            max_points = std::max(max_points, it.n_points);
        }
    }
    for (int i = 0; i < n_valid_total; ++i) { best_idx[i] = -1; if (best_dist) best_dist[i] = 256; }
    for (int k = 0; k < n_items; ++k) n_fused[k] = 0;
    if (max_points == 0) return 0;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = stream_ ? (hipStream_t)stream_ : private_stream();
    SpaceLease lease;
    BatchSpace& W = *lease.s;
    Packer in, out;
    const size_t i_item = in.take((size_t)n_items * sizeof(FuseDev)), i_scale = in.take(4 * (size_t)n_levels), i_sigma = in.take(4 * (size_t)n_levels);
    const size_t i_pts = in.take(68 * (size_t)n_points_total), i_valid = in.take((size_t)n_valid_total);
    const size_t r_idx = out.take(4 * (size_t)n_valid_total), r_dist = out.take(4 * (size_t)n_valid_total);
    const size_t in_bytes = in.off, out_bytes = out.off;
    TC2LI_HIP_CHECK(W.d_in.ensure(in_bytes)); TC2LI_HIP_CHECK(W.h_in.ensure(in_bytes)); TC2LI_HIP_CHECK(W.d_out.ensure(out_bytes)); TC2LI_HIP_CHECK(W.h_out.ensure(out_bytes));
    uint8_t *H = W.h_in.p, *D = W.d_in.p;
    memcpy(H + i_scale, scale_factors, 4 * (size_t)n_levels);
    memcpy(H + i_sigma, inv_level_sigma2, 4 * (size_t)n_levels);
    memcpy(H + i_pts, points, 68 * (size_t)n_points_total);
    memcpy(H + i_valid, valid, (size_t)n_valid_total);
    FuseDev* h_item = reinterpret_cast<FuseDev*>(H + i_item);
    for (int k = 0; k < n_items; ++k) {
        const tc2li_fuse_item& it = items[k];
        const SlotInfo& si = info[k];
        const KfDev kd = S->view(it.keyframe, si);
        FuseDev f{};
        f.keys = kd.keys; f.desc = kd.desc; f.u_right = kd.u_right; f.cell_start = S->cell_start(it.keyframe); f.items = S->items(it.keyframe);
        f.n_keys = si.n; f.n_points = it.n_points; f.n_levels = n_levels;
        memcpy(f.q, it.pose7, 16); memcpy(f.t, it.pose7 + 4, 12);
        Q7 T; memcpy(T.q, it.pose7, 16); memcpy(T.t, it.pose7 + 4, 12);
        const Q7 Tw = inv7(T);
        memcpy(f.Ow, Tw.t, 12);
        f.fx = cam4[0]; f.fy = cam4[1]; f.cx = cam4[2]; f.cy = cam4[3]; f.bf = bf; f.th = it.th; f.log_scale_factor = log_scale_factor;
        f.min_x = si.bounds[0]; f.max_x = si.bounds[1]; f.min_y = si.bounds[2]; f.max_y = si.bounds[3];
        f.scale_factors = reinterpret_cast<const float*>(D + i_scale); f.inv_level_sigma2 = reinterpret_cast<const float*>(D + i_sigma);
        f.points = D + i_pts + 68 * (size_t)it.first_point; f.valid = D + i_valid + it.first_valid;
        f.best_idx = reinterpret_cast<int32_t*>(W.d_out.p + r_idx) + it.first_valid; f.best_dist = reinterpret_cast<int32_t*>(W.d_out.p + r_dist) + it.first_valid;
        h_item[k] = f;
    }
    TC2LI_HIP_CHECK(hipMemcpyAsync(D, H, in_bytes, hipMemcpyHostToDevice, st));
    launch_fuse_search_batch(reinterpret_cast<const FuseDev*>(D + i_item), n_items, max_points, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(W.h_out.p, W.d_out.p, out_bytes, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    const int32_t* bi = reinterpret_cast<const int32_t*>(W.h_out.p + r_idx);
    const int32_t* bd = reinterpret_cast<const int32_t*>(W.h_out.p + r_dist);
    long total = 0;
    for (int k = 0; k < n_items; ++k) {
        const tc2li_fuse_item& it = items[k];
        if (it.n_points == 0) continue;
        memcpy(best_idx + it.first_valid, bi + it.first_valid, 4 * (size_t)it.n_points);
        if (best_dist) memcpy(best_dist + it.first_valid, bd + it.first_valid, 4 * (size_t)it.n_points);
        int c = 0;
        for (int i = 0; i < it.n_points; ++i) c += bi[it.first_valid + i] >= 0;
        n_fused[k] = c;
        total += c;
    }
    return (int)std::min<long>(total, 0x7fffffffL);
}

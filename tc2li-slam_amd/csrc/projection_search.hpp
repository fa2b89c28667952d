// The host driver every projection search shares (tracking_host.cpp: TrackWithMotionModel / TrackLocalMap; reloc_host.cpp: the keyframe
// overload and the refinement ladder): the scratch buffers of a search, MapPoint::PredictScale on the host for ratios on a level boundary,
// the list-form matcher with its fall-back to the one-kernel form, the keyframe points' tables, the pose-optimisation tail (also bow_host.cpp's)
// and the small helpers those entry points had a copy of each.  Every table of a call has its place from a Packer (packed_batch.hpp).
#pragma once
#include <cmath>
#include <cstring>
#include <functional>

#include "common.hpp"
#include "matcher_device.hpp"
#include "orb_handle.hpp"
#include "packed_batch.hpp"
#include "pose_opt_device.hpp"
#include "tracking_device.hpp"

namespace tc2li {

// MapPoint::PredictScale (SF/src/MapPoint.cc:540-555) with the host library's logf: the one definition
inline int predict_scale_level(float ratio, float log_scale, int n_levels) {
    int level = (int)ceilf(logf(ratio) / log_scale);
    if (level < 0) level = 0; else if (level >= n_levels) level = n_levels - 1;
    return level;
}

// ---- argument checks of the entry points that search the features of the last tc2li_orb_extract_batch call (orb_features_ready) ----
// item >= 0: the frame is item `item` of the caller's list
inline int check_capacity(const char* fn, int n_keys, int capacity, int item = -1) {
    if (n_keys <= capacity) return TC2LI_OK;
    if (item < 0) set_error("%s: capacity %d < %d keypoints", fn, capacity, n_keys);
    else set_error("%s: capacity %d < %d keypoints of item %d", fn, capacity, n_keys, item);
    return TC2LI_ERR_CAPACITY;
}
inline int check_match_keys(const char* fn, int n_keys, int item = -1) {
    if (n_keys <= kMaxMatchKeys) return TC2LI_OK;
    if (item < 0) set_error("%s: frame has %d keypoints, the matcher supports %d", fn, n_keys, kMaxMatchKeys);
    else set_error("%s: item %d has %d keypoints, the matcher supports %d", fn, item, n_keys, kMaxMatchKeys);
    return TC2LI_ERR_CAPACITY;
}

// ---- TrackConst ----
inline TrackConst track_const(const float cam4[4], const float* scale, int n_levels, float log_scale, int capacity) {
    TrackConst C;
    memset(&C, 0, sizeof(C));
    memcpy(C.cam4, cam4, 4 * sizeof(float));
    C.n_levels = n_levels; C.capacity = capacity; C.log_scale = log_scale;
    for (int l = 0; l < n_levels; ++l) C.scale[l] = scale[l];
    return C;
}
inline TrackConst track_const(const tc2li_orb* o, const tc2li_camera* cam, float b, int capacity) {
    const float cam4[4] = {(float)cam->fx, (float)cam->fy, (float)cam->cx, (float)cam->cy};
    // mfLogScaleFactor = log(mfScaleFactor) (SF/src/Frame.cc:96)
    TrackConst C = track_const(cam4, o->scale.data(), o->prm.nlevels, std::log(o->prm.scale_factor), capacity);
    C.b = b; C.bf = (float)cam->bf;
    for (int l = 0; l < C.n_levels; ++l) C.inv_sigma2[l] = o->inv_sigma2[l];
    C.cols = o->cur_w; C.rows = o->cur_h;
    return C;
}

// ---- the keyframe's points of the keyframe overload (tc2li_projection_keyframe_item / tc2li_reloc_hypothesis), query-indexed ----
struct OrbDescriptor { uint8_t b[32]; };
struct KeyframePointTables {
    Table<uint8_t> has_point;
    Table<float> Xw, min_distance, max_distance, max_distance_raw, angle;  // Xw: [3] each
    Table<OrbDescriptor> desc;
};
// the places of q1 points in the caller's upload block
inline KeyframePointTables take_keyframe_points(Packer& io, size_t q1) {
    KeyframePointTables S;
    S.has_point = io.take<uint8_t>(q1); S.Xw = io.take<float>(3 * q1); S.desc = io.take<OrbDescriptor>(q1); S.min_distance = io.take<float>(q1);
    S.max_distance = io.take<float>(q1); S.max_distance_raw = io.take<float>(q1); S.angle = io.take<float>(q1);
    return S;
}
// packs the points of `it` at query offset q
template <typename Item>
void stage_keyframe_points(const PackedTransfer& T, const KeyframePointTables& S, size_t q, const Item& it) {
    const size_t n = (size_t)it.n_points;
    uint8_t* hp = T.host(S.has_point) + q;
    for (size_t i = 0; i < n; ++i) hp[i] = it.has_point[i] ? 1 : 0;
    T.io.put(S.Xw, 3 * q, it.Xw, 3 * n); T.io.put(S.desc, q, it.point_descriptors, n); T.io.put(S.min_distance, q, it.min_distance, n);
    T.io.put(S.max_distance, q, it.max_distance, n); T.io.put(S.max_distance_raw, q, it.max_distance_raw, n); T.io.put(S.angle, q, it.angle, n);
}
inline KeyframePointArrays keyframe_point_arrays(const PackedTransfer& T, const KeyframePointTables& S, const uint8_t* d_found) {
    return KeyframePointArrays{T.dev(S.has_point), d_found, T.dev(S.Xw), T.dev(S.desc)->b, T.dev(S.min_distance), T.dev(S.max_distance),
                               T.dev(S.max_distance_raw), T.dev(S.angle)};
}

// ---- Optimizer::PoseOptimization behind a search: its eight device tables for (n_frames, n_edges), taken from the work Packer, and the
// launch over them.  A caller's kernels write probs, edges, Xw, edge_kp and poses before and read outlier and inliers after. ----
struct PoseTail {
    Table<PoseProblem> probs;
    Table<BaEdge> edges;
    Table<double> Xw, poses, chi2;
    Table<int32_t> edge_kp, inliers;
    Table<uint8_t> outlier;
    PoseTail(Packer& work, size_t n_frames, size_t n_edges) {
        probs = work.take<PoseProblem>(n_frames); edges = work.take<BaEdge>(n_edges); Xw = work.take<double>(3 * n_edges);
        edge_kp = work.take<int32_t>(n_edges); poses = work.take<double>(7 * n_frames); outlier = work.take<uint8_t>(n_edges);
        chi2 = work.take<double>(n_edges); inliers = work.take<int32_t>(n_frames);
    }
    void launch(const PackedTransfer& T, int n_frames, const tc2li_camera* cam, int max_edges, hipStream_t st, PoseFloats floats = PoseFloats::kUnknown) const {
        CameraD cd;
        memcpy(&cd, cam, sizeof(cd));
        launch_pose_optimization(T.dev_work(probs), n_frames, T.dev_work(Xw), T.dev_work(edges), cd, T.dev_work(poses), T.dev_work(outlier),
                                 T.dev_work(chi2), T.dev_work(inliers), max_edges, st, floats);
    }
};

// ---- the buffers of a search: one per work space (TrackWs, KfSearchWs, LadderWs) ----
struct SearchScratch {
    DevBuf<MatchQuery> d_queries;                                                               // [total_q]
    DevBuf<int32_t> d_query_frame, d_match, d_prev, d_cand_off, d_cand_cnt, d_amb_ids, d_amb_level;  // [total_q]
    DevBuf<float> d_amb_ratio, d_amb_r;                                                         // [total_q]
    DevBuf<int32_t> d_rounds, d_nmatch;                                                         // [n_frames]
    DevBuf<int32_t> d_cell_start;                                                               // [n_frames][kCellsPlus1]
    DevBuf<int32_t> d_small;                                                                    // pool_top [2], amb_count [1]
    DevBuf<uint16_t> d_items;                                                                   // [n_frames][capacity]
    DevBuf<uint32_t> d_pool;                                                                    // [pool_cap]
    PinnedBuf<int32_t> h_small, h_amb_level;                                                    // as d_small; [total_q]
    PinnedBuf<float> h_amb_ratio;                                                               // [total_q]
    int pool_cap = 0;  // TC2LI_MATCH_POOL_PER_QUERY (default 32) entries per query

    int32_t* pool_top() const { return d_small.p; }
    int32_t* amb_count() const { return d_small.p + 2; }
    int ensure(int n_frames, int total_q, int capacity);
};

// After the query kernel (launch_track_queries_local / _keyframe with s.amb_count(), s.d_amb_ids, s.d_amb_ratio, s.d_amb_r; the caller
// zeroes the count before): the listed ratios get their level from predict_scale_level and `patch` writes level and window of those
// queries.  Waits for the stream once, twice when something is listed.
using PatchLauncher = void (*)(const int32_t* ids, const int32_t* levels, const float* r, int n, const TrackConst& C, MatchQuery* queries, hipStream_t st);
int resolve_ambiguous_levels(SearchScratch& s, const TrackConst& C, PatchLauncher patch, hipStream_t st);

struct SearchPass {
    const MatchFrameDev* d_mframes;   // [n_pass], on the device
    const int32_t* d_key_base;        // [n_pass]: where the frame's keys start in d_items
    int n_pass, total_q;
    const TrackFrameDev* h_frames;    // host records; frame k of the pass is h_frames[h_pass ? h_pass[k] : k]
    const int32_t* h_pass;
    int mode;
    float nn_ratio;
    int orb_dist;
    // frame_grids of the handle the pass searches, or NULL: the search builds the grids of its frames itself.  With them d_key_base[k] is
    // where frame k's items start in grid_items and d_cell_row[k] its row of grid_cells (the frame's index in the handle's extraction).
    int32_t* grid_cells = nullptr;
    uint16_t* grid_items = nullptr;
    const int32_t* d_cell_row = nullptr;
};

// The feature grids of the handle's last extraction for a search on stream st: built on st by the first call after the extraction, later
// calls on other streams wait for that build.  Row f of cell_start is frame f (image 2 f), its items start at last_kp_off[2 f].
// TC2LI_MATCH_GRID_CACHE=0 (read per call): cell_start comes back NULL and the search builds its own grids, as before.
struct FrameGrids {
    int32_t* cell_start = nullptr;
    uint16_t* items = nullptr;
};
int frame_grids(tc2li_orb* o, hipStream_t st, FrameGrids* out);
// The search of one pass into s.d_match: queues the list form, then `behind` (what the caller wants queued before the single wait; may be
// empty), waits, and when the candidate pool overflowed resets the pass's matches and queues the one-kernel form -- same result -- and
// `behind` again with a second wait.  Without `behind` the fall-back is left queued: the caller's follow-up kernels go behind it.
// `behind` must overwrite what it writes: after a fall-back it has run on a partial match list before.
int projection_search(SearchScratch& s, const SearchPass& P, hipStream_t st, const std::function<int()>& behind = nullptr);

}  // namespace tc2li

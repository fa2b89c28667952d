// Host side of tc2li_track_motion_model_batch / tc2li_track_local_map_batch (include/tc2li_hip.h): the data path of
// Tracking::TrackWithMotionModel (SF/src/Tracking.cc:2737-2834) and Tracking::TrackLocalMap (:3119-3230) for a batch of independent
// frames.  Everything per keypoint / per map point runs on the device (tracking_kernels.hip: query construction, rotation filter, edge
// lists, outlier bookkeeping; matcher_kernels.hip: the search; pose_opt_kernel.hip: Optimizer::PoseOptimization).  The host packs the
// callers' arrays into one pinned staging block per call (one upload), decides the few per-frame branches the reference takes between the
// stages (fewer than 20 matches: search again with a wider window, Tracking.cc:2774-2783) and receives the per-frame results.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "balm_math.hpp"  // quat_rotate_f
#include "common.hpp"
#include "matcher_device.hpp"
#include "orb_handle.hpp"
#include "packed_batch.hpp"
#include "pose_opt_device.hpp"
#include "projection_search.hpp"
#include "tracking_device.hpp"

using namespace tc2li;

namespace {

struct TrackWs {
    PackedBuffers b;             // the call's upload block and its device-only tables
    PinnedBuf<int32_t> h_nmatch;
    SearchScratch s;
};
// one work space per host thread: TrackWithMotionModel and TrackLocalMap of different batches run side by side
TrackWs& tws() { static thread_local TrackWs w; return w; }

// The searches of one call: SearchByProjection for the frames of a pass, the rotation filter and the match counts.
struct Pass {
    TrackWs& w;
    PackedTransfer& T;
    tc2li_orb* o;
    int n_frames, total_q, capacity;
    int mode;
    float nn_ratio;
    bool check_orientation;
    hipStream_t st;
    const float* d_ur = nullptr;     // [n_frames][capacity]
    const uint8_t* d_occ = nullptr;  // [n_frames][capacity] or NULL
    Table<TrackFrameDev> frames;     // [n_frames], the last table of the block's one upload
    Table<MatchFrameDev> mframes;    // [n_pass], this and the next two: rewritten and uploaded per pass
    Table<int32_t> key_base, pass;

    // after the caller's tables: the passes' own, and every buffer of the call, once; the first pass holds every frame
    int prepare() {
        frames = T.io.take<TrackFrameDev>(n_frames);
        T.outputs_begin();
        mframes = T.io.take<MatchFrameDev>(n_frames); key_base = T.io.take<int32_t>(n_frames); pass = T.io.take<int32_t>(n_frames);
        TC2LI_HIP_CHECK(T.ensure(w.b)); TC2LI_HIP_CHECK(w.h_nmatch.ensure(n_frames));
        if (int rc = w.s.ensure(n_frames, total_q, capacity)) return rc;
        for (int f = 0; f < n_frames; ++f) T.host(pass)[f] = f;
        return TC2LI_OK;
    }
    // frames of the pass are in host(pass)[0 .. n_pass); their TrackFrameDev (slot set) are on the device already.  Returns with the
    // stream drained and w.h_nmatch holding every frame's count (the pass rewrote its own): the count rides behind the list form.
    int search(int n_pass) {
        FrameGrids G;  // the handle's grids: frame k of the pass reads row pass[k], its items start where its keys start
        if (int rc = frame_grids(o, st, &G)) return rc;
        const TrackFrameDev* h_frames = T.host(frames);
        const int32_t* h_pass = T.host(pass);
        for (int k = 0; k < n_pass; ++k) {
            const int f = h_pass[k];
            const TrackFrameDev& F = h_frames[f];
            T.host(mframes)[k] = MatchFrameDev{o->d_mkeys.p + F.key_off, o->d_desc.p + (size_t)F.key_off * 32, d_ur + (size_t)f * capacity,
                                               d_occ ? d_occ + (size_t)f * capacity : nullptr, w.s.d_queries.p + F.q_off, F.n_keys, F.n_q, F.q_off, 0,
                                               0.0f, (float)o->cur_w, 0.0f, (float)o->cur_h};
            T.host(key_base)[k] = G.cell_start ? F.key_off : f * capacity;
        }
        TC2LI_HIP_CHECK(T.upload(mframes, 0, n_pass, st)); TC2LI_HIP_CHECK(T.upload(key_base, 0, n_pass, st)); TC2LI_HIP_CHECK(T.upload(pass, 0, n_pass, st));
        const SearchPass P{T.dev(mframes), T.dev(key_base), n_pass, total_q, h_frames, h_pass, mode, nn_ratio, kMatchThHigh,
                           G.cell_start, G.items, G.cell_start ? T.dev(pass) : nullptr};
        return projection_search(w.s, P, st, [&]() -> int {
            launch_track_count(T.dev(frames), T.dev(pass), n_pass, w.s.d_queries.p, o->d_angles.p, check_orientation ? 1 : 0, w.s.d_match.p, w.s.d_nmatch.p, st);
            TC2LI_HIP_CHECK(hipGetLastError());
            TC2LI_HIP_CHECK(hipMemcpyAsync(w.h_nmatch.p, w.s.d_nmatch.p, n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, st));
            return TC2LI_OK;
        });
    }
};

}  // namespace

extern "C" int tc2li_track_motion_model_batch(tc2li_orb* o, int n_frames, const tc2li_keypoint* keypoints, const float* u_right,
                                              int capacity, const tc2li_last_frame* last, const float* pose_pred7,
                                              const tc2li_camera* cam, float b, float th, double* poses7,
                                              int32_t* map_point_of_keypoint, int32_t* n_matches, int32_t* n_inliers, void* stream_) {
    const char* fn = "tc2li_track_motion_model_batch";
    if (!o || n_frames < 0 || capacity < 0 || !keypoints || !u_right || !last || !pose_pred7 || !cam || !poses7 || !map_point_of_keypoint ||
        !n_matches || !n_inliers) {
        set_error("%s: invalid argument", fn);
        return TC2LI_ERR_INVALID;
    }
    if (n_frames == 0) return 0;
    if (!orb_features_ready(o, n_frames, fn)) return TC2LI_ERR_INVALID;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream_;
    static const bool kTiming = getenv("TC2LI_TRACK_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tm[6] = {0, 0, 0, 0, 0, 0}, t0 = now();
    TrackWs& w = tws();
    SearchScratch& S = w.s;
    const TrackConst C = track_const(o, cam, b, capacity);
    const int L = C.n_levels;

    std::vector<TrackFrameDev> frames(n_frames);
    int total_q = 0;
    for (int f = 0; f < n_frames; ++f) {
        TrackFrameDev& F = frames[f];
        memset(&F, 0, sizeof(F));
        F.key_off = o->last_kp_off[2 * f];
        F.n_keys = o->last_kp_cnt[2 * f];
        if (int rc = check_capacity(fn, F.n_keys, capacity)) return rc;
        if (int rc = check_match_keys(fn, F.n_keys)) return rc;
        if (last[f].n < 0 || (last[f].n > 0 && (!last[f].has_point || !last[f].outlier || !last[f].Xw || !last[f].keys || !last[f].descriptors))) {
            set_error("tc2li_track_motion_model_batch: last frame %d has null arrays", f);
            return TC2LI_ERR_INVALID;
        }
        F.q_off = total_q; F.n_q = last[f].n;
        total_q += last[f].n;
        memcpy(F.pose7, pose_pred7 + 7 * (size_t)f, 7 * sizeof(float));
        memcpy(F.last_pose7, last[f].pose7, 7 * sizeof(float));
        F.th = th; F.slot = f;
        // forward / backward (ORBmatcher.cc:1703-1708): tlc = Tlw * twc
        float twc[3], tlc[3];
        const float qi[4] = {-F.pose7[0], -F.pose7[1], -F.pose7[2], F.pose7[3]};
        const float nt[3] = {F.pose7[4] * -1.f, F.pose7[5] * -1.f, F.pose7[6] * -1.f};
        quat_rotate_f(qi, nt, twc);
        quat_rotate_f(F.last_pose7, twc, tlc);
        for (int c = 0; c < 3; ++c) tlc[c] += F.last_pose7[4 + c];
        F.forward = tlc[2] > b; F.backward = -tlc[2] > b;
    }
    // ---- the upload block: the last frames' points (structure of arrays), mvuRight of the current frames, the frame records; the
    // device-only tables: the keypoints' map points, the inlier counts, PoseOptimization's ----
    const size_t nq = (size_t)std::max(total_q, 1), nk = (size_t)n_frames * std::max(capacity, 1), ne = nk;
    PackedTransfer T;
    const auto t_flags = T.io.take<uint8_t>(nq);
    const auto t_Xw = T.io.take<float>(3 * nq), t_ang = T.io.take<float>(nq), t_ur = T.io.take<float>(nk);
    const auto t_oct = T.io.take<int32_t>(nq);
    const auto t_desc = T.io.take<OrbDescriptor>(nq);
    const auto t_of_key = T.work.take<int32_t>(ne), t_ninl = T.work.take<int32_t>(n_frames);
    const PoseTail pose(T.work, n_frames, ne);
    Pass pass{w, T, o, n_frames, total_q, capacity, 0, 0.9f, true, st};
    int rc = pass.prepare();
    if (rc != TC2LI_OK) return rc;
    T.io.put(pass.frames, 0, frames.data(), n_frames);
    TrackFrameDev* const h_frames = T.host(pass.frames);
    std::vector<int> bad(n_frames, 0);
    tracking_pool().parallel_for(n_frames, [&](int f) {
        const TrackFrameDev& F = h_frames[f];
        const tc2li_last_frame& lf = last[f];
        uint8_t* fl = T.host(t_flags) + F.q_off;
        float* ang = T.host(t_ang) + F.q_off;
        int32_t* oct = T.host(t_oct) + F.q_off;
        for (int i = 0; i < lf.n; ++i) {
            fl[i] = (uint8_t)((lf.has_point[i] ? 1 : 0) | (lf.outlier[i] ? 2 : 0));
            ang[i] = lf.keys[i].angle;
            oct[i] = lf.keys[i].octave;
            if (fl[i] == 1 && (oct[i] < 0 || oct[i] >= L)) bad[f] = 1;
        }
        T.io.put(t_Xw, 3 * (size_t)F.q_off, lf.Xw, 3 * (size_t)lf.n);
        T.io.put(t_desc, F.q_off, lf.descriptors, lf.n);
        T.io.put(t_ur, (size_t)f * capacity, u_right + (size_t)f * capacity, F.n_keys);
    });
    for (int f = 0; f < n_frames; ++f) if (bad[f]) { set_error("octave out of range"); return TC2LI_ERR_INVALID; }
    tm[0] = now() - t0; t0 = now();
    TC2LI_HIP_CHECK(T.upload(st));
    const TrackFrameDev* d_frames = T.dev(pass.frames);
    const LastFrameArrays A{T.dev(t_flags), T.dev(t_Xw), T.dev(t_ang), T.dev(t_oct), T.dev(t_desc)->b};
    const float* d_ur = pass.d_ur = T.dev(t_ur);
    if (total_q > 0) {
        launch_track_queries_last(d_frames, n_frames, C, A, total_q, S.d_queries.p, S.d_query_frame.p, S.d_match.p, st);
        rc = pass.search(n_frames);
        if (rc != TC2LI_OK) return rc;
        memcpy(n_matches, w.h_nmatch.p, n_frames * sizeof(int32_t));
    } else {
        for (int f = 0; f < n_frames; ++f) n_matches[f] = 0;
        TC2LI_HIP_CHECK(hipMemsetAsync(S.d_nmatch.p, 0, n_frames * sizeof(int32_t), st));
    }
    tm[1] = now() - t0; t0 = now();
    // fewer than 20 matches: wider window (Tracking.cc:2774-2783), those frames only
    int n_retry = 0;
    for (int f = 0; f < n_frames; ++f) {
        TrackFrameDev& F = h_frames[f];
        if (n_matches[f] < 20 && F.n_q > 0) { F.slot = n_retry; F.th = 2 * th; T.host(pass.pass)[n_retry++] = f; }
        else F.slot = -1;
    }
    if (n_retry > 0) {
        TC2LI_HIP_CHECK(T.upload(pass.frames, 0, n_frames, st));
        launch_track_queries_last(d_frames, n_frames, C, A, total_q, S.d_queries.p, S.d_query_frame.p, S.d_match.p, st);
        rc = pass.search(n_retry);
        if (rc != TC2LI_OK) return rc;
        memcpy(n_matches, w.h_nmatch.p, n_frames * sizeof(int32_t));  // d_nmatch holds every frame: the pass rewrote its own
    }
    tm[2] = now() - t0; t0 = now();
    // ---- Optimizer::PoseOptimization: one edge per keypoint that now holds a map point, in keypoint order ----
    auto W = [&](auto t) { return T.dev_work(t); };
    launch_track_edges_last(d_frames, n_frames, C, o->d_mkeys.p, d_ur, S.d_match.p, S.d_nmatch.p, A.Xw, W(t_of_key), W(pose.probs), W(pose.edges), W(pose.Xw),
                            W(pose.edge_kp), W(pose.poses), st);
    pose.launch(T, n_frames, cam, capacity, st, PoseFloats::kByConstruction);  // (the edge kernel widened floats)
    launch_track_finish_last(d_frames, n_frames, capacity, S.d_nmatch.p, W(pose.probs), W(pose.outlier), W(pose.edge_kp), W(pose.inliers), W(t_of_key),
                             W(pose.poses), W(t_ninl), st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(map_point_of_keypoint, W(t_of_key), ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(poses7, W(pose.poses), 7 * (size_t)n_frames * sizeof(double), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_inliers, W(t_ninl), n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    tm[3] = now() - t0;
    if (kTiming) fprintf(stderr, "track timing ms: stage %.3f search %.3f retry %.3f edges+pose-opt+results %.3f\n", tm[0], tm[1], tm[2], tm[3]);
    return n_frames;
}

// The data path of Tracking::TrackLocalMap (SF/src/Tracking.cc:3119-3230) for a batch of independent frames: SearchLocalPoints
// (:3232-3294: isInFrustum + SearchByProjection(F, mvpLocalMapPoints, th, far points) with ORBmatcher(0.8)) on the device-resident
// features, then Optimizer::PoseOptimization over every map point the frame holds, and mnMatchesInliers.
// optimise = false: SearchLocalPoints alone (tc2li_search_local_points_batch) -- with the IMU initialised TrackLocalMap hands the correspondences to
// PoseInertialOptimizationLastFrame / LastKeyFrame (Tracking.cc:2857-2878; tc2li_pose_inertial_optimization_batch) instead of PoseOptimization
static int track_local_map_impl(tc2li_orb* o, int n_frames, const tc2li_keypoint* keypoints, const float* u_right, int capacity,
                                const float* poses7, const uint8_t* held, const float* held_Xw, const tc2li_map_point* local_points,
                                const int32_t* local_offsets, const tc2li_camera* cam, float th, int far_points, float th_far_points,
                                double* poses7_out, int32_t* local_of_keypoint, uint8_t* outlier, int32_t* n_matches,
                                int32_t* n_inliers, void* stream_, const bool optimise) {
    const char* fn = "tc2li_track_local_map_batch";
    if (!o || n_frames < 0 || capacity < 0 || !keypoints || !u_right || !poses7 || !held || !held_Xw || !local_offsets || !cam || !local_of_keypoint || !n_matches ||
        (optimise && (!poses7_out || !outlier || !n_inliers))) {
        set_error("%s: invalid argument", fn);
        return TC2LI_ERR_INVALID;
    }
    if (n_frames == 0) return 0;
    if (!orb_features_ready(o, n_frames, fn)) return TC2LI_ERR_INVALID;
    if (local_offsets[0] != 0) { set_error("tc2li_track_local_map_batch: local_offsets[0] must be 0"); return TC2LI_ERR_INVALID; }
    const int total_q = local_offsets[n_frames];
    if (total_q < 0 || (total_q > 0 && !local_points)) { set_error("tc2li_track_local_map_batch: invalid local points"); return TC2LI_ERR_INVALID; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    static_assert(sizeof(tc2li_map_point) == sizeof(LocalPointDev), "ABI layout");
    hipStream_t st = (hipStream_t)stream_;
    static const bool kTiming = getenv("TC2LI_TRACK_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    double tm[5] = {0, 0, 0, 0, 0}, t0 = now();
    TrackWs& w = tws();
    SearchScratch& S = w.s;
    TrackConst C = track_const(o, cam, 0.f, capacity);
    C.far_points = far_points; C.th_far = th_far_points; C.view_cos_limit = 0.5f;

    std::vector<TrackFrameDev> frames(n_frames);
    for (int f = 0; f < n_frames; ++f) {
        TrackFrameDev& F = frames[f];
        memset(&F, 0, sizeof(F));
        F.key_off = o->last_kp_off[2 * f];
        F.n_keys = o->last_kp_cnt[2 * f];
        if (int rc = check_capacity(fn, F.n_keys, capacity)) return rc;
        if (int rc = check_match_keys(fn, F.n_keys)) return rc;
        if (local_offsets[f + 1] < local_offsets[f]) { set_error("tc2li_track_local_map_batch: local_offsets must not decrease"); return TC2LI_ERR_INVALID; }
        F.q_off = local_offsets[f]; F.n_q = local_offsets[f + 1] - local_offsets[f];
        memcpy(F.pose7, poses7 + 7 * (size_t)f, 7 * sizeof(float));
        F.th = th; F.slot = f;
    }
    // ---- the upload block: the local points, mvuRight, the held flags and positions, the frame records; the device-only tables: the
    // occupied flags, the keypoints' local points and outlier flags, the inlier counts, PoseOptimization's ----
    const size_t nq = (size_t)std::max(total_q, 1), nk = (size_t)n_frames * std::max(capacity, 1), ne = nk;
    PackedTransfer T;
    const auto t_pts = T.io.take<LocalPointDev>(nq);
    const auto t_ur = T.io.take<float>(nk), t_hx = T.io.take<float>(3 * nk);
    const auto t_held = T.io.take<uint8_t>(nk);
    const auto t_occ = T.work.take<uint8_t>(nk), t_outlier_key = T.work.take<uint8_t>(ne);
    const auto t_of_key = T.work.take<int32_t>(ne), t_ninl = T.work.take<int32_t>(n_frames);
    const PoseTail pose(T.work, n_frames, ne);
    Pass pass{w, T, o, n_frames, total_q, capacity, 1, 0.8f, false, st};
    int rc = pass.prepare();
    if (rc != TC2LI_OK) return rc;
    T.io.put(pass.frames, 0, frames.data(), n_frames);
    {
        // the callers' arrays are contiguous: copied in 1 MiB pieces by the pool
        struct Piece { uint8_t* dst; const uint8_t* src; size_t n; };
        std::vector<Piece> pieces;
        auto add = [&](auto t, const void* src, size_t count) {
            const size_t bytes = count * sizeof(*T.host(t));
            for (size_t at = 0; at < bytes; at += (size_t)1 << 20)
                pieces.push_back(Piece{(uint8_t*)T.host(t) + at, static_cast<const uint8_t*>(src) + at, std::min((size_t)1 << 20, bytes - at)});
        };
        add(t_pts, local_points, total_q);
        add(t_ur, u_right, nk); add(t_held, held, nk); add(t_hx, held_Xw, 3 * nk);
        tracking_pool().parallel_for((int)pieces.size(), [&](int k) { memcpy(pieces[k].dst, pieces[k].src, pieces[k].n); });
    }
    tm[0] = now() - t0; t0 = now();
    TC2LI_HIP_CHECK(T.upload(st));
    auto W = [&](auto t) { return T.dev_work(t); };
    const TrackFrameDev* d_frames = T.dev(pass.frames);
    const LocalPointDev* d_pts = T.dev(t_pts);
    const float *d_ur = T.dev(t_ur), *d_hx = T.dev(t_hx);
    const uint8_t* d_held = T.dev(t_held);
    pass.d_ur = d_ur; pass.d_occ = W(t_occ);
    launch_track_occupied(d_held, nk, W(t_occ), st);
    if (total_q > 0) {
        TC2LI_HIP_CHECK(hipMemsetAsync(S.amb_count(), 0, sizeof(int32_t), st));
        launch_track_queries_local(d_frames, n_frames, C, d_pts, total_q, S.d_queries.p, S.d_query_frame.p, S.d_match.p, S.amb_count(), S.d_amb_ids.p,
                                   S.d_amb_ratio.p, S.d_amb_r.p, st);
        // MapPoint::PredictScale on a level boundary: the host's logf decides (see k_track_queries_local).  One count comes back; the
        // listed ratios get their level on the host and a patch kernel writes level and window before the search starts.
        rc = resolve_ambiguous_levels(S, C, launch_track_patch_levels, st);
        if (rc != TC2LI_OK) return rc;
        tm[1] = now() - t0; t0 = now();
        rc = pass.search(n_frames);
        if (rc != TC2LI_OK) return rc;
        memcpy(n_matches, w.h_nmatch.p, n_frames * sizeof(int32_t));
    } else {
        for (int f = 0; f < n_frames; ++f) n_matches[f] = 0;
    }
    tm[2] = now() - t0; t0 = now();
    // ---- Optimizer::PoseOptimization over every map point the frame now holds, in keypoint order ----
    launch_track_edges_local(d_frames, n_frames, C, o->d_mkeys.p, d_ur, S.d_match.p, d_held, d_hx, d_pts, W(t_of_key), W(pose.probs), W(pose.edges), W(pose.Xw),
                             W(pose.edge_kp), W(pose.poses), st);
    if (!optimise) {  // the keypoints' new map points are what the caller wants; the optimisation is the pose-inertial one, elsewhere
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipMemcpyAsync(local_of_keypoint, W(t_of_key), ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
        tm[3] = now() - t0;
        if (kTiming) fprintf(stderr, "search-local-points timing ms: stage %.3f queries %.3f search %.3f results %.3f\n", tm[0], tm[1], tm[2], tm[3]);
        return n_frames;
    }
    pose.launch(T, n_frames, cam, capacity, st, PoseFloats::kByConstruction);  // (the edge kernel widened floats)
    launch_track_finish_local(d_frames, n_frames, capacity, W(pose.probs), W(pose.outlier), W(pose.edge_kp), d_held, W(t_of_key), W(t_outlier_key), W(t_ninl), st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(local_of_keypoint, W(t_of_key), ne * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(outlier, W(t_outlier_key), ne, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(poses7_out, W(pose.poses), 7 * (size_t)n_frames * sizeof(double), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(n_inliers, W(t_ninl), n_frames * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    tm[3] = now() - t0;
    if (kTiming) fprintf(stderr, "track-local-map timing ms: stage %.3f queries %.3f search %.3f edges+pose-opt+results %.3f\n", tm[0], tm[1], tm[2], tm[3]);
    return n_frames;
}

extern "C" int tc2li_track_local_map_batch(tc2li_orb* o, int n_frames, const tc2li_keypoint* keypoints, const float* u_right, int capacity,
                                           const float* poses7, const uint8_t* held, const float* held_Xw, const tc2li_map_point* local_points,
                                           const int32_t* local_offsets, const tc2li_camera* cam, float th, int far_points, float th_far_points,
                                           double* poses7_out, int32_t* local_of_keypoint, uint8_t* outlier, int32_t* n_matches,
                                           int32_t* n_inliers, void* stream_) {
    return track_local_map_impl(o, n_frames, keypoints, u_right, capacity, poses7, held, held_Xw, local_points, local_offsets, cam, th, far_points,
                                th_far_points, poses7_out, local_of_keypoint, outlier, n_matches, n_inliers, stream_, true);
}

// Tracking::SearchLocalPoints (SF/src/Tracking.cc:3232-3294) for a batch of frames: the first half of tc2li_track_local_map_batch, for the
// camera-LiDAR-inertial configuration's TrackLocalMap (the optimiser there is PoseInertialOptimization*)
extern "C" int tc2li_search_local_points_batch(tc2li_orb* o, int n_frames, const tc2li_keypoint* keypoints, const float* u_right, int capacity,
                                               const float* poses7, const uint8_t* held, const float* held_Xw, const tc2li_map_point* local_points,
                                               const int32_t* local_offsets, const tc2li_camera* cam, float th, int far_points, float th_far_points,
                                               int32_t* local_of_keypoint, int32_t* n_matches, void* stream_) {
    return track_local_map_impl(o, n_frames, keypoints, u_right, capacity, poses7, held, held_Xw, local_points, local_offsets, cam, th, far_points,
                                th_far_points, nullptr, local_of_keypoint, nullptr, n_matches, nullptr, stream_, false);
}

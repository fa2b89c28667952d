// tc2li_stereo_points_batch / tc2li_host_stereo_points_batch / tc2li_new_keyframe_batch / tc2li_host_new_keyframe_batch
// (include/tc2li_hip.h "tracking: stereo map points and the keyframe decision"): Tracking::NeedNewKeyFrame (SF/src/Tracking.cc:2942-3076)
// and the stereo map-point creation of CreateNewKeyFrame (:3132-3203), UpdateLastFrame (:2676-2734) and StereoInitialization
// (:2477-2495).  This file validates the frames and either walks them in plain C++ -- the reference's loops, std::sort included -- or
// packs them for stereo_points_kernels.hip.
#include <algorithm>
#include <cstring>
#include <utility>

#include "common.hpp"
#include "packed_batch.hpp"
#include "stereo_points_device.hpp"

namespace tc2li {
namespace {

// 0, or the error code with *what set
int validate_frame(const tc2li_stereo_points_frame& f, bool decide, const char** what) {
    *what = "";
    if (f.n < 0) { *what = "negative n"; return TC2LI_ERR_INVALID; }
    if (f.n > kStereoPointsMaxKeys) { *what = "more than 4096 keypoints"; return TC2LI_ERR_CAPACITY; }
    if (!f.counts) { *what = "null counts"; return TC2LI_ERR_INVALID; }
    if (f.n && (!f.depth || !f.keys || !f.held || !f.created_keypoint || !f.x3D)) { *what = "null depth, keys, held, created_keypoint or x3D"; return TC2LI_ERR_INVALID; }
    if (f.mode != TC2LI_STEREO_POINTS_CLOSEST && f.mode != TC2LI_STEREO_POINTS_ALL) { *what = "unknown mode"; return TC2LI_ERR_INVALID; }
    if (f.max_point < 0) { *what = "negative max_point"; return TC2LI_ERR_INVALID; }
    if (decide && f.n && !f.outlier) { *what = "null outlier"; return TC2LI_ERR_INVALID; }
    if (decide && f.mode != TC2LI_STEREO_POINTS_CLOSEST) { *what = "the new keyframe's points are made in mode CLOSEST"; return TC2LI_ERR_INVALID; }
    for (int i = 0; i < f.n; ++i)
        if (f.held[i] > 2) { *what = "held outside {0, 1, 2}"; return TC2LI_ERR_INVALID; }
    return 0;
}

const char* validate_decision(const tc2li_keyframe_decision& d) {
    if (d.n_ref < 0) return "negative n_ref";
    if (d.inertial && !d.imu_initialized && !d.has_last_kf) return "no last keyframe before the IMU is initialised (the reference dereferences it)";
    if (d.last_reloc_frame_id > 0xffffffffull || d.last_keyframe_id > 0xffffffffull) return "last_reloc_frame_id or last_keyframe_id above 2^32 - 1";
    return "";
}

int validate_all(const char* entry, const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions,
                 const tc2li_keyframe_verdict* verdicts, bool decide, int n_frames, const float* unproject4) {
    if (n_frames < 0 || !unproject4 || (n_frames && (!frames || (decide && (!decisions || !verdicts))))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "frame", n_frames, [&](int f, const char** what) {
        const int code = validate_frame(frames[f], decide, what);
        if (code || !decide) return code;
        *what = validate_decision(decisions[f]);
        return (*what)[0] ? TC2LI_ERR_INVALID : 0;
    });
}

KeyframeDecisionDev pack_decision(const tc2li_keyframe_decision& d) {
    KeyframeDecisionDev o{};
    o.frame_id = d.frame_id; o.time_frame = d.time_frame; o.time_last_kf = d.time_last_kf;
    o.last_reloc_frame_id = (uint32_t)d.last_reloc_frame_id; o.last_keyframe_id = (uint32_t)d.last_keyframe_id;
    o.max_frames = d.max_frames; o.min_frames = d.min_frames; o.n_kfs = d.n_kfs; o.matches_inliers = d.matches_inliers;
    o.n_ref_matches = d.n_ref_matches; o.keyframes_in_queue = d.keyframes_in_queue;
    o.flags = (d.inertial ? newkf::kInertial : 0) | (d.imu_initialized ? newkf::kImuInitialized : 0) | (d.only_tracking ? newkf::kOnlyTracking : 0) |
              (d.mapper_stopped ? newkf::kMapperStopped : 0) | (d.mapper_idle ? newkf::kMapperIdle : 0) |
              (d.mapper_initializing ? newkf::kMapperInitializing : 0) | (d.create_blocked ? newkf::kCreateBlocked : 0) |
              (d.has_last_kf ? newkf::kHasLastKf : 0);
    return o;
}

struct Unproject { float cx, cy, invfx, invfy; };

void create_point(const tc2li_stereo_points_frame& f, const Unproject& u, int i, int* n_created) {
    newkf::unproject(f.keys[i].x, f.keys[i].y, f.depth[i], u.cx, u.cy, u.invfx, u.invfy, f.Rwc, f.Ow, f.x3D + 3 * (size_t)*n_created);
    f.created_keypoint[(*n_created)++] = i;
}

// the loops of :3132-3203 / :2676-2734 (CLOSEST) and :2477-2495 (ALL); create == false: only n_with_depth is counted
void points_one(const tc2li_stereo_points_frame& f, const Unproject& u, bool create) {
    int n_created = 0, n_points = 0, n_with_depth = 0;
    if (f.mode == TC2LI_STEREO_POINTS_ALL && create) {
        for (int i = 0; i < f.n; ++i) {
            if (!newkf::has_depth(f.depth[i])) continue;                             // :2482
            ++n_with_depth;
            if (f.n > 500) create_point(f, u, i, &n_created);                        // :2433
        }
        n_points = n_created;
    } else {
        std::vector<std::pair<float, int>> depth_idx;                                // :3132-3142
        depth_idx.reserve(f.n);
        for (int i = 0; i < f.n; ++i)
            if (newkf::has_depth(f.depth[i])) depth_idx.push_back(std::make_pair(f.depth[i], i));
        n_with_depth = (int)depth_idx.size();
        if (create && !depth_idx.empty()) {
            std::sort(depth_idx.begin(), depth_idx.end());                           // :3146
            for (size_t j = 0; j < depth_idx.size(); ++j) {
                const int i = depth_idx[j].second;
                if (f.held[i] != 1) create_point(f, u, i, &n_created);               // :3156-3162
                ++n_points;                                                          // :3192, :3196
                if (depth_idx[j].first > f.th_depth && n_points > f.max_point) break;   // :3199
            }
        }
    }
    f.counts[0] = n_created; f.counts[1] = n_points; f.counts[2] = n_with_depth;
}

void decide_one(const tc2li_stereo_points_frame& f, const tc2li_keyframe_decision& d, tc2li_keyframe_verdict* v, const Unproject& u) {
    int tracked = 0, non_tracked = 0;
    for (int i = 0; i < f.n; ++i)                                                    // :2988-2998
        if (newkf::close_for_counts(f.depth[i], f.th_depth)) {
            if (f.held[i] != 0 && !f.outlier[i]) ++tracked;
            else ++non_tracked;
        }
    int ref = d.n_ref_matches;
    if (d.ref_nobs) {                                                                // KeyFrame.cc:352-377
        ref = 0;
        for (int i = 0; i < d.n_ref; ++i) ref += newkf::ref_match(d.ref_nobs[i], d.n_kfs);
    }
    tc2li_keyframe_verdict out{};
    newkf::decide(pack_decision(d), tracked, non_tracked, ref, &out);
    out.n_tracked_close = tracked; out.n_non_tracked_close = non_tracked; out.n_ref_matches = ref;
    *v = out;
    points_one(f, u, out.need && !d.create_blocked);
}

int device_batch(const char* entry, const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions, tc2li_keyframe_verdict* verdicts,
                 bool decide, int n_frames, const float* unproject4, void* stream) {
    const int rc = validate_all(entry, frames, decisions, verdicts, decide, n_frames, unproject4);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_frames == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    std::vector<StereoFrameDev> dev(n_frames);
    size_t total = 0, total_ref = 0;
    for (int f = 0; f < n_frames; ++f) {
        const tc2li_stereo_points_frame& in = frames[f];
        StereoFrameDev& d = dev[f];
        d.off = (int32_t)total; d.n = in.n; d.max_point = in.max_point; d.mode = in.mode; d.th_depth = in.th_depth;
        d.ref_off = (int32_t)total_ref; d.n_ref = decide && decisions[f].ref_nobs ? decisions[f].n_ref : -1; d.pad_ = 0;
        memcpy(d.Rwc, in.Rwc, sizeof d.Rwc); memcpy(d.Ow, in.Ow, sizeof d.Ow);
        total += in.n;
        if (d.n_ref > 0) total_ref += d.n_ref;
        if (total_ref > kMaxRows) {
            set_error("%s: the batch up to frame %d has more than 2^31 entries of ref_nobs; split it", entry, f);
            return TC2LI_ERR_INVALID;
        }
    }
    const size_t nf = (size_t)n_frames;
    // one buffer: [inputs | outputs]
    PackedTransfer T;
    Packer& io = T.io;
    const size_t o_frames = io.take(nf * sizeof(StereoFrameDev)), o_dec = io.take(decide ? nf * sizeof(KeyframeDecisionDev) : 0), o_depth = io.take(total * 4),
                 o_xy = io.take(total * 8), o_held = io.take(total), o_outl = io.take(decide ? total : 0), o_ref = io.take(total_ref * 4);
    T.outputs_begin();
    const size_t o_counts = io.take(nf * 12), o_verdict = io.take(decide ? nf * sizeof(tc2li_keyframe_verdict) : 0), o_created = io.take(total * 4),
                 o_x3d = io.take(total * 12);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceStereoPoints>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_frames, 0, dev.data(), nf, sizeof(StereoFrameDev));
    tracking_pool().parallel_for(n_frames, [&](int f) {
        const tc2li_stereo_points_frame& in = frames[f];
        const StereoFrameDev& d = dev[f];
        const size_t n = (size_t)in.n;
        io.put(o_depth, d.off, in.depth, n, 4); io.put(o_held, d.off, in.held, n, 1);
        if (decide) io.put(o_outl, d.off, in.outlier, n, 1);
        float* xy = T.host<float>(o_xy) + 2 * (size_t)d.off;
        for (size_t i = 0; i < n; ++i) { xy[2 * i] = in.keys[i].x; xy[2 * i + 1] = in.keys[i].y; }
        if (decide) {
            T.host<KeyframeDecisionDev>(o_dec)[f] = pack_decision(decisions[f]);
            if (d.n_ref > 0) io.put(o_ref, d.ref_off, decisions[f].ref_nobs, (size_t)d.n_ref, 4);
        }
    });
    TC2LI_HIP_CHECK(T.upload(st));
    StereoPointsBatch B{};
    B.n_frames = n_frames; B.decide = decide ? 1 : 0;
    B.cx = unproject4[0]; B.cy = unproject4[1]; B.invfx = unproject4[2]; B.invfy = unproject4[3];
    B.frames = T.dev<const StereoFrameDev>(o_frames); B.decisions = T.dev<const KeyframeDecisionDev>(o_dec);
    B.depth = T.dev<const float>(o_depth); B.xy = T.dev<const float>(o_xy); B.held = T.dev<const uint8_t>(o_held);
    B.outlier = T.dev<const uint8_t>(o_outl); B.ref_nobs = T.dev<const int32_t>(o_ref);
    B.created_keypoint = T.dev<int32_t>(o_created); B.x3D = T.dev<float>(o_x3d); B.counts = T.dev<int32_t>(o_counts);
    B.verdicts = T.dev<tc2li_keyframe_verdict>(o_verdict);
    launch_stereo_points(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    tracking_pool().parallel_for(n_frames, [&](int f) {
        const tc2li_stereo_points_frame& in = frames[f];
        const int32_t* counts = T.host<const int32_t>(o_counts) + 3 * (size_t)f;
        memcpy(in.counts, counts, 12);
        if (counts[0] > 0) {
            io.get(in.created_keypoint, o_created, dev[f].off, (size_t)counts[0], 4);
            io.get(in.x3D, o_x3d, dev[f].off, (size_t)counts[0], 12);
        }
        if (decide) verdicts[f] = T.host<const tc2li_keyframe_verdict>(o_verdict)[f];
    });
    return n_frames;
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_host_stereo_points_batch(const tc2li_stereo_points_frame* frames, int n_frames, const float unproject4[4]) {
    const int rc = validate_all("tc2li_host_stereo_points_batch", frames, nullptr, nullptr, false, n_frames, unproject4);
    if (rc < 0) return rc;
    const Unproject u{unproject4[0], unproject4[1], unproject4[2], unproject4[3]};
    tracking_pool().parallel_for(n_frames, [&](int f) { points_one(frames[f], u, true); });
    return n_frames;
}

extern "C" int tc2li_stereo_points_batch(const tc2li_stereo_points_frame* frames, int n_frames, const float unproject4[4], void* stream) {
    return device_batch("tc2li_stereo_points_batch", frames, nullptr, nullptr, false, n_frames, unproject4, stream);
}

extern "C" int tc2li_host_new_keyframe_batch(const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions,
                                             tc2li_keyframe_verdict* verdicts, int n_frames, const float unproject4[4]) {
    const int rc = validate_all("tc2li_host_new_keyframe_batch", frames, decisions, verdicts, true, n_frames, unproject4);
    if (rc < 0) return rc;
    const Unproject u{unproject4[0], unproject4[1], unproject4[2], unproject4[3]};
    tracking_pool().parallel_for(n_frames, [&](int f) { decide_one(frames[f], decisions[f], &verdicts[f], u); });
    return n_frames;
}

extern "C" int tc2li_new_keyframe_batch(const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions,
                                        tc2li_keyframe_verdict* verdicts, int n_frames, const float unproject4[4], void* stream) {
    return device_batch("tc2li_new_keyframe_batch", frames, decisions, verdicts, true, n_frames, unproject4, stream);
}

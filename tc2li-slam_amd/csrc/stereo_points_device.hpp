// Device side of tc2li_stereo_points_batch / tc2li_new_keyframe_batch (include/tc2li_hip.h "tracking: stereo map points and the keyframe
// decision"): stereo_points_host.cpp validates and packs the frames, stereo_points_kernels.hip runs one workgroup per frame.  The rules
// that the kernel and the host twins share -- the depth tests, NeedNewKeyFrame's chain, the un-projection -- are the inline functions at
// the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

namespace tc2li {

constexpr int kStereoPointsMaxKeys = TC2LI_STEREO_POINTS_MAX_KEYPOINTS;

// One frame of the packed batch.  The per-keypoint arrays of all frames are concatenated; `off` is where this frame's rows start.
struct StereoFrameDev {
    int32_t off, n;
    int32_t max_point, mode;
    float th_depth;
    int32_t ref_off, n_ref;            // the frame's rows of ref_nobs; n_ref < 0: none given, the decision's n_ref_matches holds
    int32_t pad_;
    float Rwc[9];
    float Ow[3];
};

// tc2li_keyframe_decision without its pointer
struct KeyframeDecisionDev {
    uint64_t frame_id;
    double time_frame, time_last_kf;
    uint32_t last_reloc_frame_id, last_keyframe_id;
    int32_t max_frames, min_frames, n_kfs, matches_inliers, n_ref_matches, keyframes_in_queue;
    int32_t flags;                     // newkf::kInertial ...
    int32_t pad_;
};

struct StereoPointsBatch {
    int n_frames;
    int decide;                        // 0: tc2li_stereo_points_batch, 1: tc2li_new_keyframe_batch
    float cx, cy, invfx, invfy;
    const StereoFrameDev* frames;
    const KeyframeDecisionDev* decisions;   // [n_frames] when decide
    const float* depth;                // [total]
    const float* xy;                   // [total][2] mvKeysUn[i].pt
    const uint8_t* held;               // [total]
    const uint8_t* outlier;            // [total] when decide
    const int32_t* ref_nobs;           // the frames' rows, when decide
    // out
    int32_t* created_keypoint;         // [total]
    float* x3D;                        // [total][3]
    int32_t* counts;                   // [n_frames][3]
    tc2li_keyframe_verdict* verdicts;  // [n_frames] when decide
};
void launch_stereo_points(const StereoPointsBatch& B, hipStream_t st);

namespace newkf {

enum Flag { kInertial = 1, kImuInitialized = 2, kOnlyTracking = 4, kMapperStopped = 8, kMapperIdle = 16, kMapperInitializing = 32,
            kCreateBlocked = 64, kHasLastKf = 128 };

// mvDepth[i] > 0 (:3138, :2682, :2482): NaN fails, +inf passes
__host__ __device__ inline bool has_depth(float z) { return z > 0.0f; }
// the close test of NeedNewKeyFrame's counts (:2990)
__host__ __device__ inline bool close_for_counts(float z, float th_depth) { return z > 0.0f && z < th_depth; }
// KeyFrame::TrackedMapPoints' test on one slot (SF/src/KeyFrame.cc:361-368) with nMinObs of Tracking.cc:2973-2975; nobs < 0: NULL or bad
__host__ __device__ inline bool ref_match(int nobs, int n_kfs) { return nobs >= (n_kfs <= 2 ? 2 : 3); }

// Tracking::NeedNewKeyFrame (:2942-3076) once the two close counts and nRefMatches are known.  Fills need, interrupt_ba, conditions,
// exit_rule.
__host__ __device__ inline void decide(const KeyframeDecisionDev& d, int n_tracked_close, int n_non_tracked_close, int n_ref_matches,
                                       tc2li_keyframe_verdict* v) {
    const bool inertial = d.flags & kInertial, idle = d.flags & kMapperIdle;
    v->need = 0; v->interrupt_ba = 0; v->conditions = 0;
    if (inertial && !(d.flags & kImuInitialized)) {                                  // :2944-2950
        v->exit_rule = TC2LI_NEWKF_EXIT_IMU_NOT_INITIALIZED;
        v->need = d.time_frame - d.time_last_kf >= 0.25;
        return;
    }
    if (d.flags & kOnlyTracking) { v->exit_rule = TC2LI_NEWKF_EXIT_ONLY_TRACKING; return; }      // :2952
    if (d.flags & kMapperStopped) { v->exit_rule = TC2LI_NEWKF_EXIT_MAPPER_STOPPED; return; }    // :2956
    // unsigned int + int is an unsigned 32-bit sum, widened for the comparison with the unsigned long mnId (Tracking.h:335-336)
    if (d.frame_id < (uint64_t)(uint32_t)(d.last_reloc_frame_id + (uint32_t)d.max_frames) && d.n_kfs > d.max_frames) {   // :2967
        v->exit_rule = TC2LI_NEWKF_EXIT_AFTER_RELOC;
        return;
    }
    const bool close = n_tracked_close < 100 && n_non_tracked_close > 70;            // :3003
    const float th_ref_ratio = d.n_kfs < 2 ? 0.4f : 0.75f;                           // :3006-3008
    const int inl = d.matches_inliers, ref = n_ref_matches;
    const bool c1a = d.frame_id >= (uint64_t)(uint32_t)(d.last_keyframe_id + (uint32_t)d.max_frames);            // :3023
    const bool c1b = d.frame_id >= (uint64_t)(uint32_t)(d.last_keyframe_id + (uint32_t)d.min_frames) && idle;    // :3025
    const bool c1c = !inertial && ((double)inl < (double)ref * 0.25 || close);       // :3027
    const bool c2 = ((float)inl < (float)ref * th_ref_ratio || close) && inl > 15;   // :3029
    const bool c3 = (d.flags & kHasLastKf) && inertial && d.time_frame - d.time_last_kf >= 0.5;   // :3033-3041
    v->conditions = (c1a ? TC2LI_NEWKF_C1A : 0) | (c1b ? TC2LI_NEWKF_C1B : 0) | (c1c ? TC2LI_NEWKF_C1C : 0) | (c2 ? TC2LI_NEWKF_C2 : 0) |
                    (c3 ? TC2LI_NEWKF_C3 : 0);
    if (!(((c1a || c1b || c1c) && c2) || c3)) { v->exit_rule = TC2LI_NEWKF_EXIT_CONDITIONS; return; }   // :3049, c4 is false (:3044)
    if (idle || (d.flags & kMapperInitializing)) {                                   // :3053
        v->exit_rule = TC2LI_NEWKF_EXIT_MAPPER_ACCEPTS;
        v->need = 1;
        return;
    }
    v->exit_rule = TC2LI_NEWKF_EXIT_MAPPER_BUSY;                                     // :3059-3065
    v->interrupt_ba = 1;
    v->need = d.keyframes_in_queue < 3;
}

// Frame::UnprojectStereo (SF/src/Frame.cc:1037-1050).  The library is built with -ffp-contract=off: every product and sum below is
// rounded on its own, on the host and on the device.  The order of the three-term sums defines parity (include/tc2li_hip.h).
__host__ __device__ inline void unproject(float u, float v, float z, float cx, float cy, float invfx, float invfy, const float* R, const float* Ow,
                                          float* x3D) {
    const float x = ((u - cx) * z) * invfx;
    const float y = ((v - cy) * z) * invfy;
    for (int r = 0; r < 3; ++r) x3D[r] = ((R[3 * r] * x + R[3 * r + 1] * y) + R[3 * r + 2] * z) + Ow[r];
}

}  // namespace newkf
}  // namespace tc2li

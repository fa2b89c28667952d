// Device side of tc2li_apply_scaled_rotation_batch / tc2li_gba_map_correction_batch (include/tc2li_hip.h "IMU initialisation: the map
// update"): map_update_host.cpp validates and concatenates the problems, map_update_kernels.hip runs them.  The per-keyframe and per-point
// arithmetic that the kernels and the host entries share are the inline functions at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"
#include "se3f_math.hpp"

namespace tc2li {

constexpr int kMapUpdateMaxKeyframes = 4096;   // the walk keeps one state byte per keyframe in LDS
constexpr int kMapUpdateKfTile = 64;           // keyframes per workgroup of the keyframe kernel
constexpr int kMapUpdatePointTile = 256;       // points per workgroup of the point kernels
constexpr int kMapUpdateWalkThreads = 256;

// A tile is a run of rows of ONE problem: a workgroup reads its problem through blockIdx, so everything of the problem that addresses
// memory is the same in all lanes.
struct MapTile { int32_t problem, first; };

// One problem = one Map::ApplyScaledRotation call.  The tables of all problems are concatenated; indices stay problem-local.
struct RotProblemDev {
    int32_t kf_off, n_kf;
    int32_t point_off, n_points;
    int32_t obs_row_off, obs_off;      // obs_offsets rows (point_off + problem index); obs_kf
    int32_t flags;                     // bit 0 scaled_vel, 1 has_tcb
    float s, last_level_scale;
    float T7[7], tcb[3];
};

struct RotBatch {
    int n_kf_tiles, n_point_tiles;
    const RotProblemDev* problems;
    const MapTile* kf_tiles;
    const MapTile* point_tiles;
    const float* kf_pose7;
    const float* kf_vel;
    const float* point_pos;
    const uint8_t* point_bad;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* point_ref_kf;
    const float* point_ref_level_scale;
    // out
    float* kf_pose7_out;
    float* kf_inv_pose7_out;
    float* kf_imu_pos_out;
    float* kf_vel_out;
    float* point_pos_out;
    float* point_normal;               // rows of bad points and of points without observations are not written
    float* point_min_distance;
    float* point_max_distance;
};
void launch_apply_scaled_rotation(const RotBatch& B, hipStream_t st);

// One problem = one map update after a global BA.
struct GbaProblemDev {
    int32_t kf_off, n_kf;
    int32_t point_off, n_points;
};

struct GbaBatch {
    int n_problems, n_point_tiles;
    const GbaProblemDev* problems;
    const MapTile* point_tiles;
    const int32_t* kf_parent;
    const uint8_t* kf_origin;
    const uint8_t* kf_bad;
    const uint8_t* kf_in_gba;
    const uint8_t* kf_imu;
    const uint8_t* kf_vel_set;
    const float* kf_pose7;
    const float* kf_gba_pose7;
    const float* kf_bef_gba_pose7;
    const float* kf_vel;
    const float* kf_gba_vel;
    const float* kf_bias;
    const float* kf_gba_bias;
    const uint8_t* point_bad;
    const uint8_t* point_in_gba;
    const float* point_pos;
    const float* point_gba_pos;
    const int32_t* point_ref_kf;
    // out
    uint8_t* kf_visited;
    uint8_t* kf_in_gba_out;
    float* kf_pose7_out;
    float* kf_bef_gba_pose7_out;
    float* kf_vel_out;
    float* kf_bias_out;
    float* point_pos_out;
    uint8_t* point_moved;
};
void launch_gba_map_correction(const GbaBatch& B, hipStream_t st);

namespace mapupd {

template <int N>
__host__ __device__ inline void copy_n(float* dst, const float* src) {
    for (int k = 0; k < N; ++k) dst[k] = src[k];
}

// ---- Map::ApplyScaledRotation ---------------------------------------------------------------------------------------------------------
// One keyframe (SF/src/Map.cc:268-277, KeyFrame::SetPose SF/src/KeyFrame.cc:121-134).  imu_pos_out may be NULL.
__host__ __device__ inline void rotate_keyframe(const se3f::Pose& Tyw, const se3f::Mat3& Ryw, float s, bool scaled_vel, bool has_tcb, const float* tcb,
                                                const float* pose7, const float* vel, float* pose7_out, float* inv7_out, float* imu_pos_out,
                                                float* vel_out) {
    se3f::Pose Twc = se3f::inverse(se3f::from7(pose7));                              // GetPoseInverse: mTwc = mTcw.inverse()
    for (int k = 0; k < 3; ++k) Twc.t.v[k] = Twc.t.v[k] * s;                         // :270
    const se3f::Pose Tyc = se3f::compose(Tyw, Twc);                                  // :271
    const se3f::Pose Tcy = se3f::inverse(Tyc);                                       // :272
    const se3f::Pose Twc2 = se3f::inverse(Tcy);                                      // KeyFrame.cc:127
    se3f::to7(Tcy, pose7_out);
    se3f::to7(Twc2, inv7_out);
    if (has_tcb && imu_pos_out) {                                                    // KeyFrame.cc:130-133
        const se3f::Mat3 Rwc = se3f::rotation_of(Twc2.q);
        for (int r = 0; r < 3; ++r) imu_pos_out[r] = se3f::row_dot(Rwc, r, tcb) + Twc2.t.v[r];
    }
    for (int r = 0; r < 3; ++r) {                                                    // :274-277
        const float v = se3f::row_dot(Ryw, r, vel);
        vel_out[r] = scaled_vel ? v * s : v;
    }
}

// s * Ryw, every entry rounded (:283)
__host__ __device__ inline se3f::Mat3 scaled(const se3f::Mat3& R, float s) {
    se3f::Mat3 M;
    for (int k = 0; k < 9; ++k) M.m[k] = s * R.m[k];
    return M;
}
__host__ __device__ inline void rotate_point(const se3f::Mat3& M, const float* tyw, const float* pos, float* pos_out) {
    for (int r = 0; r < 3; ++r) pos_out[r] = se3f::row_dot(M, r, pos) + tyw[r];
}
// MapPoint::UpdateNormalAndDepth (SF/src/MapPoint.cc:444-503) of a point that is not bad and has n > 0 observations: obs_kf its
// observing keyframes in the iteration order of mObservations, ref_kf mpRefKF, inv7 the problem's mTwc table (the camera centre is its
// translation).  The arithmetic of k_map_points_refresh.
__host__ __device__ inline void normal_and_depth(const float* pos, const int32_t* obs_kf, int n, int ref_kf, const float* inv7, float level_scale,
                                                 float last_level_scale, float* normal, float* min_distance, float* max_distance) {
    float nx = 0, ny = 0, nz = 0;
    for (int k = 0; k < n; ++k) {
        const float* c = inv7 + 7 * (size_t)obs_kf[k] + 4;
        const float vx = pos[0] - c[0], vy = pos[1] - c[1], vz = pos[2] - c[2];
        const float nr = se3f::norm3(vx, vy, vz);
        nx = nx + vx / nr; ny = ny + vy / nr; nz = nz + vz / nr;
    }
    const float* rc = inv7 + 7 * (size_t)ref_kf + 4;
    const float dist = se3f::norm3(pos[0] - rc[0], pos[1] - rc[1], pos[2] - rc[2]);
    const float mx = dist * level_scale;
    *max_distance = mx;
    *min_distance = mx / last_level_scale;
    normal[0] = nx / (float)n; normal[1] = ny / (float)n; normal[2] = nz / (float)n;
}

// ---- the map update after a global BA (SF/src/LocalMapping.cc:1346-1425) ----------------------------------------------------------------
// The tables of one problem, inputs and outputs, as both sides address them.
struct GbaTables {
    const int32_t* parent;
    const uint8_t *origin, *bad, *in_gba, *imu, *vel_set;
    const float *pose7, *gba_pose7, *bef7, *vel, *gba_vel, *bias, *gba_bias;
    uint8_t *visited, *in_gba_out;
    float *pose7_out, *bef7_out, *vel_out, *bias_out;
};
// Keyframe k is popped from the list (:1349-1392) with what its parent's visit left on it (:1359-1377).  An origin (is_child == false)
// and a child that is already in the GBA keep their stored mTcwGBA / mVwbGBA / mBiasGBA.  Reads pose7_out of the parent (its mTcwGBA),
// which the parent's own visit wrote.
__host__ __device__ inline void visit_keyframe(const GbaTables& t, int k, bool is_child) {
    const float* Tcw7 = t.pose7 + 7 * (size_t)k;
    float gba7[7], gba_vel[3], gba_bias[6];
    uint8_t flag = t.in_gba[k];
    if (is_child && !flag) {
        const int p = t.parent[k];
        const se3f::Pose Tcw = se3f::from7(Tcw7);
        const se3f::Pose Twc_parent = se3f::inverse(se3f::from7(t.pose7 + 7 * (size_t)p));    // the parent's mTwc when it is popped
        const se3f::Pose Tchildc = se3f::compose(Tcw, Twc_parent);                            // :1361
        const se3f::Pose gba = se3f::compose(Tchildc, se3f::from7(t.pose7_out + 7 * (size_t)p));   // :1362
        se3f::to7(gba, gba7);
        if (t.vel_set[k]) {                                                                   // :1364-1367
            const se3f::Quat Rcor = se3f::compose_q(se3f::inverse_q(gba.q), Tcw.q);
            const se3f::Vec3 v = se3f::spin(Rcor, se3f::Vec3{{t.vel[3 * (size_t)k], t.vel[3 * (size_t)k + 1], t.vel[3 * (size_t)k + 2]}});
            copy_n<3>(gba_vel, v.v);
        } else {
            copy_n<3>(gba_vel, t.gba_vel + 3 * (size_t)k);
        }
        copy_n<6>(gba_bias, t.bias + 6 * (size_t)k);                                          // :1372
        flag = 1;                                                                             // :1373
    } else {
        copy_n<7>(gba7, t.gba_pose7 + 7 * (size_t)k);
        copy_n<3>(gba_vel, t.gba_vel + 3 * (size_t)k);
        copy_n<6>(gba_bias, t.gba_bias + 6 * (size_t)k);
    }
    t.visited[k] = 1;
    t.in_gba_out[k] = flag;
    copy_n<7>(t.bef7_out + 7 * (size_t)k, Tcw7);                                              // :1379
    copy_n<7>(t.pose7_out + 7 * (size_t)k, gba7);                                             // :1380
    const bool imu = t.imu[k];                                                                // :1382-1388
    copy_n<3>(t.vel_out + 3 * (size_t)k, imu ? gba_vel : t.vel + 3 * (size_t)k);
    copy_n<6>(t.bias_out + 6 * (size_t)k, imu ? gba_bias : t.bias + 6 * (size_t)k);
}
// a keyframe the walk does not reach keeps everything
__host__ __device__ inline void keep_keyframe(const GbaTables& t, int k) {
    t.visited[k] = 0;
    t.in_gba_out[k] = t.in_gba[k];
    copy_n<7>(t.bef7_out + 7 * (size_t)k, t.bef7 + 7 * (size_t)k);
    copy_n<7>(t.pose7_out + 7 * (size_t)k, t.pose7 + 7 * (size_t)k);
    copy_n<3>(t.vel_out + 3 * (size_t)k, t.vel + 3 * (size_t)k);
    copy_n<6>(t.bias_out + 6 * (size_t)k, t.bias + 6 * (size_t)k);
}
// One point (:1399-1425) after the walk -> point_moved
__host__ __device__ inline uint8_t correct_point(bool bad, bool in_gba, const float* pos, const float* gba_pos, int ref_kf, const uint8_t* kf_in_gba_out,
                                                 const float* kf_bef7_out, const float* kf_pose7_out, float* pos_out) {
    if (bad) { copy_n<3>(pos_out, pos); return 0; }                                           // :1403
    if (in_gba) { copy_n<3>(pos_out, gba_pos); return 1; }                                    // :1406-1410
    if (!kf_in_gba_out[ref_kf]) { copy_n<3>(pos_out, pos); return 0; }                        // :1416
    const se3f::Vec3 Xc = se3f::act(se3f::from7(kf_bef7_out + 7 * (size_t)ref_kf), se3f::Vec3{{pos[0], pos[1], pos[2]}});    // :1420
    const se3f::Pose Twc = se3f::inverse(se3f::from7(kf_pose7_out + 7 * (size_t)ref_kf));     // GetPoseInverse after SetPose
    const se3f::Vec3 X = se3f::act(Twc, Xc);                                                  // :1423
    copy_n<3>(pos_out, X.v);
    return 2;
}

}  // namespace mapupd
}  // namespace tc2li

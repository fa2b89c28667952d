// The map update of IMU initialisation on gfx950: Map::ApplyScaledRotation (SF/src/Map.cc:256-287) and the correction of the map after a
// global BA (SF/src/LocalMapping.cc:1346-1425).  Float pose algebra (se3f_math.hpp) and streaming: no f64, no MFMA, no atomics.
//   k_rot_keyframes  one lane per keyframe, a workgroup of 64 per tile of one problem: the SE3 chain of :268-277 and KeyFrame::SetPose.
//                    Algorithmic bytes per keyframe: 40 in (pose, velocity), 92 out (pose, inverse, IMU position, velocity).
//   k_rot_points     one lane per point, 256 per tile: the transform of :283, then MapPoint::UpdateNormalAndDepth over the point's
//                    observation row, sequentially in the lane, against the camera centres k_rot_keyframes has just written.  Bytes per
//                    point: 12 + 1 + 8 + 4 + 4 in, 4 + 12 per observation (keyframe, centre: a gather into a table that stays in the
//                    caches), 12 + 12 + 8 out.
//   k_gba_walk       one workgroup per problem walks the spanning tree down from the origins in rounds: a state byte per keyframe in LDS
//                    (hence at most 4096 keyframes), lanes stride over the keyframes, a round resolves every keyframe whose parent was
//                    resolved in an earlier round, a barrier ends it, and the loop ends with a round that resolves nothing.  A chain of
//                    depth d takes d rounds.  What a round reads of a parent (its pose7_out row) was written before a barrier.
//   k_gba_points     one lane per point, 256 per tile, after the walk on the same stream.
// A workgroup's problem comes from its tile through blockIdx: the problem's offsets are scalars and the table bases scalar arithmetic.
#include "launch.hpp"
#pragma clang fp contract(off)
#include "map_update_device.hpp"

namespace tc2li {

__global__ __launch_bounds__(kMapUpdateKfTile) void k_rot_keyframes(RotBatch B) {
    const MapTile tile = B.kf_tiles[blockIdx.x];
    const RotProblemDev& P = B.problems[tile.problem];
    const int k = tile.first + (int)threadIdx.x;
    if (k >= P.n_kf) return;
    const size_t g = (size_t)P.kf_off + k;
    const se3f::Pose Tyw = se3f::from7(P.T7);
    const se3f::Mat3 Ryw = se3f::rotation_of(Tyw.q);
    float pose7[7], vel[3];
    mapupd::copy_n<7>(pose7, B.kf_pose7 + 7 * g);
    mapupd::copy_n<3>(vel, B.kf_vel + 3 * g);
    mapupd::rotate_keyframe(Tyw, Ryw, P.s, P.flags & 1, P.flags & 2, P.tcb, pose7, vel, B.kf_pose7_out + 7 * g, B.kf_inv_pose7_out + 7 * g,
                            B.kf_imu_pos_out + 3 * g, B.kf_vel_out + 3 * g);
}

__global__ __launch_bounds__(kMapUpdatePointTile) void k_rot_points(RotBatch B) {
    const MapTile tile = B.point_tiles[blockIdx.x];
    const RotProblemDev& P = B.problems[tile.problem];
    const int p = tile.first + (int)threadIdx.x;
    if (p >= P.n_points) return;
    const size_t g = (size_t)P.point_off + p;
    const se3f::Mat3 M = mapupd::scaled(se3f::rotation_of(se3f::Quat{P.T7[0], P.T7[1], P.T7[2], P.T7[3]}), P.s);
    float pos[3], out[3];
    mapupd::copy_n<3>(pos, B.point_pos + 3 * g);
    mapupd::rotate_point(M, P.T7 + 4, pos, out);                                     // SetWorldPos does not look at the bad flag
    mapupd::copy_n<3>(B.point_pos_out + 3 * g, out);
    const int32_t* row = B.obs_offsets + P.obs_row_off;
    const int o0 = row[p], n = row[p + 1] - o0;
    if (B.point_bad[g] || n <= 0) return;                                            // MapPoint.cc:450, :458
    float normal[3], mn, mx;
    mapupd::normal_and_depth(out, B.obs_kf + P.obs_off + o0, n, B.point_ref_kf[g], B.kf_inv_pose7_out + 7 * (size_t)P.kf_off,
                             B.point_ref_level_scale[g], P.last_level_scale, normal, &mn, &mx);
    mapupd::copy_n<3>(B.point_normal + 3 * g, normal);
    B.point_min_distance[g] = mn;
    B.point_max_distance[g] = mx;
}

void launch_apply_scaled_rotation(const RotBatch& B, hipStream_t st) {
    if (B.n_kf_tiles > 0) TC2LI_LAUNCH(k_rot_keyframes, dim3(B.n_kf_tiles), dim3(kMapUpdateKfTile), 0, st, B);
    if (B.n_point_tiles > 0) TC2LI_LAUNCH(k_rot_points, dim3(B.n_point_tiles), dim3(kMapUpdatePointTile), 0, st, B);
}

// the states of a keyframe in the walk
enum : uint8_t { kWaiting = 0, kResolved = 1, kPending = 2, kNever = 3 };

__global__ __launch_bounds__(kMapUpdateWalkThreads) void k_gba_walk(GbaBatch B) {
    __shared__ uint8_t state[kMapUpdateMaxKeyframes];
    const GbaProblemDev& P = B.problems[blockIdx.x];
    const int n = P.n_kf, tid = threadIdx.x;
    const size_t o = (size_t)P.kf_off;
    mapupd::GbaTables t;
    t.parent = B.kf_parent + o; t.origin = B.kf_origin + o; t.bad = B.kf_bad + o; t.in_gba = B.kf_in_gba + o; t.imu = B.kf_imu + o;
    t.vel_set = B.kf_vel_set + o;
    t.pose7 = B.kf_pose7 + 7 * o; t.gba_pose7 = B.kf_gba_pose7 + 7 * o; t.bef7 = B.kf_bef_gba_pose7 + 7 * o;
    t.vel = B.kf_vel + 3 * o; t.gba_vel = B.kf_gba_vel + 3 * o; t.bias = B.kf_bias + 6 * o; t.gba_bias = B.kf_gba_bias + 6 * o;
    t.visited = B.kf_visited + o; t.in_gba_out = B.kf_in_gba_out + o;
    t.pose7_out = B.kf_pose7_out + 7 * o; t.bef7_out = B.kf_bef_gba_pose7_out + 7 * o; t.vel_out = B.kf_vel_out + 3 * o; t.bias_out = B.kf_bias_out + 6 * o;
    // the origins are on the list from the start and are not asked whether they are bad (:1347)
    for (int k = tid; k < n; k += kMapUpdateWalkThreads) {
        uint8_t s;
        if (t.origin[k]) { mapupd::visit_keyframe(t, k, false); s = kResolved; }
        else s = (t.bad[k] || t.parent[k] < 0) ? kNever : kWaiting;                  // :1356: a bad child is not pushed, nor anything below it
        state[k] = s;
    }
    for (;;) {
        __syncthreads();   // the rows and states of the round before are written
        int any = 0;
        for (int k = tid; k < n; k += kMapUpdateWalkThreads) {
            if (state[k] != kWaiting || state[t.parent[k]] != kResolved) continue;   // a parent pending in this round counts in the next
            mapupd::visit_keyframe(t, k, true);
            state[k] = kPending;
            any = 1;
        }
        if (!__syncthreads_or(any)) break;
        for (int k = tid; k < n; k += kMapUpdateWalkThreads)                         // the lane's own keyframes
            if (state[k] == kPending) state[k] = kResolved;
    }
    for (int k = tid; k < n; k += kMapUpdateWalkThreads)
        if (state[k] != kResolved) mapupd::keep_keyframe(t, k);
}

__global__ __launch_bounds__(kMapUpdatePointTile) void k_gba_points(GbaBatch B) {
    const MapTile tile = B.point_tiles[blockIdx.x];
    const GbaProblemDev& P = B.problems[tile.problem];
    const int p = tile.first + (int)threadIdx.x;
    if (p >= P.n_points) return;
    const size_t g = (size_t)P.point_off + p, o = (size_t)P.kf_off;
    float pos[3], gba_pos[3], out[3];
    mapupd::copy_n<3>(pos, B.point_pos + 3 * g);
    mapupd::copy_n<3>(gba_pos, B.point_gba_pos + 3 * g);
    const uint8_t moved = mapupd::correct_point(B.point_bad[g], B.point_in_gba[g], pos, gba_pos, B.point_ref_kf[g], B.kf_in_gba_out + o,
                                                B.kf_bef_gba_pose7_out + 7 * o, B.kf_pose7_out + 7 * o, out);
    mapupd::copy_n<3>(B.point_pos_out + 3 * g, out);
    B.point_moved[g] = moved;
}

void launch_gba_map_correction(const GbaBatch& B, hipStream_t st) {
    if (B.n_problems > 0) TC2LI_LAUNCH(k_gba_walk, dim3(B.n_problems), dim3(kMapUpdateWalkThreads), 0, st, B);
    if (B.n_point_tiles > 0) TC2LI_LAUNCH(k_gba_points, dim3(B.n_point_tiles), dim3(kMapUpdatePointTile), 0, st, B);
}

}  // namespace tc2li

// tc2li_apply_scaled_rotation_batch / tc2li_host_apply_scaled_rotation_batch / tc2li_gba_map_correction_batch /
// tc2li_host_gba_map_correction_batch / tc2li_map_update_limits (include/tc2li_hip.h "IMU initialisation: the map update"):
// Map::ApplyScaledRotation (SF/src/Map.cc:256-287) with KeyFrame::SetPose (SF/src/KeyFrame.cc:121-134) and MapPoint::UpdateNormalAndDepth
// (SF/src/MapPoint.cc:444-503), and the map update that follows a global BA (SF/src/LocalMapping.cc:1346-1425), on flat copies of the map.
// This file validates the problems and either runs them in plain C++ or concatenates them for map_update_kernels.hip.
#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "map_update_device.hpp"
#include "packed_batch.hpp"

namespace tc2li {
namespace {

// ---- Map::ApplyScaledRotation ---------------------------------------------------------------------------------------------------------
const char* validate(const tc2li_scaled_rotation_problem& in) {
    if (in.n_keyframes < 0 || in.n_points < 0) return "negative size";
    if (!in.obs_offsets) return "null obs_offsets";
    if (in.n_keyframes && (!in.kf_pose7 || !in.kf_vel || !in.kf_pose7_out || !in.kf_inv_pose7_out || !in.kf_vel_out)) return "null keyframe table or output";
    if (in.n_points && (!in.point_pos || !in.point_bad || !in.point_ref_kf || !in.point_ref_level_scale || !in.point_pos_out || !in.point_normal ||
                        !in.point_min_distance || !in.point_max_distance))
        return "null point table or output";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_obs = in.obs_offsets[in.n_points];
    if (n_obs && !in.obs_kf) return "null obs_kf";
    for (int i = 0; i < n_obs; ++i)
        if (in.obs_kf[i] < 0 || in.obs_kf[i] >= in.n_keyframes) return "obs_kf out of range";
    for (int p = 0; p < in.n_points; ++p) {
        const int r = in.point_ref_kf[p];
        const bool unused = in.point_bad[p] || in.obs_offsets[p + 1] == in.obs_offsets[p];
        if (r < -1 || r >= in.n_keyframes || (r < 0 && !unused)) return "point_ref_kf out of range";
    }
    return "";
}

int validate_all(const char* entry, const tc2li_scaled_rotation_problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "problem", n_problems, invalid_if([&](int p) { return validate(problems[p]); }));
}

void rotate_one(const tc2li_scaled_rotation_problem& in) {
    const se3f::Pose Tyw = se3f::from7(in.T7);
    const se3f::Mat3 Ryw = se3f::rotation_of(Tyw.q);
    for (int k = 0; k < in.n_keyframes; ++k)
        mapupd::rotate_keyframe(Tyw, Ryw, in.s, in.scaled_vel, in.has_tcb, in.tcb3, in.kf_pose7 + 7 * (size_t)k, in.kf_vel + 3 * (size_t)k,
                                in.kf_pose7_out + 7 * (size_t)k, in.kf_inv_pose7_out + 7 * (size_t)k,
                                in.kf_imu_pos_out ? in.kf_imu_pos_out + 3 * (size_t)k : nullptr, in.kf_vel_out + 3 * (size_t)k);
    const se3f::Mat3 M = mapupd::scaled(Ryw, in.s);
    for (int p = 0; p < in.n_points; ++p) {
        float* out = in.point_pos_out + 3 * (size_t)p;
        mapupd::rotate_point(M, in.T7 + 4, in.point_pos + 3 * (size_t)p, out);
        const int o0 = in.obs_offsets[p], n = in.obs_offsets[p + 1] - o0;
        if (in.point_bad[p] || n <= 0) continue;
        mapupd::normal_and_depth(out, in.obs_kf + o0, n, in.point_ref_kf[p], in.kf_inv_pose7_out, in.point_ref_level_scale[p], in.last_level_scale,
                                 in.point_normal + 3 * (size_t)p, in.point_min_distance + p, in.point_max_distance + p);
    }
}

// the tiles of all problems: ceil(rows / tile) per problem
template <class Rows>
std::vector<MapTile> tiles_of(int n_problems, int tile, Rows rows) {
    std::vector<MapTile> t;
    for (int p = 0; p < n_problems; ++p)
        for (int first = 0; first < rows(p); first += tile) t.push_back(MapTile{p, first});
    return t;
}

// ---- the map update after a global BA ---------------------------------------------------------------------------------------------------
const char* validate(const tc2li_gba_correction_problem& in, int* code) {
    *code = TC2LI_ERR_INVALID;
    if (in.n_keyframes < 0 || in.n_points < 0) return "negative size";
    if (in.n_keyframes && (!in.kf_parent || !in.kf_origin || !in.kf_bad || !in.kf_in_gba || !in.kf_imu || !in.kf_vel_set || !in.kf_pose7 || !in.kf_gba_pose7 ||
                           !in.kf_bef_gba_pose7 || !in.kf_vel || !in.kf_gba_vel || !in.kf_bias || !in.kf_gba_bias || !in.kf_visited || !in.kf_in_gba_out ||
                           !in.kf_pose7_out || !in.kf_bef_gba_pose7_out || !in.kf_vel_out || !in.kf_bias_out))
        return "null keyframe table or output";
    if (in.n_points && (!in.point_bad || !in.point_in_gba || !in.point_pos || !in.point_gba_pos || !in.point_ref_kf || !in.point_pos_out || !in.point_moved))
        return "null point table or output";
    const int n = in.n_keyframes;
    for (int k = 0; k < n; ++k) {
        if (in.kf_parent[k] < -1 || in.kf_parent[k] >= n) return "kf_parent out of range";
        if (in.kf_origin[k] && in.kf_parent[k] >= 0) return "kf_origin with a parent";
    }
    // every parent chain ends: 1 = on the chain being followed, 2 = known to end
    std::vector<uint8_t> mark(n, 0);
    for (int k = 0; k < n; ++k) {
        int c = k;
        while (c >= 0 && !mark[c]) { mark[c] = 1; c = in.kf_parent[c]; }
        if (c >= 0 && mark[c] == 1) return "kf_parent chain does not end (a cycle)";
        for (c = k; c >= 0 && mark[c] == 1; c = in.kf_parent[c]) mark[c] = 2;
    }
    for (int p = 0; p < in.n_points; ++p) {
        const int r = in.point_ref_kf[p];
        if (r < -1 || r >= n || (r < 0 && !in.point_bad[p] && !in.point_in_gba[p])) return "point_ref_kf out of range";
    }
    if (n > kMapUpdateMaxKeyframes) { *code = TC2LI_ERR_CAPACITY; return "more than 4096 keyframes"; }
    return "";
}

int validate_all(const char* entry, const tc2li_gba_correction_problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "problem", n_problems, [&](int p, const char** what) {
        int code;
        *what = validate(problems[p], &code);
        return (*what)[0] ? code : 0;
    });
}

mapupd::GbaTables tables_of(const tc2li_gba_correction_problem& in) {
    mapupd::GbaTables t;
    t.parent = in.kf_parent; t.origin = in.kf_origin; t.bad = in.kf_bad; t.in_gba = in.kf_in_gba; t.imu = in.kf_imu; t.vel_set = in.kf_vel_set;
    t.pose7 = in.kf_pose7; t.gba_pose7 = in.kf_gba_pose7; t.bef7 = in.kf_bef_gba_pose7; t.vel = in.kf_vel; t.gba_vel = in.kf_gba_vel;
    t.bias = in.kf_bias; t.gba_bias = in.kf_gba_bias;
    t.visited = in.kf_visited; t.in_gba_out = in.kf_in_gba_out; t.pose7_out = in.kf_pose7_out; t.bef7_out = in.kf_bef_gba_pose7_out;
    t.vel_out = in.kf_vel_out; t.bias_out = in.kf_bias_out;
    return t;
}

void correct_one(const tc2li_gba_correction_problem& in) {
    const int n = in.n_keyframes;
    const mapupd::GbaTables t = tables_of(in);
    // the children of every keyframe, as rows
    std::vector<int32_t> first(n + 1, 0), child(n), list;
    for (int k = 0; k < n; ++k)
        if (in.kf_parent[k] >= 0) ++first[in.kf_parent[k] + 1];
    for (int k = 0; k < n; ++k) first[k + 1] += first[k];
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int k = 0; k < n; ++k)
        if (in.kf_parent[k] >= 0) child[fill[in.kf_parent[k]]++] = k;
    std::vector<uint8_t> reached(n, 0);
    list.reserve(n);
    for (int k = 0; k < n; ++k)
        if (in.kf_origin[k]) { mapupd::visit_keyframe(t, k, false); reached[k] = 1; list.push_back(k); }
    for (size_t head = 0; head < list.size(); ++head) {                              // lpKFtoCheck
        const int kf = list[head];
        for (int c = first[kf]; c < first[kf + 1]; ++c) {
            const int k = child[c];
            if (in.kf_bad[k]) continue;                                              // :1356
            mapupd::visit_keyframe(t, k, true);
            reached[k] = 1;
            list.push_back(k);
        }
    }
    for (int k = 0; k < n; ++k)
        if (!reached[k]) mapupd::keep_keyframe(t, k);
    for (int p = 0; p < in.n_points; ++p)
        in.point_moved[p] = mapupd::correct_point(in.point_bad[p], in.point_in_gba[p], in.point_pos + 3 * (size_t)p, in.point_gba_pos + 3 * (size_t)p,
                                                  in.point_ref_kf[p], in.kf_in_gba_out, in.kf_bef_gba_pose7_out, in.kf_pose7_out,
                                                  in.point_pos_out + 3 * (size_t)p);
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_map_update_limits(int32_t* out, int capacity) {
    if (!out || capacity < 4) {
        set_error("tc2li_map_update_limits: room for 4 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kMapUpdateMaxKeyframes; out[1] = kMapUpdateWalkThreads; out[2] = kMapUpdateKfTile; out[3] = kMapUpdatePointTile;
    return 4;
}

extern "C" int tc2li_host_apply_scaled_rotation_batch(const tc2li_scaled_rotation_problem* problems, int n_problems) {
    const int rc = validate_all("tc2li_host_apply_scaled_rotation_batch", problems, n_problems);
    if (rc < 0) return rc;
    tracking_pool().parallel_for(n_problems, [&](int p) { rotate_one(problems[p]); });
    return n_problems;
}

extern "C" int tc2li_apply_scaled_rotation_batch(const tc2li_scaled_rotation_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_apply_scaled_rotation_batch";
    const int rc = validate_all(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    std::vector<RotProblemDev> dev(n_problems);
    size_t n_kf = 0, n_points = 0, n_obs = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_scaled_rotation_problem& in = problems[p];
        RotProblemDev& d = dev[p];
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.point_off = (int32_t)n_points; d.n_points = in.n_points;
        d.obs_row_off = (int32_t)(n_points + p); d.obs_off = (int32_t)n_obs;
        d.flags = (in.scaled_vel ? 1 : 0) | (in.has_tcb ? 2 : 0);
        d.s = in.s; d.last_level_scale = in.last_level_scale;
        memcpy(d.T7, in.T7, sizeof d.T7); memcpy(d.tcb, in.tcb3, sizeof d.tcb);
        n_kf += in.n_keyframes; n_points += in.n_points; n_obs += in.obs_offsets[in.n_points];
        if (std::max(std::max(7 * n_kf, 3 * n_points + p), n_obs) > kMaxRows) return too_many_rows(entry, p);
    }
    const std::vector<MapTile> kf_tiles = tiles_of(n_problems, kMapUpdateKfTile, [&](int p) { return problems[p].n_keyframes; });
    const std::vector<MapTile> point_tiles = tiles_of(n_problems, kMapUpdatePointTile, [&](int p) { return problems[p].n_points; });
    const size_t np = (size_t)n_problems;
    PackedTransfer T;
    Packer& io = T.io;
    const auto o_prob = io.take<RotProblemDev>(np);
    const auto o_kt = io.take<MapTile>(kf_tiles.size()), o_pt = io.take<MapTile>(point_tiles.size());
    const auto o_pose = io.take<float>(7 * n_kf), o_vel = io.take<float>(3 * n_kf), o_pos = io.take<float>(3 * n_points);
    const auto o_bad = io.take<uint8_t>(n_points);
    const auto o_row = io.take<int32_t>(n_points + np), o_okf = io.take<int32_t>(n_obs), o_ref = io.take<int32_t>(n_points);
    const auto o_scale = io.take<float>(n_points);
    T.outputs_begin();
    const auto o_pose_out = io.take<float>(7 * n_kf), o_inv_out = io.take<float>(7 * n_kf), o_imu_out = io.take<float>(3 * n_kf),
               o_vel_out = io.take<float>(3 * n_kf), o_pos_out = io.take<float>(3 * n_points), o_normal = io.take<float>(3 * n_points),
               o_min = io.take<float>(n_points), o_max = io.take<float>(n_points);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceScaledRotation>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, dev.data(), np);
    io.put(o_kt, 0, kf_tiles.data(), kf_tiles.size());
    io.put(o_pt, 0, point_tiles.data(), point_tiles.size());
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_scaled_rotation_problem& in = problems[p];
        const RotProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        io.put(o_pose, 7 * (size_t)d.kf_off, in.kf_pose7, 7 * nk); io.put(o_vel, 3 * (size_t)d.kf_off, in.kf_vel, 3 * nk);
        io.put(o_pos, 3 * (size_t)d.point_off, in.point_pos, 3 * npt); io.put(o_bad, d.point_off, in.point_bad, npt);
        io.put(o_row, d.obs_row_off, in.obs_offsets, npt + 1); io.put(o_okf, d.obs_off, in.obs_kf, (size_t)in.obs_offsets[in.n_points]);
        io.put(o_ref, d.point_off, in.point_ref_kf, npt); io.put(o_scale, d.point_off, in.point_ref_level_scale, npt);
    });
    TC2LI_HIP_CHECK(T.upload(st));
    RotBatch B{};
    B.n_kf_tiles = (int)kf_tiles.size(); B.n_point_tiles = (int)point_tiles.size();
    B.problems = T.dev(o_prob); B.kf_tiles = T.dev(o_kt); B.point_tiles = T.dev(o_pt);
    B.kf_pose7 = T.dev(o_pose); B.kf_vel = T.dev(o_vel); B.point_pos = T.dev(o_pos); B.point_bad = T.dev(o_bad);
    B.obs_offsets = T.dev(o_row); B.obs_kf = T.dev(o_okf); B.point_ref_kf = T.dev(o_ref); B.point_ref_level_scale = T.dev(o_scale);
    B.kf_pose7_out = T.dev(o_pose_out); B.kf_inv_pose7_out = T.dev(o_inv_out); B.kf_imu_pos_out = T.dev(o_imu_out); B.kf_vel_out = T.dev(o_vel_out);
    B.point_pos_out = T.dev(o_pos_out); B.point_normal = T.dev(o_normal); B.point_min_distance = T.dev(o_min); B.point_max_distance = T.dev(o_max);
    launch_apply_scaled_rotation(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_scaled_rotation_problem& in = problems[p];
        const RotProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        io.get(in.kf_pose7_out, o_pose_out, 7 * (size_t)d.kf_off, 7 * nk); io.get(in.kf_inv_pose7_out, o_inv_out, 7 * (size_t)d.kf_off, 7 * nk);
        if (in.has_tcb && in.kf_imu_pos_out) io.get(in.kf_imu_pos_out, o_imu_out, 3 * (size_t)d.kf_off, 3 * nk);
        io.get(in.kf_vel_out, o_vel_out, 3 * (size_t)d.kf_off, 3 * nk); io.get(in.point_pos_out, o_pos_out, 3 * (size_t)d.point_off, 3 * npt);
        // the rows UpdateNormalAndDepth wrote
        const float* normal = T.host(o_normal) + 3 * (size_t)d.point_off;
        const float *mn = T.host(o_min) + d.point_off, *mx = T.host(o_max) + d.point_off;
        for (int i = 0; i < in.n_points; ++i) {
            if (in.point_bad[i] || in.obs_offsets[i + 1] == in.obs_offsets[i]) continue;
            memcpy(in.point_normal + 3 * (size_t)i, normal + 3 * (size_t)i, 12);
            in.point_min_distance[i] = mn[i]; in.point_max_distance[i] = mx[i];
        }
    });
    return n_problems;
}

extern "C" int tc2li_host_gba_map_correction_batch(const tc2li_gba_correction_problem* problems, int n_problems) {
    const int rc = validate_all("tc2li_host_gba_map_correction_batch", problems, n_problems);
    if (rc < 0) return rc;
    tracking_pool().parallel_for(n_problems, [&](int p) { correct_one(problems[p]); });
    return n_problems;
}

extern "C" int tc2li_gba_map_correction_batch(const tc2li_gba_correction_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_gba_map_correction_batch";
    const int rc = validate_all(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    std::vector<GbaProblemDev> dev(n_problems);
    size_t n_kf = 0, n_points = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_gba_correction_problem& in = problems[p];
        dev[p] = GbaProblemDev{(int32_t)n_kf, in.n_keyframes, (int32_t)n_points, in.n_points};
        n_kf += in.n_keyframes; n_points += in.n_points;
        if (std::max(7 * n_kf, 3 * n_points) > kMaxRows) return too_many_rows(entry, p);
    }
    const std::vector<MapTile> point_tiles = tiles_of(n_problems, kMapUpdatePointTile, [&](int p) { return problems[p].n_points; });
    const size_t np = (size_t)n_problems;
    PackedTransfer T;
    Packer& io = T.io;
    const auto o_prob = io.take<GbaProblemDev>(np);
    const auto o_pt = io.take<MapTile>(point_tiles.size());
    const auto o_parent = io.take<int32_t>(n_kf);
    const auto o_origin = io.take<uint8_t>(n_kf), o_kbad = io.take<uint8_t>(n_kf), o_kin = io.take<uint8_t>(n_kf), o_imu = io.take<uint8_t>(n_kf),
               o_vset = io.take<uint8_t>(n_kf);
    const auto o_pose = io.take<float>(7 * n_kf), o_gpose = io.take<float>(7 * n_kf), o_bef = io.take<float>(7 * n_kf), o_vel = io.take<float>(3 * n_kf),
               o_gvel = io.take<float>(3 * n_kf), o_bias = io.take<float>(6 * n_kf), o_gbias = io.take<float>(6 * n_kf);
    const auto o_pbad = io.take<uint8_t>(n_points), o_pin = io.take<uint8_t>(n_points);
    const auto o_pos = io.take<float>(3 * n_points), o_gpos = io.take<float>(3 * n_points);
    const auto o_ref = io.take<int32_t>(n_points);
    T.outputs_begin();
    const auto o_visited = io.take<uint8_t>(n_kf), o_kin_out = io.take<uint8_t>(n_kf);
    const auto o_pose_out = io.take<float>(7 * n_kf), o_bef_out = io.take<float>(7 * n_kf), o_vel_out = io.take<float>(3 * n_kf),
               o_bias_out = io.take<float>(6 * n_kf), o_pos_out = io.take<float>(3 * n_points);
    const auto o_moved = io.take<uint8_t>(n_points);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceGbaCorrection>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, dev.data(), np);
    io.put(o_pt, 0, point_tiles.data(), point_tiles.size());
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_gba_correction_problem& in = problems[p];
        const size_t k0 = (size_t)dev[p].kf_off, p0 = (size_t)dev[p].point_off, nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        io.put(o_parent, k0, in.kf_parent, nk); io.put(o_origin, k0, in.kf_origin, nk); io.put(o_kbad, k0, in.kf_bad, nk);
        io.put(o_kin, k0, in.kf_in_gba, nk); io.put(o_imu, k0, in.kf_imu, nk); io.put(o_vset, k0, in.kf_vel_set, nk);
        io.put(o_pose, 7 * k0, in.kf_pose7, 7 * nk); io.put(o_gpose, 7 * k0, in.kf_gba_pose7, 7 * nk); io.put(o_bef, 7 * k0, in.kf_bef_gba_pose7, 7 * nk);
        io.put(o_vel, 3 * k0, in.kf_vel, 3 * nk); io.put(o_gvel, 3 * k0, in.kf_gba_vel, 3 * nk);
        io.put(o_bias, 6 * k0, in.kf_bias, 6 * nk); io.put(o_gbias, 6 * k0, in.kf_gba_bias, 6 * nk);
        io.put(o_pbad, p0, in.point_bad, npt); io.put(o_pin, p0, in.point_in_gba, npt);
        io.put(o_pos, 3 * p0, in.point_pos, 3 * npt); io.put(o_gpos, 3 * p0, in.point_gba_pos, 3 * npt); io.put(o_ref, p0, in.point_ref_kf, npt);
    });
    TC2LI_HIP_CHECK(T.upload(st));
    GbaBatch B{};
    B.n_problems = n_problems; B.n_point_tiles = (int)point_tiles.size();
    B.problems = T.dev(o_prob); B.point_tiles = T.dev(o_pt);
    B.kf_parent = T.dev(o_parent); B.kf_origin = T.dev(o_origin); B.kf_bad = T.dev(o_kbad); B.kf_in_gba = T.dev(o_kin); B.kf_imu = T.dev(o_imu);
    B.kf_vel_set = T.dev(o_vset);
    B.kf_pose7 = T.dev(o_pose); B.kf_gba_pose7 = T.dev(o_gpose); B.kf_bef_gba_pose7 = T.dev(o_bef); B.kf_vel = T.dev(o_vel); B.kf_gba_vel = T.dev(o_gvel);
    B.kf_bias = T.dev(o_bias); B.kf_gba_bias = T.dev(o_gbias);
    B.point_bad = T.dev(o_pbad); B.point_in_gba = T.dev(o_pin); B.point_pos = T.dev(o_pos); B.point_gba_pos = T.dev(o_gpos); B.point_ref_kf = T.dev(o_ref);
    B.kf_visited = T.dev(o_visited); B.kf_in_gba_out = T.dev(o_kin_out); B.kf_pose7_out = T.dev(o_pose_out); B.kf_bef_gba_pose7_out = T.dev(o_bef_out);
    B.kf_vel_out = T.dev(o_vel_out); B.kf_bias_out = T.dev(o_bias_out); B.point_pos_out = T.dev(o_pos_out); B.point_moved = T.dev(o_moved);
    launch_gba_map_correction(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_gba_correction_problem& in = problems[p];
        const size_t k0 = (size_t)dev[p].kf_off, p0 = (size_t)dev[p].point_off, nk = (size_t)in.n_keyframes, npt = (size_t)in.n_points;
        io.get(in.kf_visited, o_visited, k0, nk); io.get(in.kf_in_gba_out, o_kin_out, k0, nk);
        io.get(in.kf_pose7_out, o_pose_out, 7 * k0, 7 * nk); io.get(in.kf_bef_gba_pose7_out, o_bef_out, 7 * k0, 7 * nk);
        io.get(in.kf_vel_out, o_vel_out, 3 * k0, 3 * nk); io.get(in.kf_bias_out, o_bias_out, 6 * k0, 6 * nk);
        io.get(in.point_pos_out, o_pos_out, 3 * p0, 3 * npt); io.get(in.point_moved, o_moved, p0, npt);
    });
    return n_problems;
}

// tc2li_keyframe_culling_batch / tc2li_host_keyframe_culling_batch / tc2li_map_point_culling_batch / tc2li_host_map_point_culling_batch
// (include/tc2li_hip.h "local mapping: culling"): LocalMapping::KeyFrameCulling (SF/src/LocalMapping.cc:913-1065) with the side effects of
// KeyFrame::SetBadFlag (SF/src/KeyFrame.cc:585-611) and MapPoint::EraseObservation (SF/src/MapPoint.cc:177-210) on a flat copy of the
// graph, and LocalMapping::MapPointCulling (:360-399).  This file validates the problems and either walks them in plain C++ or
// concatenates them for culling_kernels.hip.
#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "culling_device.hpp"
#include "packed_batch.hpp"

namespace tc2li {
namespace {

// "" or what is wrong with problem p
const char* validate(const tc2li_culling_problem& in) {
    if (in.n_keyframes < 0 || in.n_local < 0 || in.n_points < 0) return "negative size";
    if (!in.slot_offsets || !in.obs_offsets || !in.n_visited) return "null slot_offsets, obs_offsets or n_visited";
    if (in.n_keyframes && (!in.kf_flags || !in.kf_id || !in.kf_prev || !in.kf_next || !in.kf_time || !in.kf_imu_pos || !in.kf_th_depth))
        return "null keyframe table";
    if (in.n_points && (!in.point_bad || !in.point_nobs)) return "null point table";
    if (in.n_local && (!in.local || !in.verdict || !in.n_mps || !in.n_redundant)) return "null local list or output";
    if (!ascending(in.slot_offsets, in.n_keyframes)) return "slot_offsets do not ascend from 0";
    if (!ascending(in.obs_offsets, in.n_points)) return "obs_offsets do not ascend from 0";
    const int n_slots = in.slot_offsets[in.n_keyframes], n_obs = in.obs_offsets[in.n_points];
    if (n_slots && (!in.slot_point || !in.slot_depth || !in.slot_octave)) return "null slot array";
    if (n_obs && (!in.obs_kf || !in.obs_octave || !in.obs_weight)) return "null observation array";
    for (int i = 0; i < in.n_local; ++i)
        if (in.local[i] < 0 || in.local[i] >= in.n_keyframes) return "local index out of range";
    for (int i = 0; i < in.n_keyframes; ++i)
        if (in.kf_prev[i] < -1 || in.kf_prev[i] >= in.n_keyframes || in.kf_next[i] < -1 || in.kf_next[i] >= in.n_keyframes)
            return "kf_prev / kf_next out of range";
    for (int i = 0; i < n_slots; ++i)
        if (in.slot_point[i] < -1 || in.slot_point[i] >= in.n_points) return "slot_point out of range";
    for (int i = 0; i < n_obs; ++i)
        if (in.obs_kf[i] < 0 || in.obs_kf[i] >= in.n_keyframes) return "obs_kf out of range";
    return "";
}

int validate_all(const char* entry, const tc2li_culling_problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return validate_each(entry, "problem", n_problems, invalid_if([&](int p) { return validate(problems[p]); }));
}

// nMPs and nRedundantObservations of keyframe kf on the current state (:959-1019)
void count_keyframe(const tc2li_culling_problem& in, int kf, const uint8_t* bad, const int32_t* nobs, const uint8_t* dead, int* n_mps, int* n_red) {
    const float th_depth = in.kf_th_depth[kf];
    int mps = 0, red = 0;
    for (int s = in.slot_offsets[kf]; s < in.slot_offsets[kf + 1]; ++s) {
        const int p = in.slot_point[s];
        if (p < 0 || bad[p]) continue;                                               // :966-968
        const float depth = in.slot_depth[s];
        if (depth > th_depth || depth < 0.0f) continue;                              // :972
        ++mps;
        if (nobs[p] <= cull::kThObs) continue;                                       // :977
        const int level = (int)in.slot_octave[s] + 1;
        int n = 0;
        for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o)              // :984-1011
            if (!dead[o] && in.obs_kf[o] != kf && (int)in.obs_octave[o] <= level && ++n > cull::kThObs) break;
        red += n > cull::kThObs;
    }
    *n_mps = mps; *n_red = red;
}

void cull_one(const tc2li_culling_problem& in) {
    const int n_obs = in.obs_offsets[in.n_points];
    std::vector<uint8_t> bad(in.point_bad, in.point_bad + in.n_points), dead(n_obs, 0), kf_bad(in.n_keyframes, 0);
    std::vector<int32_t> nobs(in.point_nobs, in.point_nobs + in.n_points), prev(in.kf_prev, in.kf_prev + in.n_keyframes),
        next(in.kf_next, in.kf_next + in.n_keyframes);
    int keyframes_in_map = in.keyframes_in_map, count = 0;
    while (count < in.n_local) {
        const int i = count++;                                                       // :952
        const int kf = in.local[i];
        if ((in.kf_flags[kf] & 3) || kf_bad[kf]) { in.verdict[i] = TC2LI_CULL_SKIPPED; continue; }    // :955
        int n_mps, n_red;
        count_keyframe(in, kf, bad.data(), nobs.data(), dead.data(), &n_mps, &n_red);
        int verdict = 0;
        bool go_on = false;
        if (cull::redundant(n_red, n_mps, in.inertial)) {                            // :1021
            verdict = TC2LI_CULL_REDUNDANT;
            if (in.inertial) {
                const int pv = prev[kf], nx = next[kf];
                const bool has_links = pv >= 0 && nx >= 0;
                const cull::Gate gate = cull::inertial_gate(keyframes_in_map, in.kf_id[kf], in.current_id, in.last_id, has_links,
                                                            has_links ? in.kf_time[pv] : 0.0, has_links ? in.kf_time[nx] : 0.0, in.kf_imu_pos + 3 * (size_t)kf,
                                                            in.kf_imu_pos + 3 * (size_t)(has_links ? pv : kf), in.imu_initialized, in.inertial_ba2);
                go_on = gate == cull::kGateContinue;
                if (gate == cull::kGateMerge) {                                      // :1038-1041
                    verdict |= TC2LI_CULL_MERGED | TC2LI_CULL_SET_BAD;
                    prev[nx] = pv; next[pv] = nx; next[kf] = -1; prev[kf] = -1;
                }
            } else {
                verdict |= TC2LI_CULL_SET_BAD;                                       // :1057
            }
        }
        if (verdict & TC2LI_CULL_SET_BAD) {
            if (in.kf_flags[kf] & 4) {
                verdict |= TC2LI_CULL_DEFERRED;                                      // KeyFrame.cc:593-597
            } else {
                for (int s = in.slot_offsets[kf]; s < in.slot_offsets[kf + 1]; ++s) {    // KeyFrame.cc:605-611
                    const int p = in.slot_point[s];
                    if (p < 0 || bad[p]) continue;                                   // a bad point holds no observations (MapPoint.cc:233)
                    int w = 0;
                    bool held = false;
                    for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o)
                        if (in.obs_kf[o] == kf && !dead[o]) { dead[o] = 1; w += in.obs_weight[o]; held = true; }
                    if (!held) continue;                                             // MapPoint.cc:182
                    nobs[p] -= w;                                                    // :187-192
                    if (nobs[p] <= 2) bad[p] = 1;                                    // :203-209
                }
                kf_bad[kf] = 1;
                --keyframes_in_map;                                                  // Map::EraseKeyFrame
            }
        }
        in.verdict[i] = verdict; in.n_mps[i] = n_mps; in.n_redundant[i] = n_red;
        if (go_on) continue;                                                         // :1026, :1029 jump over the closing test
        if ((count > 20 && in.abort_ba) || count > 100) break;                       // :1060
    }
    *in.n_visited = count;
    for (int i = count; i < in.n_local; ++i) in.verdict[i] = TC2LI_CULL_NOT_VISITED;
    if (in.point_bad_after && in.n_points) memcpy(in.point_bad_after, bad.data(), in.n_points);
    if (in.point_nobs_after && in.n_points) memcpy(in.point_nobs_after, nobs.data(), (size_t)in.n_points * 4);
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_host_keyframe_culling_batch(const tc2li_culling_problem* problems, int n_problems) {
    const int rc = validate_all("tc2li_host_keyframe_culling_batch", problems, n_problems);
    if (rc < 0) return rc;
    tracking_pool().parallel_for(n_problems, [&](int p) { cull_one(problems[p]); });
    return n_problems;
}

extern "C" int tc2li_keyframe_culling_batch(const tc2li_culling_problem* problems, int n_problems, void* stream) {
    const char* entry = "tc2li_keyframe_culling_batch";
    const int rc = validate_all(entry, problems, n_problems);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    // where every problem's tables start in the concatenation
    std::vector<CullProblemDev> dev(n_problems);
    size_t n_kf = 0, n_slots = 0, n_local = 0, n_points = 0, n_obs = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_culling_problem& in = problems[p];
        CullProblemDev& d = dev[p];
        d.kf_off = (int32_t)n_kf; d.n_kf = in.n_keyframes; d.slot_row_off = (int32_t)(n_kf + p); d.slot_off = (int32_t)n_slots;
        d.local_off = (int32_t)n_local; d.n_local = in.n_local;
        d.point_off = (int32_t)n_points; d.n_points = in.n_points; d.obs_row_off = (int32_t)(n_points + p); d.obs_off = (int32_t)n_obs;
        d.keyframes_in_map = in.keyframes_in_map;
        d.flags = (in.inertial ? 1 : 0) | (in.imu_initialized ? 2 : 0) | (in.inertial_ba2 ? 4 : 0) | (in.abort_ba ? 8 : 0);
        d.current_id = in.current_id; d.last_id = in.last_id;
        n_kf += in.n_keyframes; n_slots += in.slot_offsets[in.n_keyframes]; n_local += in.n_local; n_points += in.n_points;
        n_obs += in.obs_offsets[in.n_points];
        if (std::max(std::max(n_kf + p, n_slots), std::max(n_points + p, n_obs)) > kMaxRows) return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    // one buffer: [inputs | state with initial values | outputs]; the upload is the first two parts, the download the last two
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const size_t o_prob = io.take(np * sizeof(CullProblemDev)), o_pol = io.take(n_local * 4), o_flags = io.take(n_kf), o_id = io.take(n_kf * 8),
                 o_time = io.take(n_kf * 8), o_pos = io.take(n_kf * 12), o_thd = io.take(n_kf * 4), o_srow = io.take((n_kf + np) * 4),
                 o_spt = io.take(n_slots * 4), o_sdep = io.take(n_slots * 4), o_soct = io.take(n_slots), o_local = io.take(n_local * 4),
                 o_orow = io.take((n_points + np) * 4), o_okf = io.take(n_obs * 4), o_ooct = io.take(n_obs), o_ow = io.take(n_obs),
                 o_prev = io.take(n_kf * 4), o_next = io.take(n_kf * 4);
    T.state_begins();
    const size_t o_nobs = io.take(n_points * 4), o_bad = io.take(n_points);
    T.outputs_begin();
    const size_t o_verdict = io.take(n_local * 4), o_nmps = io.take(n_local * 4), o_nred = io.take(n_local * 4), o_nvis = io.take(np * 4);
    const size_t o_kfbad = work.take(n_kf), o_dead = work.take(n_obs), o_changed = work.take(n_points), o_claim = work.take(n_points * 4);
    const size_t zero_bytes = work.off;
    const size_t o_spec = work.take(n_local * 8);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceKeyframeCulling>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, dev.data(), np, sizeof(CullProblemDev));
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_culling_problem& in = problems[p];
        const CullProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, ns = (size_t)in.slot_offsets[in.n_keyframes], npt = (size_t)in.n_points, no = (size_t)in.obs_offsets[in.n_points];
        int32_t* pol = T.host<int32_t>(o_pol) + d.local_off;
        for (int i = 0; i < in.n_local; ++i) pol[i] = p;
        io.put(o_flags, d.kf_off, in.kf_flags, nk, 1); io.put(o_id, d.kf_off, in.kf_id, nk, 8); io.put(o_time, d.kf_off, in.kf_time, nk, 8);
        io.put(o_pos, d.kf_off, in.kf_imu_pos, nk, 12); io.put(o_thd, d.kf_off, in.kf_th_depth, nk, 4);
        io.put(o_srow, d.slot_row_off, in.slot_offsets, nk + 1, 4);
        io.put(o_spt, d.slot_off, in.slot_point, ns, 4); io.put(o_sdep, d.slot_off, in.slot_depth, ns, 4); io.put(o_soct, d.slot_off, in.slot_octave, ns, 1);
        io.put(o_local, d.local_off, in.local, in.n_local, 4);
        io.put(o_orow, d.obs_row_off, in.obs_offsets, npt + 1, 4);
        io.put(o_okf, d.obs_off, in.obs_kf, no, 4); io.put(o_ooct, d.obs_off, in.obs_octave, no, 1); io.put(o_ow, d.obs_off, in.obs_weight, no, 1);
        io.put(o_prev, d.kf_off, in.kf_prev, nk, 4); io.put(o_next, d.kf_off, in.kf_next, nk, 4);
        io.put(o_nobs, d.point_off, in.point_nobs, npt, 4); io.put(o_bad, d.point_off, in.point_bad, npt, 1);
    });
    TC2LI_HIP_CHECK(T.upload(st));
    TC2LI_HIP_CHECK(T.zero_work(zero_bytes, st));
    CullBatch B{};
    B.n_problems = n_problems; B.n_local = (int)n_local;
    B.problems = T.dev<const CullProblemDev>(o_prob); B.problem_of_local = T.dev<const int32_t>(o_pol);
    B.kf_flags = T.dev<const uint8_t>(o_flags); B.kf_id = T.dev<const int64_t>(o_id); B.kf_time = T.dev<const double>(o_time);
    B.kf_imu_pos = T.dev<const float>(o_pos); B.kf_th_depth = T.dev<const float>(o_thd);
    B.slot_offsets = T.dev<const int32_t>(o_srow); B.slot_point = T.dev<const int32_t>(o_spt); B.slot_depth = T.dev<const float>(o_sdep);
    B.slot_octave = T.dev<const int8_t>(o_soct); B.local = T.dev<const int32_t>(o_local);
    B.obs_offsets = T.dev<const int32_t>(o_orow); B.obs_kf = T.dev<const int32_t>(o_okf); B.obs_octave = T.dev<const int8_t>(o_ooct);
    B.obs_weight = T.dev<const uint8_t>(o_ow);
    B.kf_prev = T.dev<int32_t>(o_prev); B.kf_next = T.dev<int32_t>(o_next); B.point_nobs = T.dev<int32_t>(o_nobs); B.point_bad = T.dev<uint8_t>(o_bad);
    B.kf_bad = T.dev_work<uint8_t>(o_kfbad); B.obs_dead = T.dev_work<uint8_t>(o_dead); B.point_changed = T.dev_work<uint8_t>(o_changed);
    B.point_claim = T.dev_work<int32_t>(o_claim); B.spec = T.dev_work<int32_t>(o_spec);
    B.verdict = T.dev<int32_t>(o_verdict); B.n_mps = T.dev<int32_t>(o_nmps); B.n_redundant = T.dev<int32_t>(o_nred); B.n_visited = T.dev<int32_t>(o_nvis);
    launch_keyframe_culling(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_culling_problem& in = problems[p];
        const CullProblemDev& D = dev[p];
        const int32_t* verdict = T.host<const int32_t>(o_verdict) + D.local_off;
        const int32_t* nmps = T.host<const int32_t>(o_nmps) + D.local_off;
        const int32_t* nred = T.host<const int32_t>(o_nred) + D.local_off;
        for (int i = 0; i < in.n_local; ++i) {
            in.verdict[i] = verdict[i];
            if (verdict[i] >= 0) { in.n_mps[i] = nmps[i]; in.n_redundant[i] = nred[i]; }
        }
        *in.n_visited = T.host<const int32_t>(o_nvis)[p];
        if (in.point_bad_after) io.get(in.point_bad_after, o_bad, D.point_off, (size_t)in.n_points, 1);
        if (in.point_nobs_after) io.get(in.point_nobs_after, o_nobs, D.point_off, (size_t)in.n_points, 4);
    }
    return n_problems;
}

static int check_mp_cull(const char* entry, const uint8_t* bad, const int32_t* n_found, const int32_t* n_visible, const int64_t* first_kf_id,
                         const int32_t* n_obs, const int64_t* current_kf_id, int n_points, const uint8_t* action) {
    if (n_points < 0 || (n_points && (!bad || !n_found || !n_visible || !first_kf_id || !n_obs || !current_kf_id || !action))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

extern "C" int tc2li_host_map_point_culling_batch(const uint8_t* bad, const int32_t* n_found, const int32_t* n_visible, const int64_t* first_kf_id,
                                                  const int32_t* n_obs, const int64_t* current_kf_id, int n_points, int th_obs, uint8_t* action) {
    const int rc = check_mp_cull("tc2li_host_map_point_culling_batch", bad, n_found, n_visible, first_kf_id, n_obs, current_kf_id, n_points, action);
    if (rc < 0) return rc;
    for (int i = 0; i < n_points; ++i)
        action[i] = cull::map_point_action(bad[i] != 0, n_found[i], n_visible[i], first_kf_id[i], n_obs[i], current_kf_id[i], th_obs);
    return n_points;
}

extern "C" int tc2li_map_point_culling_batch(const uint8_t* bad, const int32_t* n_found, const int32_t* n_visible, const int64_t* first_kf_id,
                                             const int32_t* n_obs, const int64_t* current_kf_id, int n_points, int th_obs, uint8_t* action, void* stream) {
    const int rc = check_mp_cull("tc2li_map_point_culling_batch", bad, n_found, n_visible, first_kf_id, n_obs, current_kf_id, n_points, action);
    if (rc < 0) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_points == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    const size_t n = (size_t)n_points;
    PackedTransfer T;
    Packer& io = T.io;
    const size_t o_first = io.take(n * 8), o_cur = io.take(n * 8), o_found = io.take(n * 4), o_vis = io.take(n * 4), o_obs = io.take(n * 4), o_bad = io.take(n);
    T.outputs_begin();
    const size_t o_act = io.take(n);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceMapPointCulling>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_first, 0, first_kf_id, n, 8); io.put(o_cur, 0, current_kf_id, n, 8); io.put(o_found, 0, n_found, n, 4);
    io.put(o_vis, 0, n_visible, n, 4); io.put(o_obs, 0, n_obs, n, 4); io.put(o_bad, 0, bad, n, 1);
    TC2LI_HIP_CHECK(T.upload(st));
    MpCullBatch B{};
    B.n_points = n_points; B.th_obs = th_obs;
    B.bad = T.dev<const uint8_t>(o_bad); B.n_found = T.dev<const int32_t>(o_found); B.n_visible = T.dev<const int32_t>(o_vis);
    B.first_kf_id = T.dev<const int64_t>(o_first); B.n_obs = T.dev<const int32_t>(o_obs); B.current_kf_id = T.dev<const int64_t>(o_cur);
    B.action = T.dev<uint8_t>(o_act);
    launch_map_point_culling(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    io.get(action, o_act, 0, n, 1);
    return n_points;
}

// tc2li_keyframe_culling_batch / tc2li_host_keyframe_culling_batch / tc2li_map_point_culling_batch / tc2li_host_map_point_culling_batch
// (include/tc2li_hip.h "local mapping: culling"): LocalMapping::KeyFrameCulling (SF/src/LocalMapping.cc:913-1065) with the side effects of
// KeyFrame::SetBadFlag (SF/src/KeyFrame.cc:585-611) and MapPoint::EraseObservation (SF/src/MapPoint.cc:177-210) on a flat copy of the
// graph, and LocalMapping::MapPointCulling (:360-399).  This file validates the problems and either walks them in plain C++ or
// concatenates them for culling_kernels.hip.
#include <algorithm>
#include <cstring>

#include "common.hpp"
#include "culling_device.hpp"

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
    std::vector<const char*> what(n_problems, "");
    tracking_pool().parallel_for(n_problems, [&](int p) { what[p] = validate(problems[p]); });
    for (int p = 0; p < n_problems; ++p)
        if (what[p][0]) {
            set_error("%s: problem %d: %s", entry, p, what[p]);
            return TC2LI_ERR_INVALID;
        }
    return 0;
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

// the device buffers of a call, kept between calls
struct CullSpace {
    std::mutex mu;
    DevBuf<uint8_t> io, work;
    PinnedBuf<uint8_t> h_io;
};
struct MpCullSpace {
    std::mutex mu;
    DevBuf<uint8_t> io;
    PinnedBuf<uint8_t> h_io;
};

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
    const int rc = validate_all("tc2li_keyframe_culling_batch", problems, n_problems);
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
        if (std::max(std::max(n_kf + p, n_slots), std::max(n_points + p, n_obs)) > 0x7fffff00u) {
            set_error("tc2li_keyframe_culling_batch: the batch up to problem %d has more than 2^31 rows in one table; split it", p);
            return TC2LI_ERR_INVALID;
        }
    }
    const size_t np = (size_t)n_problems;
    // one buffer: [inputs | state with initial values | outputs]; the upload is the first two parts, the download the last two
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_prob = take(np * sizeof(CullProblemDev)), o_pol = take(n_local * 4), o_flags = take(n_kf), o_id = take(n_kf * 8), o_time = take(n_kf * 8),
                 o_pos = take(n_kf * 12), o_thd = take(n_kf * 4), o_srow = take((n_kf + np) * 4), o_spt = take(n_slots * 4), o_sdep = take(n_slots * 4),
                 o_soct = take(n_slots), o_local = take(n_local * 4), o_orow = take((n_points + np) * 4), o_okf = take(n_obs * 4), o_ooct = take(n_obs),
                 o_ow = take(n_obs), o_prev = take(n_kf * 4), o_next = take(n_kf * 4);
    const size_t o_nobs = take(n_points * 4), o_bad = take(n_points);
    const size_t up_bytes = off, down_from = o_nobs;
    const size_t o_verdict = take(n_local * 4), o_nmps = take(n_local * 4), o_nred = take(n_local * 4), o_nvis = take(np * 4);
    const size_t io_bytes = off;
    off = 0;
    const size_t o_kfbad = take(n_kf), o_dead = take(n_obs), o_changed = take(n_points), o_claim = take(n_points * 4);
    const size_t zero_bytes = off;
    const size_t o_spec = take(n_local * 8);
    const size_t work_bytes = off;
    CullSpace& S = shutdown_owned<CullSpace>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(S.io.ensure(io_bytes));
    TC2LI_HIP_CHECK(S.work.ensure(std::max(work_bytes, (size_t)256)));
    TC2LI_HIP_CHECK(S.h_io.ensure(io_bytes));
    uint8_t* h = S.h_io.p;
    memcpy(h + o_prob, dev.data(), np * sizeof(CullProblemDev));
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_culling_problem& in = problems[p];
        const CullProblemDev& d = dev[p];
        const size_t nk = (size_t)in.n_keyframes, ns = (size_t)in.slot_offsets[in.n_keyframes], npt = (size_t)in.n_points, no = (size_t)in.obs_offsets[in.n_points];
        auto put = [h](size_t o, size_t start, const void* src, size_t count, size_t width) {
            if (count) memcpy(h + o + start * width, src, count * width);
        };
        int32_t* pol = (int32_t*)(h + o_pol) + d.local_off;
        for (int i = 0; i < in.n_local; ++i) pol[i] = p;
        put(o_flags, d.kf_off, in.kf_flags, nk, 1); put(o_id, d.kf_off, in.kf_id, nk, 8); put(o_time, d.kf_off, in.kf_time, nk, 8);
        put(o_pos, d.kf_off, in.kf_imu_pos, nk, 12); put(o_thd, d.kf_off, in.kf_th_depth, nk, 4);
        put(o_srow, d.slot_row_off, in.slot_offsets, nk + 1, 4);
        put(o_spt, d.slot_off, in.slot_point, ns, 4); put(o_sdep, d.slot_off, in.slot_depth, ns, 4); put(o_soct, d.slot_off, in.slot_octave, ns, 1);
        put(o_local, d.local_off, in.local, in.n_local, 4);
        put(o_orow, d.obs_row_off, in.obs_offsets, npt + 1, 4);
        put(o_okf, d.obs_off, in.obs_kf, no, 4); put(o_ooct, d.obs_off, in.obs_octave, no, 1); put(o_ow, d.obs_off, in.obs_weight, no, 1);
        put(o_prev, d.kf_off, in.kf_prev, nk, 4); put(o_next, d.kf_off, in.kf_next, nk, 4);
        put(o_nobs, d.point_off, in.point_nobs, npt, 4); put(o_bad, d.point_off, in.point_bad, npt, 1);
    });
    TC2LI_HIP_CHECK(hipMemcpyAsync(S.io.p, h, up_bytes, hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemsetAsync(S.work.p, 0, std::max(zero_bytes, (size_t)256), st));
    uint8_t* d = S.io.p;
    uint8_t* w = S.work.p;
    CullBatch B{};
    B.n_problems = n_problems; B.n_local = (int)n_local;
    B.problems = (const CullProblemDev*)(d + o_prob); B.problem_of_local = (const int32_t*)(d + o_pol);
    B.kf_flags = d + o_flags; B.kf_id = (const int64_t*)(d + o_id); B.kf_time = (const double*)(d + o_time);
    B.kf_imu_pos = (const float*)(d + o_pos); B.kf_th_depth = (const float*)(d + o_thd);
    B.slot_offsets = (const int32_t*)(d + o_srow); B.slot_point = (const int32_t*)(d + o_spt); B.slot_depth = (const float*)(d + o_sdep);
    B.slot_octave = (const int8_t*)(d + o_soct); B.local = (const int32_t*)(d + o_local);
    B.obs_offsets = (const int32_t*)(d + o_orow); B.obs_kf = (const int32_t*)(d + o_okf); B.obs_octave = (const int8_t*)(d + o_ooct);
    B.obs_weight = d + o_ow;
    B.kf_prev = (int32_t*)(d + o_prev); B.kf_next = (int32_t*)(d + o_next); B.point_nobs = (int32_t*)(d + o_nobs); B.point_bad = d + o_bad;
    B.kf_bad = w + o_kfbad; B.obs_dead = w + o_dead; B.point_changed = w + o_changed; B.point_claim = (int32_t*)(w + o_claim);
    B.spec = (int32_t*)(w + o_spec);
    B.verdict = (int32_t*)(d + o_verdict); B.n_mps = (int32_t*)(d + o_nmps); B.n_redundant = (int32_t*)(d + o_nred); B.n_visited = (int32_t*)(d + o_nvis);
    launch_keyframe_culling(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(h + down_from, d + down_from, io_bytes - down_from, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_culling_problem& in = problems[p];
        const CullProblemDev& D = dev[p];
        const int32_t* verdict = (const int32_t*)(h + o_verdict) + D.local_off;
        const int32_t* nmps = (const int32_t*)(h + o_nmps) + D.local_off;
        const int32_t* nred = (const int32_t*)(h + o_nred) + D.local_off;
        for (int i = 0; i < in.n_local; ++i) {
            in.verdict[i] = verdict[i];
            if (verdict[i] >= 0) { in.n_mps[i] = nmps[i]; in.n_redundant[i] = nred[i]; }
        }
        *in.n_visited = ((const int32_t*)(h + o_nvis))[p];
        if (in.point_bad_after && in.n_points) memcpy(in.point_bad_after, h + o_bad + D.point_off, in.n_points);
        if (in.point_nobs_after && in.n_points) memcpy(in.point_nobs_after, (const int32_t*)(h + o_nobs) + D.point_off, (size_t)in.n_points * 4);
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
    size_t off = 0;
    auto take = [&off](size_t bytes) { const size_t o = off; off = align256(off + bytes); return o; };
    const size_t o_first = take(n * 8), o_cur = take(n * 8), o_found = take(n * 4), o_vis = take(n * 4), o_obs = take(n * 4), o_bad = take(n);
    const size_t up_bytes = off;
    const size_t o_act = take(n);
    MpCullSpace& S = shutdown_owned<MpCullSpace>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(S.io.ensure(off));
    TC2LI_HIP_CHECK(S.h_io.ensure(off));
    uint8_t* h = S.h_io.p;
    memcpy(h + o_first, first_kf_id, n * 8); memcpy(h + o_cur, current_kf_id, n * 8); memcpy(h + o_found, n_found, n * 4);
    memcpy(h + o_vis, n_visible, n * 4); memcpy(h + o_obs, n_obs, n * 4); memcpy(h + o_bad, bad, n);
    TC2LI_HIP_CHECK(hipMemcpyAsync(S.io.p, h, up_bytes, hipMemcpyHostToDevice, st));
    uint8_t* d = S.io.p;
    MpCullBatch B{};
    B.n_points = n_points; B.th_obs = th_obs;
    B.bad = d + o_bad; B.n_found = (const int32_t*)(d + o_found); B.n_visible = (const int32_t*)(d + o_vis);
    B.first_kf_id = (const int64_t*)(d + o_first); B.n_obs = (const int32_t*)(d + o_obs); B.current_kf_id = (const int64_t*)(d + o_cur);
    B.action = d + o_act;
    launch_map_point_culling(B, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(h + o_act, d + o_act, n, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(stream_wait_blocking(st));
    memcpy(action, h + o_act, n);
    return n_points;
}

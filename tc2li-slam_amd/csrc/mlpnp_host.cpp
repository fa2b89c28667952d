// tc2li_mlpnp_iterations / tc2li_mlpnp_ransac_batch / tc2li_host_mlpnp_ransac_batch (include/tc2li_hip.h "MLPnP RANSAC"):
// MLPnPsolver of SF/src/MLPnPsolver.cpp with the rand() values handed in.  This file validates and packs the problems (constructor :35-77,
// SetRansacParameters :205-240), draws the minimal sets (:108-120) and either runs the arithmetic of mlpnp_math.hpp on the host or hands
// the batch to mlpnp_kernels.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "mlpnp_device.hpp"
#include "mlpnp_math.hpp"
#include "packed_batch.hpp"

namespace tc2li {
namespace {

// SetRansacParameters (:205-240) for N correspondences
void ransac_parameters(int N, const tc2li_mlpnp_params& p, int* min_inliers, int* max_its) {
    float epsilon = p.epsilon;
    int n_min = (int)(N * epsilon);
    if (n_min < p.min_inliers) n_min = p.min_inliers;
    if (n_min < p.min_set) n_min = p.min_set;
    int n_it = 1;
    if (n_min != N && N > 0) {
        if (epsilon < (float)n_min / N) epsilon = (float)n_min / N;
        const double x = std::ceil(std::log(1 - p.probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
        // N < min_inliers makes the logarithm NaN; the reference's conversion to int then gives INT_MIN on x86-64, and iterate() never
        // looks at the value
        n_it = std::isnan(x) ? 1 : x > 2147483647.0 ? 2147483647 : x < -2147483648.0 ? (-2147483647 - 1) : (int)x;
    }
    *min_inliers = n_min;
    *max_its = std::max(1, std::min(n_it, p.max_iterations));
}

struct Packed {
    std::vector<MlpnpProblemDev> problems;
    std::vector<float> p2d, Xw, max_error;
    std::vector<int32_t> kp_index, idx6, problem_of_solve;
    int max_corr = 0;
};

int pack(const tc2li_mlpnp_problem* problems, int n_problems, const tc2li_mlpnp_params* params, const float* level_sigma2, int n_levels,
         const tc2li_camera* cam, int capacity, Packed& K) {
    if (n_problems < 0 || (n_problems && !problems) || !params || !level_sigma2 || n_levels < 1 || !cam || capacity < 0) {
        set_error("tc2li_mlpnp_ransac_batch: null or negative argument");
        return TC2LI_ERR_INVALID;
    }
    if (params->min_set != 6) {
        set_error("tc2li_mlpnp_ransac_batch: min_set = %d; the minimal solver takes 6 points (SF/src/Tracking.cc:3526)", params->min_set);
        return TC2LI_ERR_INVALID;
    }
    std::vector<int32_t> avail;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_mlpnp_problem& in = problems[p];
        if (in.n_keypoints < 0 || in.n_points < 0 || in.n_draws < 0 || (in.n_keypoints && (!in.keys || !in.match)) || (in.n_points && !in.Xw) ||
            (in.n_draws && !in.draws) || !in.state || (in.n_keypoints && !in.best_inlier)) {
            set_error("tc2li_mlpnp_ransac_batch: problem %d: null or negative field", p);
            return TC2LI_ERR_INVALID;
        }
        if (in.n_keypoints > capacity) {
            set_error("tc2li_mlpnp_ransac_batch: problem %d has %d keypoints, capacity is %d", p, in.n_keypoints, capacity);
            return TC2LI_ERR_CAPACITY;
        }
        MlpnpProblemDev d{};
        d.corr_off = (int32_t)K.kp_index.size();
        for (int i = 0; i < in.n_keypoints; ++i) {
            const int m = in.match[i];
            if (m < -1 || m >= in.n_points) {
                set_error("tc2li_mlpnp_ransac_batch: problem %d: match[%d] = %d outside [-1, %d)", p, i, m, in.n_points);
                return TC2LI_ERR_INVALID;
            }
            if (m < 0) continue;
            const tc2li_keypoint& kp = in.keys[i];
            if (kp.octave < 0 || kp.octave >= n_levels) {
                set_error("tc2li_mlpnp_ransac_batch: problem %d: keypoint %d has octave %d of %d levels", p, i, kp.octave, n_levels);
                return TC2LI_ERR_INVALID;
            }
            K.p2d.push_back(kp.x); K.p2d.push_back(kp.y);
            K.max_error.push_back(level_sigma2[kp.octave] * params->th2);
            K.Xw.insert(K.Xw.end(), in.Xw + 3 * (size_t)m, in.Xw + 3 * (size_t)m + 3);
            K.kp_index.push_back(i);
        }
        d.n_corr = (int32_t)K.kp_index.size() - d.corr_off;
        K.max_corr = std::max(K.max_corr, d.n_corr);
        ransac_parameters(d.n_corr, *params, &d.min_inliers, &d.max_its);
        d.n_iterations = in.n_iterations;
        d.n_keypoints = in.n_keypoints;
        d.st_iterations = in.state->iterations; d.st_best = in.state->best_inliers;
        memcpy(d.st_Tcw, in.state->best_Tcw, sizeof(d.st_Tcw));
        d.it_off = (int32_t)K.problem_of_solve.size();
        d.n_it = d.n_corr < d.min_inliers ? 0 : mlpnp::iterations_of_call(d.max_its, d.n_iterations, d.st_iterations);
        if ((long long)d.n_it * 6 > in.n_draws) {
            set_error("tc2li_mlpnp_ransac_batch: problem %d may run %d iterations and needs %d draws, %d given", p, d.n_it, 6 * d.n_it, in.n_draws);
            return TC2LI_ERR_INVALID;
        }
        for (int i = 0; i < 6 * d.n_it; ++i)
            if (in.draws[i] > 2147483647u) {
                set_error("tc2li_mlpnp_ransac_batch: problem %d: draws[%d] = %u is no rand() value (RAND_MAX = 2^31 - 1)", p, i, in.draws[i]);
                return TC2LI_ERR_INVALID;
            }
        // :100-120: six draws without replacement from a fresh copy of mvAllIndices, the taken entry replaced by the last
        for (int j = 0; j < d.n_it; ++j) {
            avail.resize(d.n_corr);
            for (int i = 0; i < d.n_corr; ++i) avail[i] = i;
            for (int i = 0; i < 6; ++i) {
                const int r = mlpnp::random_int(in.draws[6 * (size_t)j + i], (int)avail.size());
                K.idx6.push_back(avail[r]);
                avail[r] = avail.back();
                avail.pop_back();
            }
            K.problem_of_solve.push_back(p);
        }
        K.problems.push_back(d);
    }
    return 0;
}

void write_back(const tc2li_mlpnp_problem* problems, int n_problems, int capacity, const int32_t* result, const MlpnpStateOut* state,
                const uint8_t* best, int32_t* found, int32_t* no_more, int32_t* n_inliers) {
    for (int p = 0; p < n_problems; ++p) {
        if (found) found[p] = result[4 * p];
        if (no_more) no_more[p] = result[4 * p + 1];
        if (n_inliers) n_inliers[p] = result[4 * p + 2];
        problems[p].state->iterations = state[p].iterations;
        problems[p].state->best_inliers = state[p].best_inliers;
        memcpy(problems[p].state->best_Tcw, state[p].best_Tcw, sizeof(state[p].best_Tcw));
        if (problems[p].n_keypoints) memcpy(problems[p].best_inlier, best + (size_t)p * capacity, problems[p].n_keypoints);
    }
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_mlpnp_iterations(int n_correspondences, const tc2li_mlpnp_params* params, int32_t* min_inliers, int32_t* max_iterations) {
    if (!params || n_correspondences < 0) { set_error("tc2li_mlpnp_iterations: bad argument"); return TC2LI_ERR_INVALID; }
    int a, b;
    ransac_parameters(n_correspondences, *params, &a, &b);
    if (min_inliers) *min_inliers = a;
    if (max_iterations) *max_iterations = b;
    return 0;
}

extern "C" int tc2li_host_mlpnp_ransac_batch(const tc2li_mlpnp_problem* problems, int n_problems, const tc2li_mlpnp_params* params,
                                             const float* level_sigma2, int n_levels, const tc2li_camera* cam, int32_t* found, int32_t* no_more,
                                             int32_t* n_inliers, float* pose7, double* Rt12, uint8_t* inlier, int capacity) {
    Packed K;
    const int rc = pack(problems, n_problems, params, level_sigma2, n_levels, cam, capacity, K);
    if (rc < 0) return rc;
    if (!pose7 || (!inlier && capacity > 0)) { set_error("tc2li_host_mlpnp_ransac_batch: null output"); return TC2LI_ERR_INVALID; }
    const int n_solves = (int)K.problem_of_solve.size();
    const int words = std::max(1, (K.max_corr + 63) / 64);
    std::vector<double> Rt((size_t)n_solves * 12);
    std::vector<int32_t> count(n_solves);
    std::vector<unsigned long long> mask((size_t)n_solves * words);
    const float fx = (float)cam->fx, fy = (float)cam->fy, cx = (float)cam->cx, cy = (float)cam->cy;
    tracking_pool().parallel_for(n_solves, [&](int g) {
        const MlpnpProblemDev& P = K.problems[K.problem_of_solve[g]];
        const mlpnp::Corr c = {K.p2d.data() + 2 * (size_t)P.corr_off, K.Xw.data() + 3 * (size_t)P.corr_off, fx, fy, cx, cy};
        double ws[mlpnp::kWsDoubles];
        double* R = Rt.data() + 12 * (size_t)g;
        mlpnp::compute_pose6(c, K.idx6.data() + 6 * (size_t)g, mlpnp::Ws{ws, 1}, R);
        unsigned long long* m = mask.data() + (size_t)g * words;
        for (int w = 0; w < words; ++w) m[w] = 0;
        int n = 0;
        for (int i = 0; i < P.n_corr; ++i)
            if (mlpnp::is_inlier(c, i, R, K.max_error[P.corr_off + i])) { m[i >> 6] |= 1ull << (i & 63); ++n; }
        count[g] = n;
    });
    std::vector<int32_t> result((size_t)n_problems * 4);
    std::vector<MlpnpStateOut> state(n_problems);
    std::vector<uint8_t> best((size_t)n_problems * capacity);
    for (int p = 0; p < n_problems; ++p) {
        const MlpnpProblemDev& P = K.problems[p];
        const int32_t* cnt = count.data() + P.it_off;
        const mlpnp::Selection s = mlpnp::select(P.n_corr, P.min_inliers, P.max_its, P.n_iterations, P.st_iterations, P.st_best, [cnt](int j) { return cnt[j]; });
        uint8_t* in = inlier + (size_t)p * capacity;
        uint8_t* b = best.data() + (size_t)p * capacity;
        const int32_t* kp = K.kp_index.data() + P.corr_off;
        memset(in, 0, capacity);
        if (P.n_keypoints) memcpy(b, problems[p].best_inlier, P.n_keypoints);
        auto scatter = [&](int it, uint8_t* dst) {
            const unsigned long long* m = mask.data() + (size_t)(P.it_off + it) * words;
            for (int i = 0; i < P.n_corr; ++i)
                if ((m[i >> 6] >> (i & 63)) & 1ull) dst[kp[i]] = 1;
        };
        if (s.best >= 0) { memset(b, 0, P.n_keypoints); scatter(s.best, b); }
        if (s.ret >= 0) scatter(s.ret, in);
        if (s.ret == -1 && P.n_keypoints) memcpy(in, b, P.n_keypoints);
        state[p].iterations = s.iterations; state[p].best_inliers = s.best_inliers;
        for (int i = 0; i < 12; ++i) state[p].best_Tcw[i] = s.best >= 0 ? (float)Rt[12 * (size_t)(P.it_off + s.best) + i] : P.st_Tcw[i];
        double R[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        if (s.ret >= 0 || (s.ret == -1 && s.best >= 0)) memcpy(R, Rt.data() + 12 * (size_t)(P.it_off + (s.ret >= 0 ? s.ret : s.best)), sizeof(R));
        else if (s.ret == -1) for (int i = 0; i < 12; ++i) R[i] = (double)P.st_Tcw[i];
        mlpnp::pose7_of(R, pose7 + 7 * (size_t)p);
        if (Rt12) memcpy(Rt12 + 12 * (size_t)p, R, sizeof(R));
        result[4 * p] = s.found; result[4 * p + 1] = s.no_more; result[4 * p + 2] = s.n_inliers;
    }
    write_back(problems, n_problems, capacity, result.data(), state.data(), best.data(), found, no_more, n_inliers);
    return n_problems;
}

extern "C" int tc2li_mlpnp_ransac_batch(const tc2li_mlpnp_problem* problems, int n_problems, const tc2li_mlpnp_params* params,
                                        const float* level_sigma2, int n_levels, const tc2li_camera* cam, int32_t* found, int32_t* no_more,
                                        int32_t* n_inliers, float* pose7, double* Rt12, uint8_t* inlier, int capacity, void* stream) {
    Packed K;
    const int rc = pack(problems, n_problems, params, level_sigma2, n_levels, cam, capacity, K);
    if (rc < 0) return rc;
    if (!pose7 || (!inlier && capacity > 0)) { set_error("tc2li_mlpnp_ransac_batch: null output"); return TC2LI_ERR_INVALID; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    const size_t n_solves = K.problem_of_solve.size(), n_corr = K.kp_index.size(), np = (size_t)n_problems, cap = (size_t)capacity;
    const int words = std::max(1, (K.max_corr + 63) / 64);
    // one buffer: [problems, correspondences, minimal sets | the state's flags, with their values so far | outputs]
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const size_t o_prob = io.take(np * sizeof(MlpnpProblemDev)), o_p2d = io.take(n_corr * 8), o_Xw = io.take(n_corr * 12), o_err = io.take(n_corr * 4),
                 o_kp = io.take(n_corr * 4), o_idx = io.take(n_solves * 24), o_pos = io.take(n_solves * 4);
    T.state_begins();
    const size_t o_best = io.take(np * cap);
    T.outputs_begin();
    const size_t o_res = io.take(np * 16), o_state = io.take(np * sizeof(MlpnpStateOut)), o_pose = io.take(np * 28), o_Rt = io.take(np * 96),
                 o_inl = io.take(np * cap);
    const size_t o_wRt = work.take(n_solves * 96), o_cnt = work.take(n_solves * 4), o_mask = work.take(n_solves * words * 8);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceMlpnp>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, K.problems.data(), np, sizeof(MlpnpProblemDev));
    io.put(o_p2d, 0, K.p2d.data(), n_corr, 8); io.put(o_Xw, 0, K.Xw.data(), n_corr, 12);
    io.put(o_err, 0, K.max_error.data(), n_corr, 4); io.put(o_kp, 0, K.kp_index.data(), n_corr, 4);
    io.put(o_idx, 0, K.idx6.data(), n_solves, 24); io.put(o_pos, 0, K.problem_of_solve.data(), n_solves, 4);
    memset(T.host<void>(o_best), 0, np * cap);
    for (int p = 0; p < n_problems; ++p) io.put(o_best, (size_t)p * cap, problems[p].best_inlier, (size_t)problems[p].n_keypoints, 1);
    TC2LI_HIP_CHECK(T.upload(st));
    MlpnpBatch B{};
    B.n_problems = n_problems; B.n_solves = (int)n_solves; B.capacity = capacity; B.mask_words = words;
    B.fx = (float)cam->fx; B.fy = (float)cam->fy; B.cx = (float)cam->cx; B.cy = (float)cam->cy;
    B.problems = T.dev<const MlpnpProblemDev>(o_prob);
    B.p2d = T.dev<const float>(o_p2d); B.Xw = T.dev<const float>(o_Xw); B.max_error = T.dev<const float>(o_err);
    B.kp_index = T.dev<const int32_t>(o_kp); B.idx6 = T.dev<const int32_t>(o_idx); B.problem_of_solve = T.dev<const int32_t>(o_pos);
    B.Rt = T.dev_work<double>(o_wRt); B.count = T.dev_work<int32_t>(o_cnt); B.mask = T.dev_work<unsigned long long>(o_mask);
    B.result = T.dev<int32_t>(o_res); B.state = T.dev<MlpnpStateOut>(o_state); B.pose7 = T.dev<float>(o_pose);
    B.Rt12 = T.dev<double>(o_Rt); B.inlier = T.dev<uint8_t>(o_inl); B.best_inlier = T.dev<uint8_t>(o_best);
    if (!launch_mlpnp(B, st)) {
        set_error("tc2li_mlpnp_ransac_batch: the runtime refused the solve kernel's LDS");
        return TC2LI_ERR_HIP;
    }
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    io.get(pose7, o_pose, 0, np, 28);
    if (Rt12) io.get(Rt12, o_Rt, 0, np, 96);
    io.get(inlier, o_inl, 0, np * cap, 1);
    write_back(problems, n_problems, capacity, T.host<const int32_t>(o_res), T.host<const MlpnpStateOut>(o_state), T.host<const uint8_t>(o_best), found,
               no_more, n_inliers);
    return n_problems;
}

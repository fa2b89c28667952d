// tc2li_inertial_optimization_batch / tc2li_inertial_scale_refinement_batch / tc2li_host_inertial_optimization_batch /
// tc2li_host_inertial_scale_refinement_batch / tc2li_inertial_init_limits (include/tc2li_hip.h "IMU initialisation: the inertial
// optimisation, batched"): Optimizer::InertialOptimization, both overloads (SF/src/Optimizer.cc:2169-2356, 2359-2466), for many maps at
// once.  This file validates the problems and either hands each to the single-problem entry of imu_init_host.cpp on a pool thread, or
// prepares the links' informations (InertialLinkHost::prepare(1.0): the host entry's function, the host entry's bits), concatenates the maps
// into the tables of imu_init_device.hpp and sends them through imu_init_kernels.hip: one upload, one launch per form, one download.
#include <cstring>
#include <string>
#include <vector>

#include "imu_init_device.hpp"
#include "inertial_host.hpp"
#include "packed_batch.hpp"

static_assert(sizeof(tc2li_inertial_init_problem) == 136, "ABI layout");

namespace tc2li {
namespace {

// What is wrong with the arguments of one problem ("" = nothing); device: the limits of a device call apply
std::string check_arguments(const tc2li_inertial_init_problem& in, bool refine, bool device) {
    char text[160];
    if (in.n_keyframes < 2) return "fewer than 2 keyframes";
    if (in.iterations < 0) return "negative iterations";
    if (!in.Rwb9 || !in.twb3 || !in.vel3 || !in.pre || !in.Rwg9 || !in.scale) return "null Rwb9, twb3, vel3, pre, Rwg9 or scale";
    if (!refine && (!in.bg || !in.ba)) return "null bg or ba";
    if (refine && (!in.bg3 || !in.ba3)) return "null bg3 or ba3";
    if (!device) return "";
    const int most = refine ? kIiMaxRefineKeyframes : kIiMaxKeyframes;
    if (in.n_keyframes > most) {
        snprintf(text, sizeof(text), "%d keyframes are beyond the limit of %d", in.n_keyframes, most);
        return text;
    }
    if (in.iterations > kIiMaxIterations) {
        snprintf(text, sizeof(text), "%d iterations are beyond the limit of %d", in.iterations, kIiMaxIterations);
        return text;
    }
    return "";
}

int check_batch(const char* entry, const tc2li_inertial_init_problem* problems, int n_problems) {
    if (n_problems < 0 || (n_problems && !problems)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

// The single-problem entries on the pool, each on copies of what it writes: a refused batch leaves every problem as it was.
int run_host(const char* entry, const tc2li_inertial_init_problem* problems, int n_problems, bool all_refine) {
    int rc = check_batch(entry, problems, n_problems);
    if (rc < 0) return rc;
    std::vector<std::string> found(n_problems);
    rc = validate_each(entry, "problem", n_problems, [&](int p, const char** what) {
        found[p] = check_arguments(problems[p], all_refine || problems[p].refine, false);
        *what = found[p].c_str();
        return found[p].empty() ? 0 : TC2LI_ERR_INVALID;
    });
    if (rc) return rc;
    struct Out {
        std::vector<double> vel;
        double Rwg[9], scale, bg[3], ba[3], chi2[2];
        tc2li_inertial_init_stats stats;
        int rc;
    };
    std::vector<Out> out(n_problems);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_inertial_init_problem& in = problems[p];
        Out& o = out[p];
        memcpy(o.Rwg, in.Rwg9, sizeof o.Rwg);
        o.scale = *in.scale;
        if (all_refine || in.refine) {
            o.rc = tc2li_inertial_scale_refinement(in.n_keyframes, in.Rwb9, in.twb3, in.vel3, in.bg3, in.ba3, in.pre, o.Rwg, &o.scale, in.iterations, o.chi2);
            return;
        }
        o.vel.assign(in.vel3, in.vel3 + 3 * (size_t)in.n_keyframes);
        memcpy(o.bg, in.bg, sizeof o.bg); memcpy(o.ba, in.ba, sizeof o.ba);
        o.rc = tc2li_inertial_optimization(in.n_keyframes, in.Rwb9, in.twb3, o.vel.data(), in.pre, o.Rwg, &o.scale, o.bg, o.ba, in.mono, in.fixed_vel, in.prior_g,
                                           in.prior_a, in.iterations, &o.stats);
    });
    for (int p = 0; p < n_problems; ++p)
        if (out[p].rc < 0) {
            set_error("%s: problem %d: the pre-integration covariance of a link is not positive definite", entry, p);
            return out[p].rc;
        }
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_init_problem& in = problems[p];
        const Out& o = out[p];
        memcpy(in.Rwg9, o.Rwg, sizeof o.Rwg);
        *in.scale = o.scale;
        if (in.iterations_run) *in.iterations_run = o.rc;
        if (all_refine || in.refine) {
            if (in.chi2) memcpy(in.chi2, o.chi2, sizeof o.chi2);
            continue;
        }
        memcpy(in.vel3, o.vel.data(), o.vel.size() * sizeof(double));
        memcpy(in.bg, o.bg, sizeof o.bg); memcpy(in.ba, o.ba, sizeof o.ba);
        if (in.stats) *in.stats = o.stats;
    }
    return n_problems;
}

int run_device(const char* entry, const tc2li_inertial_init_problem* problems, int n_problems, bool all_refine, void* stream) {
    int rc = check_batch(entry, problems, n_problems);
    if (rc < 0) return rc;
    // the arguments, then the informations of every link: once per link and call
    std::vector<std::string> found(n_problems);
    std::vector<std::vector<double>> info(n_problems);
    rc = validate_each(entry, "problem", n_problems, [&](int p, const char** what) {
        const tc2li_inertial_init_problem& in = problems[p];
        found[p] = check_arguments(in, all_refine || in.refine, true);
        if (found[p].empty()) {
            info[p].assign((size_t)81 * in.n_keyframes, 0.0);
            for (int i = 1; i < in.n_keyframes && found[p].empty(); ++i) {
                if (!in.pre[i]) continue;
                InertialLinkHost h;
                h.pre = in.pre[i];
                if (!h.prepare(1.0)) found[p] = "the pre-integration covariance of link " + std::to_string(i) + " is not positive definite";
                else memcpy(&info[p][(size_t)81 * i], h.info, sizeof h.info);
            }
        }
        *what = found[p].c_str();
        return found[p].empty() ? 0 : TC2LI_ERR_INVALID;
    });
    if (rc) return rc;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();
    std::vector<IiProblem> dev(n_problems);
    std::vector<int32_t> which[2];
    size_t rows = 0, work_rows = 0;
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_init_problem& in = problems[p];
        const bool refine = all_refine || in.refine;
        IiProblem& d = dev[p];
        memset(&d, 0, sizeof d);
        d.kf_off = (int32_t)rows; d.n_kf = in.n_keyframes; d.work_off = (int32_t)work_rows;
        d.mono = in.mono ? 1 : 0; d.fixed_vel = in.fixed_vel ? 1 : 0; d.iterations = in.iterations;
        d.prior_g = (double)in.prior_g; d.prior_a = (double)in.prior_a;
        memcpy(d.Rwg, in.Rwg9, sizeof d.Rwg);
        d.scale = *in.scale;
        if (!refine) { memcpy(d.bg, in.bg, sizeof d.bg); memcpy(d.ba, in.ba, sizeof d.ba); }
        which[refine ? 1 : 0].push_back(p);
        rows += (size_t)in.n_keyframes;
        if (!refine) work_rows += (size_t)in.n_keyframes;
        if (9 * rows > kMaxRows) return too_many_rows(entry, p);
    }
    const size_t np = (size_t)n_problems;
    PackedTransfer T;
    Packer& io = T.io;
    const auto o_prob = io.take<IiProblem>(np);
    const auto o_which0 = io.take<int32_t>(which[0].size()), o_which1 = io.take<int32_t>(which[1].size());
    const auto o_Rwb = io.take<double>(9 * rows), o_twb = io.take<double>(3 * rows), o_bg3 = io.take<double>(3 * rows), o_ba3 = io.take<double>(3 * rows);
    const auto o_pre = io.take<PiPreint>(rows);
    const auto o_ok = io.take<uint8_t>(rows);
    T.state_begins();
    const auto o_vel = io.take<double>(3 * rows);
    T.outputs_begin();
    const auto o_res = io.take<IiResult>(np);
    const auto o_work = T.work.take<double>(work_rows * kIiWorkPerKf);
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceInertialInit>();
    std::lock_guard<std::mutex> lk(S.mu);
    TC2LI_HIP_CHECK(T.ensure(S));
    io.put(o_prob, 0, dev.data(), np);
    io.put(o_which0, 0, which[0].data(), which[0].size());
    io.put(o_which1, 0, which[1].data(), which[1].size());
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const tc2li_inertial_init_problem& in = problems[p];
        const size_t k0 = (size_t)dev[p].kf_off, nk = (size_t)in.n_keyframes;
        io.put(o_Rwb, 9 * k0, in.Rwb9, 9 * nk); io.put(o_twb, 3 * k0, in.twb3, 3 * nk); io.put(o_vel, 3 * k0, in.vel3, 3 * nk);
        if (all_refine || in.refine) { io.put(o_bg3, 3 * k0, in.bg3, 3 * nk); io.put(o_ba3, 3 * k0, in.ba3, 3 * nk); }
        PiPreint* pre = T.host(o_pre) + k0;
        uint8_t* ok = T.host(o_ok) + k0;
        for (size_t i = 0; i < nk; ++i) {
            memset(&pre[i], 0, sizeof(PiPreint));
            ok[i] = i > 0 && in.pre[i] ? 1 : 0;
            if (!ok[i]) continue;
            pi_preint_from(*in.pre[i], pre[i]);  // (the 15 x 15 covariance stays behind: the kernels read the information)
            memcpy(pre[i].info, &info[p][81 * i], sizeof pre[i].info);
        }
    });
    TC2LI_HIP_CHECK(T.upload(st));
    IiBatch B{};
    B.problems = T.dev(o_prob);
    B.Rwb = T.dev(o_Rwb); B.twb = T.dev(o_twb); B.vel = T.dev(o_vel); B.bg3 = T.dev(o_bg3); B.ba3 = T.dev(o_ba3);
    B.pre = T.dev(o_pre); B.link_ok = T.dev(o_ok); B.work = T.dev_work(o_work); B.results = T.dev(o_res);
    B.which = T.dev(o_which0); B.n = (int32_t)which[0].size();
    launch_inertial_init(B, false, st);
    B.which = T.dev(o_which1); B.n = (int32_t)which[1].size();
    launch_inertial_init(B, true, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(T.download_and_wait(st));
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_inertial_init_problem& in = problems[p];
        const IiResult& r = T.host(o_res)[p];
        memcpy(in.Rwg9, r.Rwg, sizeof r.Rwg);
        *in.scale = r.scale;
        if (in.iterations_run) *in.iterations_run = r.iterations;
        if (all_refine || in.refine) {
            if (in.chi2) memcpy(in.chi2, r.chi2, sizeof r.chi2);
            continue;
        }
        io.get(in.vel3, o_vel, 3 * (size_t)dev[p].kf_off, 3 * (size_t)in.n_keyframes);
        memcpy(in.bg, r.bg, sizeof r.bg); memcpy(in.ba, r.ba, sizeof r.ba);
        if (in.stats) {
            in.stats->iterations = r.iterations; in.stats->trials = r.trials;
            in.stats->initial_chi2 = r.chi2[0]; in.stats->final_chi2 = r.chi2[1]; in.stats->final_lambda = r.lambda;
        }
    }
    return n_problems;
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_inertial_init_limits(int32_t* out, int capacity) {
    if (!out || capacity < 3) {
        set_error("tc2li_inertial_init_limits: room for 3 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kIiMaxKeyframes; out[1] = kIiMaxRefineKeyframes; out[2] = kIiMaxIterations;
    return 3;
}

extern "C" int tc2li_inertial_init_arrow_pivot(const double D[9], const double L[9], const double Sinv_prev[9], double lambda, double Sinv[9]) {
    if (!D || !Sinv || (Sinv_prev && !L)) {
        set_error("tc2li_inertial_init_arrow_pivot: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    double G[9], S[9];
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!ii_arrow_pivot(D, Sinv_prev ? L : zero, Sinv_prev ? Sinv_prev : zero, !Sinv_prev, lambda, G, S)) return 0;
    memcpy(Sinv, S, sizeof S);
    return 1;
}

extern "C" int tc2li_host_inertial_optimization_batch(const tc2li_inertial_init_problem* problems, int n_problems) {
    return run_host("tc2li_host_inertial_optimization_batch", problems, n_problems, false);
}
extern "C" int tc2li_host_inertial_scale_refinement_batch(const tc2li_inertial_init_problem* problems, int n_problems) {
    return run_host("tc2li_host_inertial_scale_refinement_batch", problems, n_problems, true);
}
extern "C" int tc2li_inertial_optimization_batch(const tc2li_inertial_init_problem* problems, int n_problems, void* stream) {
    return run_device("tc2li_inertial_optimization_batch", problems, n_problems, false, stream);
}
extern "C" int tc2li_inertial_scale_refinement_batch(const tc2li_inertial_init_problem* problems, int n_problems, void* stream) {
    return run_device("tc2li_inertial_scale_refinement_batch", problems, n_problems, true, stream);
}

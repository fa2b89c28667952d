// LocalInertialBA / LocalLVIBA: the one-window entry points, the lock-step batch of such windows and the reduced-system solvers' entry points (include/tc2li_hip.h).
#include "lockstep_host.hpp"

using namespace tc2li;
using namespace tc2li::ba_detail;

namespace {

// ---- the host steps the one-window entry point and the lock-step batch share ----------------------------------------------------------------
static_assert(offsetof(tc2li_inertial_keyframe, Rcw) == 0 && offsetof(tc2li_inertial_keyframe, tcw) == 72, "Rcw, tcw first");
static_assert(offsetof(ImuPose, Rcw) == 0 && offsetof(ImuPose, tcw) == 72, "Rcw, tcw first");

// keyframe states: ImuCamPose on the device (authoritative), a host mirror for the inertial edges
void load_keyframes(const tc2li_inertial_keyframe* kfs, int n_kfs, std::vector<ImuPose>& hp, std::vector<ImuVertexState>& sv) {
    hp.resize(n_kfs); sv.resize(n_kfs);
    for (int k = 0; k < n_kfs; ++k) {
        memcpy(hp[k].Rcw, kfs[k].Rcw, 72); memcpy(hp[k].tcw, kfs[k].tcw, 24); memcpy(hp[k].Rwb, kfs[k].Rwb, 72); memcpy(hp[k].twb, kfs[k].twb, 24);
        hp[k].its = 0; hp[k].pad_ = 0;
        memcpy(sv[k].v, kfs[k].velocity, 24); memcpy(sv[k].bg, kfs[k].gyro_bias, 24); memcpy(sv[k].ba, kfs[k].acc_bias, 24);
    }
}
void store_keyframes(tc2li_inertial_keyframe* kfs, int n_kfs, const std::vector<ImuPose>& hp, const std::vector<ImuVertexState>& sv) {
    for (int k = 0; k < n_kfs; ++k) {
        memcpy(kfs[k].Rcw, hp[k].Rcw, 72); memcpy(kfs[k].tcw, hp[k].tcw, 24); memcpy(kfs[k].Rwb, hp[k].Rwb, 72); memcpy(kfs[k].twb, hp[k].twb, 24);
        memcpy(kfs[k].velocity, sv[k].v, 24); memcpy(kfs[k].gyro_bias, sv[k].bg, 24); memcpy(kfs[k].acc_bias, sv[k].ba, 24);
    }
}
// the LiDAR term's blocks of the reduced system (BalmTerm::add_quadratic_form)
void note_lidar_blocks(InertialTerm& inertial, const tc2li_lidar_window* lidar, const std::vector<int>& pose_var) {
    for (int i = 0; i < lidar->n_keyframes; ++i)
        for (int j = 0; j < lidar->n_keyframes; ++j) {
            const int vi = pose_var[lidar->pose_index[i]], vj = pose_var[lidar->pose_index[j]];
            if (vi >= 0 && vj >= 0) inertial.note_block(6 * vi, 6 * vj, 6, 6);
        }
}
// After the synchronisation of a linearisation: the LiDAR edge's cost (returned) and its part of the inertial normal equations.
double lvi_lidar_after_linearize(BalmTerm& lidar, bool first, const std::vector<int>& pose_var, InertialTerm& inertial) {
    if (first) lidar.finish_error();  // the computeActiveErrors() before optimize() (OptimizerWithLidar.cc:978)
    lidar.finish_error();
    const double chi = lidar.chi2();
    lidar.finish_linearization();  // constructQuadraticForm uses the stored Jacobian / Hessian when the cost grew
    lidar.add_quadratic_form(pose_var.data(), inertial.n, inertial.Hi.data(), inertial.bi.data());
    return chi;
}
// computeLambdaInit over the whole diagonal (not used by the reference's settings); sc: the kernels' sums (largest landmark / pose diagonal in [1], [2])
double lvi_lambda_init(const double* sc, const InertialTerm& inertial) {
    const int n = inertial.n;
    double mx = std::max(sc[1], sc[2]);
    for (int j = inertial.np; j < n; ++j) mx = std::max(mx, std::fabs(inertial.Hi[(size_t)j * n + j]));
    return 1e-5 * mx;
}
// computeScale() without the landmarks' part: x (lambda x + b), b = the inertial gradient + b_p of the visual term (bp [np])
double lvi_scale(const InertialTerm& inertial, const double* x, double lambda, const double* bp) {
    double scale = 0;
    for (int j = 0; j < inertial.n; ++j) {
        const double bfull = inertial.bi[j] + (j < inertial.np ? bp[j] : 0.0);
        scale += x[j] * (lambda * x[j] + bfull);
    }
    return scale;
}
// the velocity / bias part of the step x, on the host
void step_imu_states(const InertialTerm& inertial, const double* x, const std::vector<ImuVertexState>& sv, std::vector<ImuVertexState>& sv_trial) {
    sv_trial = sv;
    for (size_t k = 0; k < sv.size(); ++k)
        if (inertial.imu_var[k] >= 0) {
            const double* u = &x[inertial.np + 9 * inertial.imu_var[k]];
            for (int c = 0; c < 3; ++c) { sv_trial[k].v[c] += u[c]; sv_trial[k].bg[c] += u[3 + c]; sv_trial[k].ba[c] += u[6 + c]; }
        }
}
// the reduced system of the host's envelope LDL^T (reduced_solve.hpp: velocity / bias unknowns first, the pose rows after them):
// [S_visual + H_inertial(poses)   H_inertial(poses, imu) ; ...   H_inertial(imu) + lambda I] x = b_inertial + b_s; false: a pivot was unusable
bool lvi_host_solve(ReducedSolver& solver, const InertialTerm& inertial, const double* S, const double* bs, double lambda, std::vector<double>& rhs, std::vector<double>& x) {
    const int n = inertial.n;
    for (int j = 0; j < n; ++j) rhs[j] = inertial.bi[j] + (j < inertial.np ? bs[j] : 0.0);
    const bool ok = n == 0 ? true : solver.factorise(inertial.Hi.data(), S, lambda);
    if (ok && n) solver.solve(rhs.data(), x.data());
    return ok;
}

}  // namespace

extern "C" {

static_assert(sizeof(tc2li_imu_calib) == sizeof(ImuCalib), "ABI layout");

int tc2li_local_inertial_bundle_adjustment(tc2li_inertial_keyframe* kfs, const uint8_t* fixed, const uint8_t* has_imu, int n_kfs,
                                           const tc2li_imu_calib* calib, double* points3, int n_points, const tc2li_ba_edge* edges,
                                           int n_edges, const tc2li_inertial_link* links, int n_links, const tc2li_camera* cam,
                                           int iterations, double lambda_init, const volatile uint8_t* stop_flag, double* edge_chi2,
                                           uint8_t* edge_depth_positive, tc2li_ba_stats* stats, void* stream_) {
    return tc2li_local_lvi_bundle_adjustment(kfs, fixed, has_imu, n_kfs, calib, points3, n_points, edges, n_edges, links, n_links, cam, iterations,
                                             lambda_init, stop_flag, edge_chi2, edge_depth_positive, stats, nullptr, nullptr, nullptr, stream_);
}

int tc2li_local_lvi_bundle_adjustment(tc2li_inertial_keyframe* kfs, const uint8_t* fixed, const uint8_t* has_imu, int n_kfs,
                                      const tc2li_imu_calib* calib, double* points3, int n_points, const tc2li_ba_edge* edges, int n_edges,
                                      const tc2li_inertial_link* links, int n_links, const tc2li_camera* cam, int iterations,
                                      double lambda_init, const volatile uint8_t* stop_flag, double* edge_chi2, uint8_t* edge_depth_positive,
                                      tc2li_ba_stats* stats, const tc2li_lidar_window* lidar_window, const float* Tbl7,
                                      tc2li_lidar_ba_stats* lidar_stats, void* stream_) {
    if (!kfs || !fixed || !has_imu || !calib || !points3 || !edges || !cam || n_kfs <= 0 || n_points <= 0 || n_edges <= 0 || n_links < 0 ||
        (n_links > 0 && !links) || iterations < 0 || (lidar_window && !Tbl7)) {
        set_error("tc2li_local_inertial_bundle_adjustment: invalid argument");
        return TC2LI_ERR_INVALID;
    }
    if (lidar_stats) memset(lidar_stats, 0, sizeof(*lidar_stats));
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream_;
    if (stats) memset(stats, 0, sizeof(*stats));
    // ---- inertial edges ----
    InertialTerm inertial;
    std::vector<uint8_t> extra_used;
    {
        const int rc = inertial.prepare(links, n_links, has_imu, n_kfs, extra_used);
        if (rc < 0) return rc;
    }
    std::vector<uint8_t> imu_used = extra_used;  // keyframes whose velocity / bias vertices an inertial edge touches
    BaWorkspace& ws = ba_ws();
    std::lock_guard<std::mutex> lk(ws.mu);
    BalmTerm* lidar = nullptr;
    if (lidar_window) {
        const int rc = ws.lidar.build_body(kfs, sizeof(tc2li_inertial_keyframe), n_kfs, lidar_window, Tbl7, sizeof(ImuPose), st);
        if (rc < 0) return rc;
        lidar = &ws.lidar;
        for (int i = 0; i < lidar_window->n_keyframes; ++i) extra_used[lidar_window->pose_index[i]] = 1;
    }
    VisualProblem vp;
    {
        const int rc = vp.setup(ws, nullptr, fixed, n_kfs, points3, n_points, edges, n_edges, cam, extra_used.data(), st);
        if (rc < 0) return rc;
    }
    BaProblemDev& pb = vp.pb;
    const std::vector<int>& pose_var = vp.pose_var;
    const int n_free = vp.n_free, np = vp.np;
    inertial.number(fixed, has_imu, imu_used, n_kfs, pose_var, np);
    if (lidar_window) note_lidar_blocks(inertial, lidar_window, pose_var);
    const int n = inertial.n;
    std::vector<ImuPose> hp, hp_trial(n_kfs);
    std::vector<ImuVertexState> sv, sv_trial(n_kfs);
    load_keyframes(kfs, n_kfs, hp, sv);
    TC2LI_HIP_CHECK(ws.d_iposes.ensure(n_kfs)); TC2LI_HIP_CHECK(ws.d_iposes_trial.ensure(n_kfs)); TC2LI_HIP_CHECK(ws.h_iposes.ensure(n_kfs));
    TC2LI_HIP_CHECK(hipMemcpyAsync(ws.d_iposes.p, hp.data(), n_kfs * sizeof(ImuPose), hipMemcpyHostToDevice, st));
    pb.inertial = 1; pb.iposes = ws.d_iposes.p; pb.iposes_trial = ws.d_iposes_trial.p;
    vp.decide_trial_fused();
    memcpy(&pb.calib, calib, sizeof(ImuCalib));
    auto &h_S = ws.h_S, &h_bs = ws.h_bs, &h_xp = ws.h_xp, &h_scal = ws.h_scal;
    const size_t E = n_edges, P = n_points;

    auto stopped = [&] { return stop_flag && *stop_flag; };
    LmHost lm;
    double last_chi = 0;
    std::vector<double> rhs(std::max(n, 1)), x(std::max(n, 1), 0.0);
    ReducedSolver solver;
    // the reduced system on the device (k_lvi_solve: the kernel body of the lock-step batch, so a window gives the same bits here and there)
    const bool dev_solve = inertial.device_solve_ok();
    if (dev_solve) {
        TC2LI_HIP_CHECK(ws.lvi.ensure(np, n - np)); TC2LI_HIP_CHECK(ws.d_S.ensure((size_t)np * np)); TC2LI_HIP_CHECK(ws.d_bs.ensure(2 * (size_t)np));
        TC2LI_HIP_CHECK(ws.d_xp.ensure(n)); TC2LI_HIP_CHECK(ws.h_xp.ensure(n)); TC2LI_HIP_CHECK(ws.h_ok.ensure(1));
    }
    for (int it = 0; it < iterations && !stopped() && lm.ok; ++it) {
        ba_launch_linearize(pb, h_scal.p, h_scal.p + 1, it == 0 && !(lambda_init > 0), st);
        TC2LI_HIP_CHECK(hipGetLastError());
        if (lidar) {  // computeActiveErrors + linearizeOplus of the LiDAR edge ride on the same synchronisation
            lidar->enqueue_error(reinterpret_cast<const Se3*>(pb.iposes), st);
            const int rc = lidar->enqueue_linearization(reinterpret_cast<const Se3*>(pb.iposes), st);
            if (rc < 0) return rc;
        }
        double chi_imu = inertial.cost(hp, sv, true);  // overlaps with the kernels
        TC2LI_HIP_CHECK(hipStreamSynchronize(st));
        if (lidar) chi_imu += lvi_lidar_after_linearize(*lidar, it == 0, pose_var, inertial);
        solver.set_pattern(inertial.Hi.data(), n, np, !dev_solve);
        if (dev_solve) {
            if (solver.band() > kLviBand) { set_error("tc2li_local_lvi_bundle_adjustment: inertial band wider than the device solve holds"); return TC2LI_ERR_INVALID; }
            const size_t bytes = ws.lvi.pack(solver, inertial.Hi.data(), inertial.bi.data());
            TC2LI_HIP_CHECK(hipMemcpyAsync(ws.lvi.d_blob.p, ws.lvi.h_blob.p, bytes, hipMemcpyHostToDevice, st));
        }
        const double chi = chi_imu + h_scal.p[0];
        if (it == 0) {
            if (stats) stats->initial_chi2 = chi;
            last_chi = chi;
        }
        lm.begin_iteration(chi, it == 0, it == 0 && !(lambda_init > 0) ? lvi_lambda_init(h_scal.p, inertial) : lambda_init);
        do {
            const double lambda = lm.lambda;   // of this trial (decide() moves it on)
            bool ok2;
            if (dev_solve) {  // Schur product, solve, trial estimate and its cost in one queue, one synchronisation
                ba_launch_schur(pb, lambda, lambda, vp.n_slices, vp.k_per_slice, ws.d_S.p, ws.d_bs.p, st);
                lvi_launch_solve(ws.lvi.dev, ws.d_S.p, ws.d_bs.p, lambda, ws.d_xp.p, h_xp.p, ws.h_ok.p, st);
                TC2LI_HIP_CHECK(hipMemcpyAsync(h_bs.p + np, ws.d_bs.p + np, (size_t)np * sizeof(double), hipMemcpyDeviceToHost, st));
                ba_launch_trial(pb, ws.d_xp.p, lambda, h_scal.p + 3, h_scal.p + 4, st);
                TC2LI_HIP_CHECK(hipGetLastError());
                TC2LI_HIP_CHECK(hipMemcpyAsync(ws.h_iposes.p, pb.iposes_trial, n_kfs * sizeof(ImuPose), hipMemcpyDeviceToHost, st));
                if (lidar) lidar->enqueue_error(reinterpret_cast<const Se3*>(pb.iposes_trial), st);
                TC2LI_HIP_CHECK(hipStreamSynchronize(st));
                ok2 = ws.h_ok.p[0] != 0;
                memcpy(x.data(), h_xp.p, (size_t)n * sizeof(double));
                if (ok2) step_imu_states(inertial, x.data(), sv, sv_trial);
            } else {  // the reduced system on the host between the Schur product and the trial
                ba_launch_schur(pb, lambda, lambda, vp.n_slices, vp.k_per_slice, h_S.p, h_bs.p, st);
                TC2LI_HIP_CHECK(hipGetLastError());
                TC2LI_HIP_CHECK(hipStreamSynchronize(st));
                ok2 = lvi_host_solve(solver, inertial, h_S.p, h_bs.p, lambda, rhs, x);
                if (ok2) {
                    if (np) memcpy(h_xp.p, x.data(), np * sizeof(double));
                    ba_launch_trial(pb, h_xp.p, lambda, h_scal.p + 3, h_scal.p + 4, st);
                    TC2LI_HIP_CHECK(hipGetLastError());
                    TC2LI_HIP_CHECK(hipMemcpyAsync(ws.h_iposes.p, pb.iposes_trial, n_kfs * sizeof(ImuPose), hipMemcpyDeviceToHost, st));
                    if (lidar) lidar->enqueue_error(reinterpret_cast<const Se3*>(pb.iposes_trial), st);
                    step_imu_states(inertial, x.data(), sv, sv_trial);
                    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
                }
            }
            double scale = lvi_scale(inertial, x.data(), lambda, h_bs.p + np), trial_chi = 0;
            if (ok2) {
                memcpy(hp_trial.data(), ws.h_iposes.p, n_kfs * sizeof(ImuPose));
                trial_chi = inertial.cost(hp_trial, sv_trial, false) + h_scal.p[4];
                if (lidar) { lidar->finish_error(); trial_chi += lidar->chi2(); }
                scale += h_scal.p[3];
                last_chi = trial_chi;
            }
            if (lm.decide(ok2, trial_chi, scale)) {
                std::swap(pb.iposes, pb.iposes_trial);
                std::swap(pb.points, pb.points_trial);
                hp.swap(hp_trial);
                sv.swap(sv_trial);
            }
        } while (lm.try_again(stopped()));
        lm.end_iteration();
        if (stats) stats->final_lambda = lm.lambda;
    }
    if (stats) { stats->iterations = lm.done; stats->trials = lm.trials_total; stats->n_free_poses = n_free; stats->final_chi2 = last_chi; }
    if (lidar && lidar_stats) write_lidar_stats(*lidar, lidar_stats);
    // ---- results ----
    ba_launch_depth(pb, ws.d_depth.p, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipMemcpyAsync(points3, pb.points, 3 * P * sizeof(double), hipMemcpyDeviceToHost, st));
    if (edge_chi2) TC2LI_HIP_CHECK(hipMemcpyAsync(edge_chi2, ws.d_chi2.p, E * sizeof(double), hipMemcpyDeviceToHost, st));
    if (edge_depth_positive) TC2LI_HIP_CHECK(hipMemcpyAsync(edge_depth_positive, ws.d_depth.p, E, hipMemcpyDeviceToHost, st));
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    store_keyframes(kfs, n_kfs, hp, sv);
    return lm.done;
}

}  // extern "C"

namespace {

// ---- lock-step batch of LocalLVIBA windows (tc2li_local_lvi_bundle_adjustment_batch) -------------------------------------------
// The phases of ba_batch_lockstep (the skeleton is lockstep_host.hpp's) with the host steps of tc2li_local_lvi_bundle_adjustment between
// them: the inertial edges' normal equations (InertialTerm, overlapping the linearisation kernels), the dense reduced system [6 per free pose
// | 9 per free keyframe with IMU state] = Schur complement of the landmarks + inertial + LiDAR blocks, its LDL^T, and the inertial cost of
// every trial state (the trial ImuCamPose states come back through slot.iposes_host, written by the trial kernel).  Same kernel bodies and host
// arithmetic as the one-window entry point: a window gives the same result alone and in a batch.  The LM decisions of the inertial windows
// stay on the host: no device-side state in their slots.
struct LviWindow : WindowBase<tc2li_lvi_problem> {
    InertialTerm inertial;
    std::vector<uint8_t> imu_used;
    std::vector<ImuPose> hp, hp_trial;
    std::vector<ImuVertexState> sv, sv_trial;
    std::vector<double> rhs, x;
    ReducedSolver solver;
    bool dev_solve = false;    // the reduced system on the device (k_lvi_solve_b)
    size_t blob_bytes = 0;
    double chi_imu = 0, last_chi = 0, trial_chi = 0;
};
LockstepContext& lvi_lockstep_ctx(int group) { return shutdown_owned<LockstepContexts, 1>().c[group]; }

struct LviRun : LockstepRun {
    using LockstepRun::LockstepRun;
    std::vector<LviWindow> W;
    const tc2li_imu_calib* calib = nullptr;
    const tc2li_camera* cam = nullptr;
    bool dev_solve = false;   // the reduced systems of the call's windows on the device
    int max_lvi_np = 0, max_lvi_ni = 0;
    template <typename Fn>
    void pieces(const std::vector<int>& list, const double* xp_area, Fn&& fn) const { LockstepRun::pieces(W, list, xp_area, fn); }
};

// ---- set-up: argument checks, inertial links, plane extraction (device, queued first), uploads ----
// two tasks per window: structure + uploads (even), the LiDAR window (odd)
void lvi_setup_task(LviRun& R, int task) {
    const int i = task >> 1;
    LviWindow& w = R.W[i];
    const tc2li_lvi_problem& p = *w.p;
    hipStream_t st = R.st;
    const bool args_ok = p.keyframes && p.fixed && p.has_imu && p.points3 && p.edges && p.n_keyframes > 0 && p.n_points > 0 && p.n_edges > 0 &&
                         p.n_links >= 0 && (p.n_links == 0 || p.links) && p.iterations >= 0 && (!p.lidar || p.Tbl);
    const bool lidar_ok = !(args_ok && p.lidar) || lidar_window_ok(p.lidar, p.n_keyframes, kLockstepMaxLidarKeyframes);
    if (task & 1) {
        if (!args_ok || !lidar_ok || !p.lidar) return;
        R.rc_lidar[i] = w.ws->lidar.build_body(p.keyframes, sizeof(tc2li_inertial_keyframe), p.n_keyframes, p.lidar, p.Tbl, sizeof(ImuPose), st, &R.C.h_cut.p[i]);
        return;
    }
    if (!args_ok) { set_error("tc2li_local_lvi_bundle_adjustment_batch: problem %d: invalid argument", i); w.rc = TC2LI_ERR_INVALID; return; }
    if (!lidar_ok) { set_error("lidar window: invalid argument or pose_index out of range"); w.rc = TC2LI_ERR_INVALID; return; }
    if (p.stats) memset(p.stats, 0, sizeof(*p.stats));
    if (p.lidar_stats) memset(p.lidar_stats, 0, sizeof(*p.lidar_stats));
    const int n_kfs = p.n_keyframes;
    w.rc = w.inertial.prepare(p.links, p.n_links, p.has_imu, n_kfs, w.extra_used);
    if (w.rc < 0) return;
    w.imu_used = w.extra_used;
    if (p.lidar) for (int k = 0; k < p.lidar->n_keyframes; ++k) w.extra_used[p.lidar->pose_index[k]] = 1;
    w.rc = w.vp.setup(*w.ws, nullptr, p.fixed, n_kfs, p.points3, p.n_points, p.edges, p.n_edges, R.cam, w.extra_used.data(), st);
    if (w.rc < 0) return;
    w.inertial.number(p.fixed, p.has_imu, w.imu_used, n_kfs, w.vp.pose_var, w.vp.np);
    if (p.lidar) note_lidar_blocks(w.inertial, p.lidar, w.vp.pose_var);
    BaWorkspace& ws = *w.ws;
    load_keyframes(p.keyframes, n_kfs, w.hp, w.sv);
    w.hp_trial.resize(n_kfs); w.sv_trial.resize(n_kfs);
    if (ws.d_iposes.ensure(n_kfs) != hipSuccess || ws.d_iposes_trial.ensure(n_kfs) != hipSuccess || ws.h_iposes.ensure(n_kfs) != hipSuccess ||
        ws.h_iposes_up.ensure(n_kfs) != hipSuccess) { w.rc = TC2LI_ERR_HIP; return; }
    memcpy(ws.h_iposes_up.p, w.hp.data(), n_kfs * sizeof(ImuPose));
    if (upload_or_defer(ws.d_iposes.p, ws.h_iposes_up.p, n_kfs * sizeof(ImuPose), st) != hipSuccess) { w.rc = TC2LI_ERR_HIP; return; }
    BaProblemDev& pb = w.vp.pb;
    pb.inertial = 1; pb.iposes = ws.d_iposes.p; pb.iposes_trial = ws.d_iposes_trial.p;
    w.vp.decide_trial_fused();
    memcpy(&pb.calib, R.calib, sizeof(ImuCalib));
    const int nn = w.inertial.n;
    w.dev_solve = w.inertial.device_solve_ok();
    if (w.dev_solve) {
        const int np1 = w.vp.np;
        if (ws.lvi.ensure(np1, nn - np1) != hipSuccess || ws.d_S.ensure((size_t)np1 * np1) != hipSuccess || ws.d_bs.ensure(2 * (size_t)np1) != hipSuccess ||
            ws.d_xp.ensure(nn) != hipSuccess || ws.h_xp.ensure(nn) != hipSuccess || ws.h_ok.ensure(1) != hipSuccess) { w.rc = TC2LI_ERR_HIP; return; }
    }
    w.rhs.assign(std::max(nn, 1), 0.0); w.x.assign(std::max(nn, 1), 0.0);
}

// The reduced systems on the device or on the host, the whole call one way: a window decides for itself (InertialTerm::device_solve_ok), and
// where the windows disagree the majority stays in lock step, the others are handed back one by one to the one-window entry point -- every
// window then runs exactly as it would alone (the whole group used to go back -- one window without a velocity vertex sent 43
// through the serial path).
void lvi_choose_solver(LviRun& R) {
    int n_dev = 0, n_ok = 0;
    for (const LviWindow& w : R.W) if (w.rc >= 0) { ++n_ok; n_dev += w.dev_solve; }
    const bool keep_dev = n_dev && 2 * n_dev >= n_ok;
    for (LviWindow& w : R.W) {
        if (w.rc < 0) continue;
        if (w.dev_solve != keep_dev) { w.rc = kLockstepDeclined; continue; }
        if (keep_dev) { R.max_lvi_np = std::max(R.max_lvi_np, w.vp.np); R.max_lvi_ni = std::max(R.max_lvi_ni, w.inertial.n - w.vp.np); }
    }
    R.dev_solve = keep_dev;
}

BaBatchSlot lvi_slot(const LviWindow& w) {
    BaBatchSlot s = lockstep_slot(w);
    s.iposes_host = w.ws->h_iposes.p;  // the trial kernel leaves the trial ImuCamPose states there for the host's inertial cost
    if (w.dev_solve) {  // (x_dev / x_host take all n unknowns)
        slot_device_solve(s, w);
        s.lvi = w.ws->lvi.dev;
    }
    return s;
}

// phase A: linearisation at the accepted estimate, the inertial edges on the host meanwhile; then the host's part of it.  Returns whether
// the first trial's Schur product came with it.
bool lvi_linearize(LviRun& R, const std::vector<int>& active) {
    std::vector<LviWindow>& W = R.W;
    hipStream_t st = R.st;
    std::vector<int> with_lidar;
    bool any_maxdiag = false;
    for (int i : active) {
        W[i].begin_linearize();
        any_maxdiag |= W[i].want_maxdiag;
        if (W[i].lidar) with_lidar.push_back(i);
    }
    R.pieces(active, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_linearize(ph, cnt, R.X, any_maxdiag, st); });
    // computeActiveErrors + linearizeOplus of the LiDAR edge: the residual at the accepted estimate and the Hessian, every iteration
    // (the one-window path's enqueue_error + enqueue_linearization)
    R.pieces(with_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) {
        balm_batch_launch_residual(ph, cnt, false, st);
        balm_batch_launch_hessian(ph, cnt, R.X, st);
    });
    // (the first trial's Schur product behind the linearisation, as in ba_batch_lockstep: the host's inertial edges, the LiDAR term's change of
    // variables and the upload of the reduced system's inertial part run beside it)
    const bool pre_schur = !any_maxdiag;
    if (pre_schur) {
        for (int i : active) if (W[i].it == 0) W[i].lm.lambda = W[i].p->lambda_init;  // (what the host's part sets below)
        R.pieces(active, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_schur(ph, cnt, R.X, st); });
    }
    R.pool.parallel_for((int)active.size(), [&](int k) { LviWindow& w = W[active[k]]; w.chi_imu = w.inertial.cost(w.hp, w.sv, true); });
    R.lap(8);
    R.sync();
    if (R.failed) return false;
    R.lap(1);
    R.pool.parallel_for((int)active.size(), [&](int k) {
        LviWindow& w = W[active[k]];
        const double* sc = w.ws->h_scal.p;
        double chi_imu = w.chi_imu;
        if (w.lidar) chi_imu += lvi_lidar_after_linearize(*w.lidar, w.it == 0, w.vp.pose_var, w.inertial);
        w.solver.set_pattern(w.inertial.Hi.data(), w.inertial.n, w.vp.np, !w.dev_solve);
        if (w.dev_solve) {
            if (w.solver.band() > kLviBand) w.rc = TC2LI_ERR_INVALID;  // (device_solve_ok bounds the band by the links: not reached)
            else w.blob_bytes = w.ws->lvi.pack(w.solver, w.inertial.Hi.data(), w.inertial.bi.data());
        }
        const double chi = chi_imu + sc[0];
        if (w.it == 0) {
            if (w.p->stats) w.p->stats->initial_chi2 = chi;
            w.last_chi = chi;
        }
        w.lm.begin_iteration(chi, w.it == 0, w.it == 0 && !(w.p->lambda_init > 0) ? lvi_lambda_init(sc, w.inertial) : w.p->lambda_init);
    });
    if (R.dev_solve) {  // this linearisation's inertial / LiDAR part of the reduced systems goes up: one launch
        if (R.C.h_tasks.ensure(active.size()) != hipSuccess) { R.failed = true; return false; }
        size_t max_bytes = 0;
        for (size_t k = 0; k < active.size(); ++k) {
            LviWindow& w = W[active[k]];
            if (w.rc < 0) { R.failed = true; return false; }
            R.C.h_tasks.p[k] = CopyTask{w.ws->lvi.d_blob.p, w.ws->lvi.h_blob.p, w.blob_bytes};
            max_bytes = std::max(max_bytes, w.blob_bytes);
        }
        launch_copy_tasks(R.C.h_tasks.p, (int)active.size(), max_bytes, st);
    }
    R.lap(2);
    return pre_schur;
}

// after the synchronisation of a trial: the cost of the window's trial state (the inertial edges on the host)
void lvi_trial_cost(LviWindow& w) {
    memcpy(w.hp_trial.data(), w.ws->h_iposes.p, w.hp.size() * sizeof(ImuPose));
    w.trial_chi = w.inertial.cost(w.hp_trial, w.sv_trial, false) + w.ws->h_scal.p[4];
    if (w.lidar) { w.lidar->finish_error(); w.trial_chi += w.lidar->chi2(); }
    w.scale += w.ws->h_scal.p[3];
    w.last_chi = w.trial_chi;
}

// OptimizationAlgorithmLevenberg::solve's gain ratio and damping update for the windows of a trial; returns those that try again
std::vector<int> lvi_decide(LviRun& R, const std::vector<int>& trial) {
    std::vector<int> again;
    for (int i : trial) {
        LviWindow& w = R.W[i];
        if (w.lm.decide(w.ok2, w.trial_chi, w.scale)) {
            std::swap(w.vp.pb.iposes, w.vp.pb.iposes_trial);
            std::swap(w.vp.pb.points, w.vp.pb.points_trial);
            w.parity ^= 1;
            w.hp.swap(w.hp_trial);
            w.sv.swap(w.sv_trial);
        }
        if (w.lm.try_again(w.stopped())) again.push_back(i);
    }
    return again;
}

// Schur product, solve, trial estimate and its cost in one queue; the host sees the step, whether the factorisation went through, and
// the sums at the one synchronisation
void lvi_trials_device_solve(LviRun& R, std::vector<int> trial, bool have_schur) {
    std::vector<LviWindow>& W = R.W;
    hipStream_t st = R.st;
    while (!trial.empty() && !R.failed) {
        std::vector<int> trial_lidar;
        for (int i : trial) if (W[i].lidar) trial_lidar.push_back(i);
        R.pieces(trial, nullptr, [&](const BaPhaseHost& ph, int cnt) {
            if (!have_schur) ba_batch_launch_schur(ph, cnt, R.X, st);  // (else: this trial's product came with the linearisation)
            lvi_batch_launch_solve(ph, cnt, R.max_lvi_np, R.max_lvi_ni, st);
            ba_batch_launch_trial(ph, cnt, R.X, st);
        });
        have_schur = false;
        if (R.X.any_trial_unfused) R.pieces(trial_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, true, st); });
        R.sync();
        if (R.failed) return;
        R.lap(3);
        R.pool.parallel_for((int)trial.size(), [&](int k) {
            LviWindow& w = W[trial[k]];
            BaWorkspace& ws = *w.ws;
            w.ok2 = ws.h_ok.p[0] != 0;
            memcpy(w.x.data(), ws.h_xp.p, (size_t)w.inertial.n * sizeof(double));
            w.scale = lvi_scale(w.inertial, w.x.data(), w.lm.lambda, ws.h_bs.p + w.vp.np);
            if (!w.ok2) return;
            step_imu_states(w.inertial, w.x.data(), w.sv, w.sv_trial);
            lvi_trial_cost(w);
        });
        R.lap(6);
        trial = lvi_decide(R, trial);
    }
}

// the reduced systems on the pool threads (TC2LI_LVI_DEVICE_SOLVE=0, or windows the solve kernel does not take)
void lvi_trials_host_solve(LviRun& R, std::vector<int> trial, bool have_schur) {
    std::vector<LviWindow>& W = R.W;
    hipStream_t st = R.st;
    while (!trial.empty() && !R.failed) {
        if (have_schur) have_schur = false;  // (this trial's product came with the linearisation)
        else {
            R.pieces(trial, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_schur(ph, cnt, R.X, st); });
            R.sync();
            if (R.failed) return;
        }
        R.lap(3);
        R.pool.parallel_for((int)trial.size(), [&](int k) {
            LviWindow& w = W[trial[k]];
            BaWorkspace& ws = *w.ws;
            w.ok2 = lvi_host_solve(w.solver, w.inertial, ws.h_S.p, ws.h_bs.p, w.lm.lambda, w.rhs, w.x);
            w.scale = lvi_scale(w.inertial, w.x.data(), w.lm.lambda, ws.h_bs.p + w.vp.np);
            if (w.ok2 && w.vp.np) memcpy(ws.h_xp.p, w.x.data(), w.vp.np * sizeof(double));
        });
        R.lap(4);
        std::vector<int> step, step_lidar;
        for (int i : trial) if (W[i].ok2) { step.push_back(i); if (W[i].lidar) step_lidar.push_back(i); }
        if (!step.empty()) {
            stage_steps(R, W, step);
            R.pieces(step, R.h_xp_area, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_trial(ph, cnt, R.X, st); });
            if (R.X.any_trial_unfused) R.pieces(step_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, true, st); });  // (windows with pb.trial_fused: inside the trial launch)
            R.pool.parallel_for((int)step.size(), [&](int k) { LviWindow& w = W[step[k]]; step_imu_states(w.inertial, w.x.data(), w.sv, w.sv_trial); });  // beside the kernels
            R.sync();
            if (R.failed) return;
            R.lap(5);
            R.pool.parallel_for((int)step.size(), [&](int k) { lvi_trial_cost(W[step[k]]); });
        }
        R.lap(6);
        trial = lvi_decide(R, trial);
    }
}

// one iteration of every window that wants one; false when none does (or after a HIP error)
bool lvi_iteration(LviRun& R) {
    std::vector<int> active;
    for (int i = 0; i < R.n; ++i) if (R.W[i].wants_iteration()) active.push_back(i);
    if (active.empty() || R.failed) return false;
    R.lap(7);
    const bool have_schur = lvi_linearize(R, active);
    if (R.failed) return false;
    if (R.dev_solve) lvi_trials_device_solve(R, active, have_schur);
    else lvi_trials_host_solve(R, active, have_schur);
    for (int i : active) {
        LviWindow& w = R.W[i];
        ++w.it;
        w.lm.end_iteration();
        if (w.p->stats) w.p->stats->final_lambda = w.lm.lambda;
    }
    return true;
}

bool lvi_batch_lockstep(const tc2li_lvi_problem* problems, int n, const tc2li_imu_calib* calib, const tc2li_camera* cam, WorkerPool& pool, int32_t* results,
                        int group = 0) {
    LockstepContext& C = lvi_lockstep_ctx(group);
    std::lock_guard<std::mutex> lk(C.mu);
    if (!lidar_windows_in_range(problems, n)) return false;
    LviRun R(C, pool, n);
    R.calib = calib; R.cam = cam;
    if (!R.acquire()) return false;
    R.W.resize(n);
    for (int i = 0; i < n; ++i) R.W[i].bind(problems[i], C.ws[i].get());
    if (!lockstep_setup(R, R.W, [&](int task) { lvi_setup_task(R, task); }, false)) return false;
    lvi_choose_solver(R);
    lockstep_extent(R, R.W);
    R.X.inertial = 1;
    if (!lockstep_upload(R, R.W, [&](int i) { return lvi_slot(R.W[i]); })) return false;
    R.lap(0);
    while (lvi_iteration(R)) {}
    lockstep_results(R, R.W, false, [](const std::vector<int>&) {}, [](LviWindow& w) { store_keyframes(w.p->keyframes, w.p->n_keyframes, w.hp, w.sv); });
    R.lap(7);
    if (R.opt.timing) fprintf(stderr, "LVI lock-step timing ms (%d windows): setup %.3f inertial edges (host, kernels queued) %.3f + wait %.3f host-lin %.3f schur %.3f solve %.3f trial %.3f trial-cost %.3f results+rest %.3f total %.3f\n",
                              n, R.tm[0], R.tm[8], R.tm[1], R.tm[2], R.tm[3], R.tm[4], R.tm[5], R.tm[6], R.tm[7], R.now() - R.t_begin);
    lockstep_write_stats(R, R.W, "tc2li_local_lvi_bundle_adjustment_batch", results, [](LviWindow& w) { if (w.p->stats) w.p->stats->final_chi2 = w.last_chi; });
    return true;
}

}  // namespace

extern "C" {

int tc2li_local_lvi_bundle_adjustment_batch(const tc2li_lvi_problem* problems, int n_problems, const tc2li_imu_calib* calib, const tc2li_camera* cam,
                                            int max_concurrency, int32_t* results) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !results)) || !calib || !cam) { set_error("tc2li_local_lvi_bundle_adjustment_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    if (n_problems == 0) return 0;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const BaOptions opt = BaOptions::read();
    const bool kNoLockstep = !opt.lockstep;
    const int kGroups = opt.groups;
    // as in tc2li_local_bundle_adjustment_batch: only the windows of a group that declined go through the one-window path
    std::vector<uint8_t> todo(n_problems, 1);
    if (max_concurrency > 1 && n_problems > 1 && !kNoLockstep) {
        const int groups = std::max(1, std::min(kGroups, n_problems / 2));
        auto run_group = [&](int g) {
            const int b = (int)((long)n_problems * g / groups), e = (int)((long)n_problems * (g + 1) / groups);
            if (lvi_batch_lockstep(problems + b, e - b, calib, cam, named_pool(kPoolLviGroup0 + g), results + b, g))
                for (int i = b; i < e; ++i) todo[i] = results[i] == kLockstepDeclined;
        };
        if (groups == 1) run_group(0);
        else named_pool(kPoolLviTop).parallel_for(groups, run_group);
    }
    // one window after the other (a LiDAR window outside the batched kernels' range, or a batch of one)
    for (int i = 0; i < n_problems; ++i) {
        if (!todo[i]) continue;
        const tc2li_lvi_problem& p = problems[i];
        results[i] = tc2li_local_lvi_bundle_adjustment(p.keyframes, p.fixed, p.has_imu, p.n_keyframes, calib, p.points3, p.n_points, p.edges, p.n_edges, p.links,
                                                       p.n_links, cam, p.iterations, p.lambda_init, p.stop_flag, p.edge_chi2, p.edge_depth_positive, p.stats,
                                                       p.lidar, p.Tbl, p.lidar_stats, private_stream());
    }
    int ok = 0;
    for (int i = 0; i < n_problems; ++i) ok += results[i] >= 0;
    return ok;
}

int tc2li_host_reduced_solve(const double* Hi, const double* S, int n, int np, double lambda, const double* rhs, double* x) {
    if (!Hi || n <= 0 || np < 0 || np > n || (np > 0 && !S) || !rhs || !x) { set_error("tc2li_host_reduced_solve: invalid argument"); return TC2LI_ERR_INVALID; }
    ReducedSolver solver;
    solver.set_pattern(Hi, n, np);
    if (!solver.factorise(Hi, S, lambda)) return 0;
    solver.solve(rhs, x);
    return 1;
}

int tc2li_device_reduced_solve(const double* Hi, const double* S, int n, int np, double lambda, const double* rhs, double* x, void* stream_) {
    if (!Hi || n <= 0 || np <= 0 || np >= n || !S || !rhs || !x) { set_error("tc2li_device_reduced_solve: invalid argument"); return TC2LI_ERR_INVALID; }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    ReducedSolver solver;
    solver.set_pattern(Hi, n, np, false);
    if (np > kLviMaxPoseRows || solver.band() > kLviBand || !lvi_device_solve_available()) {
        set_error("tc2li_device_reduced_solve: %d pose unknowns / band %d: outside the kernel's range (%d / %d)", np, solver.band(), kLviMaxPoseRows, kLviBand);
        return TC2LI_ERR_INVALID;
    }
    hipStream_t st = (hipStream_t)stream_;
    BaWorkspace& ws = ba_ws();
    std::lock_guard<std::mutex> lk(ws.mu);
    TC2LI_HIP_CHECK(ws.lvi.ensure(np, n - np)); TC2LI_HIP_CHECK(ws.d_S.ensure((size_t)np * np)); TC2LI_HIP_CHECK(ws.d_bs.ensure(2 * (size_t)np));
    TC2LI_HIP_CHECK(ws.d_xp.ensure(n)); TC2LI_HIP_CHECK(ws.h_xp.ensure(n)); TC2LI_HIP_CHECK(ws.h_ok.ensure(1));
    const size_t bytes = ws.lvi.pack(solver, Hi, rhs);   // (the whole right-hand side as the inertial part's; the visual part b_s is zero)
    TC2LI_HIP_CHECK(hipMemcpyAsync(ws.lvi.d_blob.p, ws.lvi.h_blob.p, bytes, hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemcpyAsync(ws.d_S.p, S, (size_t)np * np * sizeof(double), hipMemcpyHostToDevice, st));
    TC2LI_HIP_CHECK(hipMemsetAsync(ws.d_bs.p, 0, 2 * (size_t)np * sizeof(double), st));
    lvi_launch_solve(ws.lvi.dev, ws.d_S.p, ws.d_bs.p, lambda, ws.d_xp.p, ws.h_xp.p, ws.h_ok.p, st);
    TC2LI_HIP_CHECK(hipGetLastError());
    TC2LI_HIP_CHECK(hipStreamSynchronize(st));
    memcpy(x, ws.h_xp.p, (size_t)n * sizeof(double));
    return ws.h_ok.p[0] != 0 ? 1 : 0;
}

// The same as ONE lock-step group on the context `group` (as tc2li_local_bundle_adjustment_batch_group): for the mapping workers of a multi-sequence
// camera-LiDAR-inertial system
int tc2li_local_lvi_bundle_adjustment_batch_group(const tc2li_lvi_problem* problems, int n_problems, const tc2li_imu_calib* calib, const tc2li_camera* cam,
                                                  int group, int32_t* results) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !results)) || !calib || !cam || group < 0 || group >= kMaxLockstepGroups) {
        set_error("tc2li_local_lvi_bundle_adjustment_batch_group: invalid argument (group 0 .. %d)", kMaxLockstepGroups - 1);
        return TC2LI_ERR_INVALID;
    }
    if (n_problems == 0) return 0;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const BaOptions opt = BaOptions::read();
    const bool kNoLockstep = !opt.lockstep;
    bool done = false;
    if (n_problems > 1 && !kNoLockstep) done = lvi_batch_lockstep(problems, n_problems, calib, cam, named_pool(kPoolLviGroup0 + group), results, group);
    {   // a window outside the batched kernels' range or a batch of one: all of them; windows the group handed back: those
        for (int i = 0; i < n_problems; ++i) {
            if (done && results[i] != kLockstepDeclined) continue;
            const tc2li_lvi_problem& p = problems[i];
            results[i] = tc2li_local_lvi_bundle_adjustment(p.keyframes, p.fixed, p.has_imu, p.n_keyframes, calib, p.points3, p.n_points, p.edges, p.n_edges, p.links,
                                                           p.n_links, cam, p.iterations, p.lambda_init, p.stop_flag, p.edge_chi2, p.edge_depth_positive, p.stats,
                                                           p.lidar, p.Tbl, p.lidar_stats, private_stream());
        }
    }
    int ok = 0;
    for (int i = 0; i < n_problems; ++i) ok += results[i] >= 0;
    return ok;
}

}  // extern "C"

// The lock-step batch of LocalBundleAdjustment / LocalLVBundleAdjustment windows: ba_batch_lockstep and the batch entry points (include/tc2li_hip.h).
// The skeleton of a call -- context, set-up in two passes, slot table, phases, results -- is lockstep_host.hpp's, shared with lvi_host.cpp.
#include "lockstep_host.hpp"

using namespace tc2li;
using namespace tc2li::ba_detail;

namespace {

struct LvRun : LockstepRun {
    using LockstepRun::LockstepRun;
    std::vector<LockstepWindow> W;
    const tc2li_camera* cam = nullptr;
    const BaPrepared* prepared = nullptr;
    bool dev_solve = false;   // TC2LI_BA_DEVICE_SOLVE=1 and every window within k_ba_solve_b's range
    bool device_lm = false;   // the Levenberg-Marquardt decisions on the device
    template <typename Fn>
    void pieces(const std::vector<int>& list, const double* xp_area, Fn&& fn) const { LockstepRun::pieces(W, list, xp_area, fn); }
};

// ---- set-up: argument checks, plane extraction (device, queued first: it runs while the host builds the visual structure), uploads ----
// two tasks per window: the visual structure + uploads (even), the LiDAR window (odd)
void lv_setup_task(LvRun& R, int task) {
    const int i = task >> 1;
    LockstepWindow& w = R.W[i];
    const tc2li_ba_problem& p = *w.p;
    const BaPrepared* const prep = R.prepared && R.prepared[i].sizes.n_poses > 0 ? R.prepared + i : nullptr;  // (its edges may stay on the device)
    const bool args_ok = lv_window_args_ok(p, prep != nullptr);
    const bool lidar_ok = !(args_ok && p.lidar) || lidar_window_ok(p.lidar, p.n_poses, kLockstepMaxLidarKeyframes);
    const bool kTiming = R.opt.timing && i == 0;
    const double t0 = kTiming ? R.now() : 0;
    if (task & 1) {
        if (!args_ok || !lidar_ok || !p.lidar) return;
        R.rc_lidar[i] = w.ws->lidar.build(p.poses7, p.n_poses, p.lidar, R.st, &R.C.h_cut.p[i]);
        if (kTiming) fprintf(stderr, "  window 0: lidar build %.3f ms\n", R.now() - t0);
        return;
    }
    if (!args_ok) { set_error("tc2li_local_bundle_adjustment: invalid argument"); w.rc = TC2LI_ERR_INVALID; return; }
    if (!lidar_ok) { set_error("lidar window: invalid argument or pose_index out of range"); w.rc = TC2LI_ERR_INVALID; return; }
    if (p.stats) memset(p.stats, 0, sizeof(*p.stats));
    if (p.lidar_stats) memset(p.lidar_stats, 0, sizeof(*p.lidar_stats));
    w.rc = lv_window_structure(w, prep, R.cam, R.st);   // (a prepared window's structure is the device's: no host structure, no upload)
    if (kTiming) fprintf(stderr, "  window 0: visual setup %.3f ms\n", R.now() - t0);
    if (w.rc < 0) return;
    const int np = w.vp.np;
    const size_t nn = (size_t)std::max(np * np, 1), n1 = (size_t)std::max(np, 1);
    w.Swork.assign(nn, 0.0);
    w.x.assign(n1, 0.0);
    BaWorkspace& ws = *w.ws;
    if (!lv_window_device_buffers(w) || ws.h_ok.ensure(1) != hipSuccess) { w.rc = TC2LI_ERR_HIP; return; }
    if (p.lidar) {
        // computeLambdaInit with a LiDAR term reads the diagonal of Hpp on the host (first iteration, no lambda given): where the reduction writes it
        if (ws.h_Hpp.ensure(27 * (size_t)std::max(w.vp.n_free, 1)) != hipSuccess || ws.h_Hl.ensure(nn + n1) != hipSuccess) { w.rc = TC2LI_ERR_HIP; return; }
        w.Hl = ws.h_Hl.p; w.bl_ = ws.h_Hl.p + nn;
        std::fill(w.Hl, w.Hl + nn + n1, 0.0);
    }
}

BaBatchSlot lv_slot(LvRun& R, int i) {
    const LockstepWindow& w = R.W[i];
    BaBatchSlot s;
    if (R.device_lm) { fill_device_lm_slot(s, w, R.C, i); return s; }   // (everything stays in device memory)
    s = lockstep_slot(w);
    s.lambda_init = w.p->lambda_init; s.iterations = w.p->iterations;
    s.hpp_out = w.lidar ? w.ws->h_Hpp.p : nullptr;  // written when a phase asks for it (kBaWantHpp)
    if (R.dev_solve) {
        slot_device_solve(s, w);
        if (w.lidar) { s.Hl = w.ws->d_Hl.p; s.bl_lidar = w.ws->d_Hl.p + (size_t)w.vp.np * w.vp.np; }
    }
    return s;
}

bool lv_upload(LvRun& R) {
    LockstepContext& C = R.C;
    if (R.device_lm)
        for (int i = 0; i < R.n; ++i)
            if (R.W[i].rc < 0) { C.h_lm_init.p[i] = BaLmState{}; C.h_lm.p[i] = BaLmState{}; C.h_stop.p[i] = 0; }
    const CopyTask lm_states{C.d_lm.p, C.h_lm_init.p, (size_t)R.n * sizeof(BaLmState)};
    return lockstep_upload(R, R.W, [&](int i) { return lv_slot(R, i); }, R.device_lm ? &lm_states : nullptr);
}

// ---- device-side LM: rounds queued ahead of the device, one status read per window and round ----
// A round = [linearisation set: the windows in kLmIterate | trial set: the windows in kLmTrial]; a window that accepted its step takes both
// halves of the next round, one that rejected it only the second, each at its own pace.  The host's lists are what it last SAW alive -- a
// superset: the kernels themselves skip a window whose status is not the launch's -- so round r + 1 is queued before round r has been
// waited for and the device never idles on the host; the wait is a sleeping one (no spinning thread per group: 2.8 of the 13 CPUs the
// loop kept busy in round 5), and the reduced solves, the LiDAR term's change of variables and the LM bookkeeping (5.3 more) are gone
// from the pool threads.  The caller's stop flag is polled at every round and handed to the decide kernel through a pinned word.
void lv_device_lm_loop(LvRun& R) {
    LockstepContext& C = R.C;
    std::vector<LockstepWindow>& W = R.W;
    const int n = R.n;
    for (hipEvent_t& e : C.round_done)
        if (!e && hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { e = nullptr; R.failed = true; }
    std::vector<int> live, live_lidar;
    bool first_maxdiag = false;
    BaBatchExtent XL = R.X;   // the extent of the windows still alive (the batch's fusion switches stay: a window's sums keep their order)
    auto refresh = [&] {
        const size_t before = live.size();
        live.clear(); live_lidar.clear();
        for (int i = 0; i < n; ++i)
            if (W[i].rc >= 0 && C.h_lm.p[i].status != kLmDone) { live.push_back(i); if (W[i].lidar) live_lidar.push_back(i); }
        if (live.size() != before && !live.empty()) {
            XL = batch_extent(W, live);
            XL.fuse_trial = R.X.fuse_trial; XL.fuse_linearize = R.X.fuse_linearize; XL.inertial = R.X.inertial; XL.tally = R.X.tally;
        }
    };
    refresh();
    for (int i : live) first_maxdiag |= !(W[i].p->lambda_init > 0);
    int queued = 0, seen = 0;
    auto queue_round = [&] {
        const bool first = queued == 0;
        queue_lm_round(R.d_table, W, live, live_lidar, first ? live_lidar : std::vector<int>(), XL, first && first_maxdiag, R.st);
        if (hipGetLastError() != hipSuccess || hipEventRecord(C.round_done[queued & 1], R.st) != hipSuccess) R.failed = true;
        ++queued;
        R.lap(6);  // the host's time to queue the rounds
    };
    while (!live.empty() && !R.failed) {
        if (queued == seen) queue_round();
        // one round ahead while some window cannot be finished by what is queued (it has iterations left even if every queued trial is accepted)
        if (!R.failed && queued - seen < 2) {
            bool more = false;
            for (int i : live) more |= C.h_lm.p[i].it + (queued - seen) < W[i].p->iterations;
            if (more) queue_round();
        }
        if (R.failed || event_wait_sleeping(C.round_done[seen & 1]) != hipSuccess) { R.failed = true; break; }
        ++seen;
        for (int i : live) if (W[i].stopped()) C.h_stop.p[i] = 1;
        refresh();
        R.lap(1);
    }
    if (!R.failed && queued > seen && event_wait_sleeping(C.round_done[(queued - 1) & 1]) != hipSuccess) R.failed = true;  // (a round queued ahead that found nothing to do)
    R.lap(1);
    for (int i = 0; i < n && !R.failed; ++i) {
        LockstepWindow& w = W[i];
        if (w.rc < 0) continue;
        const BaLmState& m = C.h_lm.p[i];
        w.lm.lambda = m.lambda; w.lm.currentChi = m.currentChi; w.lm.done = m.done; w.it = m.it; w.lm.trials_total = m.trials_total; w.parity = m.parity;
        if (m.parity) { std::swap(w.vp.pb.poses, w.vp.pb.poses_trial); std::swap(w.vp.pb.points, w.vp.pb.points_trial); }
        if (w.p->stats && m.done > 0) { w.p->stats->initial_chi2 = m.initial_chi2; w.p->stats->final_chi2 = m.currentChi; w.p->stats->final_lambda = m.lambda; }
        if (w.lidar) { w.lidar->error = m.lidar_error; w.lidar->hessian_evaluations = m.hessian_evaluations; }
    }
}

// ---- the host-driven loop (TC2LI_BA_DEVICE_LM=0, or a window beyond the solve kernel's range): the decisions between the phases ----
// phase A: the linearisation of the windows in `active` at the accepted estimate, queued and waited for; the host's part of it after that.
// Returns whether the first trial's Schur product came with it.
bool lv_linearize(LvRun& R, const std::vector<int>& active) {
    std::vector<LockstepWindow>& W = R.W;
    hipStream_t st = R.st;
    std::vector<int> with_lidar;
    bool any_maxdiag = false;
    for (int i : active) {
        LockstepWindow& w = W[i];
        w.begin_linearize();
        w.need_diag = w.lidar && w.want_maxdiag && w.vp.n_free > 0;
        any_maxdiag |= w.want_maxdiag;
        if (w.lidar) with_lidar.push_back(i);
    }
    R.pieces(active, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_linearize(ph, cnt, R.X, any_maxdiag, st); });
    // (running the LiDAR kernels on a second stream of the group beside the visual ones -- fork / join by events around the plane
    // Hessian and around the planes' residual of a trial -- was measured twice: round 3 with the BA stage alone, no gain; round 4 in
    // the whole loop, three A/B pairs in one call: 30.2-30.5 ms per step against 28.8-29.5 without: the events' cross-stream waits cost
    // more than the overlap of two short kernels brings)
    // the residual pass at the accepted estimate: only before the first iteration -- later the accepted estimate is the last
    // trial, whose residual and plane decompositions are still in place (same bits)
    bool first_pass = false;
    for (int i : with_lidar) first_pass |= W[i].it == 0;
    R.pieces(with_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) {
        if (first_pass) balm_batch_launch_residual(ph, cnt, false, st);
        balm_batch_launch_hessian(ph, cnt, R.X, st);
    });
    // Round 5: the first trial's Schur product does not wait for the host -- its operands are the linearisation's, its damping the window's
    // current lambda (known unless this is the first iteration of a window whose lambda comes from computeLambdaInit) -- so it is queued
    // behind the linearisation and the phase's one synchronisation covers both: a host round trip fewer per iteration, and the host's part
    // of the linearisation (the LiDAR term's change of variables) runs beside the product.
    const bool pre_schur = !R.dev_solve && !any_maxdiag;
    if (pre_schur) {
        for (int i : active) if (W[i].it == 0) W[i].lm.lambda = W[i].p->lambda_init;  // (what the host's part sets below)
        R.pieces(active, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_schur(ph, cnt, R.X, st); });
    }
    R.lap(6);  // of the phase: the time to queue it
    R.sync();
    if (R.failed) return false;
    R.lap(1);
    R.pool.parallel_for((int)active.size(), [&](int k) {
        LockstepWindow& w = W[active[k]];
        const double* sc = w.ws->h_scal.p;
        double chi = sc[0];
        w.max_pose_diag = sc[2];
        if (w.lidar) {
            chi = lidar_after_linearize(*w.lidar, chi, w.vp.pose_var.data(), w.vp.np, w.Hl, w.bl_);
            if (w.need_diag) w.max_pose_diag = max_pose_diagonal(w.ws->h_Hpp.p, w.Hl, w.vp.np);
        }
        if (w.it == 0 && w.p->stats) w.p->stats->initial_chi2 = chi;
        w.lm.begin_iteration(chi, w.it == 0, w.p->lambda_init > 0 ? w.p->lambda_init : 1e-5 * std::max(sc[1], w.max_pose_diag));
    });
    if (R.dev_solve && !with_lidar.empty()) {  // the LiDAR term of this linearisation goes where the solve kernel adds it (one launch)
        if (R.C.h_tasks.ensure(with_lidar.size()) != hipSuccess) { R.failed = true; return false; }
        size_t max_bytes = 0;
        for (size_t k = 0; k < with_lidar.size(); ++k) {
            LockstepWindow& w = W[with_lidar[k]];
            const size_t bytes = ((size_t)w.vp.np * w.vp.np + w.vp.np) * sizeof(double);
            R.C.h_tasks.p[k] = CopyTask{w.ws->d_Hl.p, w.ws->h_Hl.p, bytes};
            max_bytes = std::max(max_bytes, bytes);
        }
        launch_copy_tasks(R.C.h_tasks.p, (int)with_lidar.size(), max_bytes, st);
    }
    R.lap(2);
    return pre_schur;
}

// OptimizationAlgorithmLevenberg::solve's gain ratio and damping update for the windows of a trial; returns those that try again
std::vector<int> lv_decide(LvRun& R, const std::vector<int>& trial) {
    std::vector<int> again;
    for (int i : trial) {
        LockstepWindow& w = R.W[i];
        double trial_chi = 0;
        if (w.ok2) {
            const double* sc = w.ws->h_scal.p;
            trial_chi = sc[4];
            w.scale += sc[3];
            if (w.lidar) { w.lidar->finish_error(); trial_chi = w.lidar->chi2() + trial_chi; }
        }
        if (w.lm.decide(w.ok2, trial_chi, w.scale)) {
            std::swap(w.vp.pb.poses, w.vp.pb.poses_trial);  // the host's record (the results are read through it); the device's view: parity
            std::swap(w.vp.pb.points, w.vp.pb.points_trial);
            w.parity ^= 1;
        }
        if (w.lm.try_again(w.stopped())) again.push_back(i);
    }
    return again;
}

// TC2LI_BA_DEVICE_SOLVE=1 (read per call): the reduced systems of the batch are solved on the device (k_ba_solve_b; every window on the
// sparse Schur path, i.e. at most 21 free keyframes) -- Schur product, solve and trial estimate are then one queue of launches with one
// host round trip per LM trial instead of two, and the step is the host's bit for bit.  Built for VERDICT 5 and measured: the
// workgroup-per-window LDL^T (its substitutions are serial chains through LDS) takes longer on the stream than the host's solves on
// the pool threads plus the extra synchronisation -- 8.8 against 10.2 k frames/s at 64 sequences, no difference at 512 -- so the host
// solve stays the default.
void lv_trials_device_solve(LvRun& R, std::vector<int> trial) {
    std::vector<LockstepWindow>& W = R.W;
    hipStream_t st = R.st;
    while (!trial.empty() && !R.failed) {
        // phases B + C in one queue: Schur product, solve, trial estimate and its cost; the host sees the step, whether the
        // factorisation went through, and the sums at the one synchronisation
        std::vector<int> trial_lidar;
        for (int i : trial) if (W[i].lidar) trial_lidar.push_back(i);
        R.pieces(trial, nullptr, [&](const BaPhaseHost& ph, int cnt) {
            ba_batch_launch_schur(ph, cnt, R.X, st);
            ba_batch_launch_solve(ph, cnt, R.X, st);
            ba_batch_launch_trial(ph, cnt, R.X, st);
        });
        if (R.X.any_trial_unfused) R.pieces(trial_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, true, st); });  // (windows with pb.trial_fused: inside the trial launch)
        R.sync();
        if (R.failed) return;
        R.lap(3);
        for (int i : trial) {
            LockstepWindow& w = W[i];
            const int np = w.vp.np;
            BaWorkspace& ws = *w.ws;
            w.ok2 = np == 0 || ws.h_ok.p[0] != 0;
            w.scale = 0;
            // pose part of computeScale(): b_p (+ the LiDAR gradient) as the host path has it in h_bs[np .. 2 np)
            for (int j = 0; j < np; ++j) {
                const double bpj = w.lidar ? ws.h_bs.p[np + j] + w.bl_[j] : ws.h_bs.p[np + j];
                w.scale += ws.h_xp.p[j] * (w.lm.lambda * ws.h_xp.p[j] + bpj);
            }
        }
        R.lap(4);
        trial = lv_decide(R, trial);
    }
}

// the reduced systems on the pool threads.  have_schur: the first trial's product came with the linearisation
void lv_trials_host_solve(LvRun& R, std::vector<int> trial, bool have_schur) {
    std::vector<LockstepWindow>& W = R.W;
    hipStream_t st = R.st;
    while (!trial.empty() && !R.failed) {
        // phase B: reduced camera system at the window's lambda
        if (have_schur) have_schur = false;
        else {
            R.pieces(trial, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_schur(ph, cnt, R.X, st); });
            R.sync();
            if (R.failed) return;
        }
        R.lap(3);
        R.pool.parallel_for((int)trial.size(), [&](int k) {
            LockstepWindow& w = W[trial[k]];
            const int np = w.vp.np;
            BaWorkspace& ws = *w.ws;
            w.ok2 = true;
            if (np > 0) {
                memcpy(w.Swork.data(), ws.h_S.p, (size_t)np * np * sizeof(double));
                if (w.lidar) {
                    for (size_t q = 0; q < (size_t)np * np; ++q) w.Swork[q] += w.Hl[q];
                    for (int j = 0; j < np; ++j) { ws.h_bs.p[j] += w.bl_[j]; ws.h_bs.p[np + j] += w.bl_[j]; }
                }
                w.ok2 = ldlt_solve_small(w.Swork.data(), np, ws.h_bs.p, w.x.data(), false);
                memcpy(ws.h_xp.p, w.x.data(), np * sizeof(double));
            }
            w.scale = 0;
            for (int j = 0; j < np; ++j) w.scale += w.x[j] * (w.lm.lambda * w.x[j] + ws.h_bs.p[np + j]);
        });
        // phase C: the trial estimate and its cost
        R.lap(4);
        std::vector<int> step, step_lidar;
        for (int i : trial) if (W[i].ok2) { step.push_back(i); if (W[i].lidar) step_lidar.push_back(i); }
        if (!step.empty()) {
            stage_steps(R, W, step);
            R.pieces(step, R.h_xp_area, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_trial(ph, cnt, R.X, st); });
            if (R.X.any_trial_unfused) R.pieces(step_lidar, nullptr, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, true, st); });  // (windows with pb.trial_fused: inside the trial launch)
            R.sync();
            if (R.failed) return;
        }
        R.lap(5);
        trial = lv_decide(R, trial);
    }
}

// one iteration of every window that wants one; false when none does (or after a HIP error)
bool lv_host_iteration(LvRun& R) {
    std::vector<int> active;
    for (int i = 0; i < R.n; ++i) if (R.W[i].wants_iteration()) active.push_back(i);
    if (active.empty() || R.failed) return false;
    const bool have_schur = lv_linearize(R, active);
    if (R.failed) return false;
    if (R.dev_solve) lv_trials_device_solve(R, active);
    else lv_trials_host_solve(R, active, have_schur);
    for (int i : active) {
        LockstepWindow& w = R.W[i];
        ++w.it;
        w.lm.end_iteration();
        if (w.p->stats) { w.p->stats->final_chi2 = w.lm.currentChi; w.p->stats->final_lambda = w.lm.lambda; }
    }
    return true;
}

void lv_results(LvRun& R, int32_t* results) {
    auto outliers = [&](const std::vector<int>& all) {   // the outlier rule of the prepared windows, from the chi2 and the depth flags where the kernels left them
        if (!R.prepared) return;
        int m = 0, n_back = 0;
        size_t max_bytes = 0;
        if (R.C.h_outliers.ensure(2 * all.size()) != hipSuccess || R.C.h_write_back.ensure(2 * all.size()) != hipSuccess) { R.failed = true; return; }
        for (int i : all) {
            const BaPrepared& pr = R.prepared[i];
            if (!(pr.sizes.n_poses > 0)) continue;
            const LockstepWindow& w = R.W[i];
            if (pr.write_back) {   // the accepted estimate back over the gather's copy of the window, for a caller that goes on from it on the device
                const size_t pose_bytes = (size_t)w.vp.pb.n_poses * sizeof(Se3), point_bytes = 3 * (size_t)w.vp.pb.n_points * sizeof(double);
                R.C.h_write_back.p[n_back++] = CopyTask{const_cast<void*>(pr.poses), w.vp.pb.poses, pose_bytes};
                R.C.h_write_back.p[n_back++] = CopyTask{const_cast<void*>(pr.points), w.vp.pb.points, point_bytes};
                max_bytes = std::max(max_bytes, std::max(pose_bytes, point_bytes));
            }
            if (!pr.n_erase) continue;
            R.C.h_outliers.p[m++] = BasOutlierTask{(const tc2li_ba_edge*)w.vp.pb.edges, w.ws->d_chi2.p, w.ws->d_depth.p, pr.erase_pose, pr.erase_point,
                                                   pr.n_erase, w.vp.pb.n_edges, pr.erase_capacity};
            if (pr.erase_dev)
                R.C.h_outliers.p[m++] = BasOutlierTask{(const tc2li_ba_edge*)w.vp.pb.edges, w.ws->d_chi2.p, w.ws->d_depth.p, pr.erase_dev + 4, pr.erase_dev + 4 + pr.erase_capacity,
                                                       pr.erase_dev, w.vp.pb.n_edges, pr.erase_capacity};
        }
        launch_ba_outliers(R.C.h_outliers.p, m, R.st);
        launch_copy_tasks(R.C.h_write_back.p, n_back, max_bytes, R.st);
    };
    lockstep_results(R, R.W, true, outliers, [](LockstepWindow& w) { write_poses7(w.vp.poses, w.p->poses7); });
    lockstep_write_stats(R, R.W, "tc2li_local_bundle_adjustment_batch", results, [](LockstepWindow&) {});
    R.lap(7);
}

}  // namespace

namespace tc2li {
namespace ba_detail {

// returns false when the batch has to go through the one-thread-per-window path (a LiDAR window outside the batched kernels' range)
bool ba_batch_lockstep(const tc2li_ba_problem* problems, int n, const tc2li_camera* cam, WorkerPool& pool, int32_t* results, int group,
                       const BaPrepared* prepared) {
    LockstepContext& C = lockstep_ctx(group);
    std::lock_guard<std::mutex> lk(C.mu);
    if (!lidar_windows_in_range(problems, n)) return false;
    LvRun R(C, pool, n);
    R.cam = cam; R.prepared = prepared;
    if (!R.acquire()) return false;
    R.W.resize(n);
    for (int i = 0; i < n; ++i) R.W[i].bind(problems[i], C.ws[i].get());
    if (!lockstep_setup(R, R.W, [&](int task) { lv_setup_task(R, task); }, R.opt.timing)) return false;
    R.lap(0);
    lockstep_extent(R, R.W);
    R.dev_solve = R.opt.device_solve && R.X.max_free <= kSolveMaxFree && R.X.max_free > 0;
    // TC2LI_BA_DEVICE_LM=0: the Levenberg-Marquardt decisions of rounds 2-5, on the host between the phases.  Default (round 6): on
    // the device (ba_device.hpp: BaLmState) for every batch whose reduced systems the solve kernel takes: at most kSolveMaxFree free keyframes.
    R.device_lm = R.sleeping_sync = R.opt.device_lm && R.X.max_free <= kSolveMaxFree;
    if (R.device_lm && (C.d_lm.ensure(n) != hipSuccess || C.h_lm_init.ensure(n) != hipSuccess || C.h_lm.ensure(n) != hipSuccess || C.h_stop.ensure(n) != hipSuccess)) return false;
    if (!lv_upload(R)) return false;
    if (R.device_lm) lv_device_lm_loop(R);
    else while (lv_host_iteration(R)) {}
    lv_results(R, results);
    if (R.opt.timing) {
        const double* tm = R.tm;
        fprintf(stderr, "BA lock-step timing ms (%d windows): setup %.3f linearize %.3f (queueing %.3f) host-lin %.3f schur %.3f solve %.3f trial %.3f results %.3f total %.3f\n",
                n, tm[0], tm[1] + tm[6], tm[6], tm[2], tm[3], tm[4], tm[5], tm[7], R.now() - R.t_begin);
        // per batched launch kind: what 2-D grids of (largest extent among the launch's windows) x (windows) would start, and what the windows own
        static const char* const kNames[kGridKinds] = {"linearize", "reduce_all", "schur_lean", "schur_finish", "trial_fused", "trial_update", "errors", "depth",
                                                       "balm_hessian", "balm_combine"};
        for (int k = 0; k < kGridKinds; ++k)
            if (R.tally.launches[k])
                fprintf(stderr, "BA lock-step grids (%d windows): %-12s launches %llu workgroups 2-D %llu own %llu (%.1f %%)\n", n, kNames[k], (unsigned long long)R.tally.launches[k],
                        (unsigned long long)R.tally.rect[k], (unsigned long long)R.tally.own[k], R.tally.rect[k] ? 100.0 * (double)R.tally.own[k] / (double)R.tally.rect[k] : 0.0);
    }
    return true;
}

}  // namespace ba_detail
}  // namespace tc2li

extern "C" {

int tc2li_local_bundle_adjustment_batch(const tc2li_ba_problem* problems, int n_problems, const tc2li_camera* cam, int max_concurrency,
                                        int32_t* results) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !results)) || !cam) { set_error("tc2li_local_bundle_adjustment_batch: invalid argument"); return TC2LI_ERR_INVALID; }
    if (n_problems == 0) return 0;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const int workers = std::max(1, std::min(std::min(max_concurrency, n_problems), 16));
    WorkerPool* pool = &named_pool(kPoolBaGroup0);  // persistent: its threads keep their streams and workspaces
    const BaOptions opt = BaOptions::read();
    const bool kNoLockstep = !opt.lockstep;
    // The lock-step loop is a chain of dependent launches with a host step after every phase: while the host works the stream is
    // empty.  Several groups of windows, each a lock-step batch of its own on its own stream and host thread, fill each other's gaps.
    const int kGroups = opt.groups;
    // windows the lock-step groups could not take (a LiDAR window outside the batched kernels' range: a group that declines has written
    // nothing but zeroed stats) go through the one-window path below -- those windows only, every other window keeps its lock-step result
    std::vector<uint8_t> todo(n_problems, 1);
    if (max_concurrency > 1 && n_problems > 1 && !kNoLockstep) {
        const int groups = std::max(1, std::min(kGroups, n_problems / 2));
        // the setup of a group (per window: graph structure + staging, plane extraction of the LiDAR window) and the per-window host steps
        // between the phases (LiDAR quadratic form, 6K LDL^T) are host work on the group's own pool (common.cpp pool_threads: 16 threads per
        // group on a one-GPU box -- 8 -> 16 took the step from 41.8-42.9 to 40.7-40.8 ms in round 2, 32: 41.0 -- fewer under a smaller budget)
        auto run_group = [&](int g) {
            const int b = (int)((long)n_problems * g / groups), e = (int)((long)n_problems * (g + 1) / groups);
            if (ba_batch_lockstep(problems + b, e - b, cam, named_pool(kPoolBaGroup0 + g), results + b, g))
                std::fill(todo.begin() + b, todo.begin() + e, (uint8_t)0);
        };
        if (groups == 1) run_group(0);
        else named_pool(kPoolBaTop).parallel_for(groups, run_group);
    }
    std::vector<int> rest;
    for (int i = 0; i < n_problems; ++i) if (todo[i]) rest.push_back(i);
    if (rest.empty()) {
        int ok_ = 0;
        for (int i = 0; i < n_problems; ++i) ok_ += results[i] >= 0;
        return ok_;
    }
    struct ThreadStream {
        hipStream_t s = nullptr;
        ~ThreadStream() { if (s) (void)hipStreamDestroy(s); }
    };
    std::atomic<int> next{0};
    pool->parallel_for(std::min(workers, (int)rest.size()), [&](int) {
        static thread_local ThreadStream ts;
        if (!ts.s && hipStreamCreateWithFlags(&ts.s, hipStreamNonBlocking) != hipSuccess) ts.s = nullptr;
        for (int k; (k = next.fetch_add(1)) < (int)rest.size();) {
            const int i = rest[k];
            const tc2li_ba_problem& p = problems[i];
            results[i] = tc2li_local_lv_bundle_adjustment(p.poses7, p.fixed, p.n_poses, p.points3, p.n_points, p.edges, p.n_edges, cam,
                                                          p.iterations, p.lambda_init, p.stop_flag, p.edge_chi2, p.edge_depth_positive,
                                                          p.stats, p.lidar, p.lidar_stats, ts.s);
        }
    });
    int ok = 0;
    for (int i = 0; i < n_problems; ++i) ok += results[i] >= 0;
    return ok;
}

int tc2li_local_bundle_adjustment_batch_group(const tc2li_ba_problem* problems, int n_problems, const tc2li_camera* cam, int group, int32_t* results) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !results)) || !cam || group < 0 || group >= kMaxLockstepGroups) {
        set_error("tc2li_local_bundle_adjustment_batch_group: invalid argument (group 0 .. %d)", kMaxLockstepGroups - 1);
        return TC2LI_ERR_INVALID;
    }
    if (n_problems == 0) return 0;
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    const BaOptions opt = BaOptions::read();
    const bool kNoLockstep = !opt.lockstep;
    // ONE lock-step group on the caller's thread: the context `group` (stream, work spaces, host pool) is the caller's choice, so that the
    // mapping workers of a multi-sequence system run their windows side by side without meeting at the end of a common call
    bool done = false;
    if (n_problems > 1 && !kNoLockstep) done = ba_batch_lockstep(problems, n_problems, cam, named_pool(kPoolBaGroup0 + group), results, group);
    if (!done) {  // a window outside the batched kernels' range (the group has written nothing but zeroed stats), or a batch of one
        for (int i = 0; i < n_problems; ++i) {
            const tc2li_ba_problem& p = problems[i];
            results[i] = tc2li_local_lv_bundle_adjustment(p.poses7, p.fixed, p.n_poses, p.points3, p.n_points, p.edges, p.n_edges, cam, p.iterations,
                                                          p.lambda_init, p.stop_flag, p.edge_chi2, p.edge_depth_positive, p.stats, p.lidar,
                                                          p.lidar_stats, private_stream());
        }
    }
    int ok = 0;
    for (int i = 0; i < n_problems; ++i) ok += results[i] >= 0;
    return ok;
}

}  // extern "C"

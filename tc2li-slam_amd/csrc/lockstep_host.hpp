// What the lock-step drivers of the local bundle adjustment share (ba_lockstep.cpp: LocalBA / LocalLVBA windows; lvi_host.cpp: LocalInertialBA /
// LocalLVIBA windows; ba_engine.cpp: the running queue): the window record, the context of a group, the skeleton of a call -- set-up in two
// passes, slot table, phases, results -- and the device-side Levenberg-Marquardt round.  Host only: no .hip includes this header.
#pragma once
#include "ba_internal.hpp"
#include "lm_host.hpp"

namespace tc2li {
namespace ba_detail {

// ---- the LiDAR term's host steps (one-window entries and lock-step drivers alike) ----------------------------------------------------------
constexpr int kLockstepMaxLidarKeyframes = 7;   // keyframes of a LiDAR window the batched kernels take
// a LiDAR window of 1 .. max_keyframes keyframes whose pose_index entries name poses of the window
inline bool lidar_window_ok(const tc2li_lidar_window* lidar, int n_poses, int max_keyframes) {
    if (lidar->n_keyframes < 1 || lidar->n_keyframes > max_keyframes || !lidar->pose_index) return false;
    for (int k = 0; k < lidar->n_keyframes; ++k) if (lidar->pose_index[k] < 0 || lidar->pose_index[k] >= n_poses) return false;
    return true;
}
// After the synchronisation of a linearisation of a LocalLVBA window: the LiDAR edge's cost joins the visual one, its Jacobian / Hessian
// (constructQuadraticForm uses the stored ones when the cost grew) become the dense pose-pose block Hl and the gradient bl.  Returns chi2.
inline double lidar_after_linearize(BalmTerm& lidar, double chi_visual, const int* pose_var, int np, double* Hl, double* bl) {
    lidar.finish_error();
    const double chi = lidar.chi2() + chi_visual;
    lidar.finish_linearization();
    std::fill(Hl, Hl + (size_t)np * np, 0.0);
    std::fill(bl, bl + np, 0.0);
    lidar.add_quadratic_form(pose_var, np, Hl, bl);
    return chi;
}
// computeLambdaInit's largest pose diagonal when another term adds to Hpp: hpp = the packed upper triangles of the 6 x 6 blocks, Hl or NULL
inline double max_pose_diagonal(const double* hpp, const double* Hl, int np) {
    static const int dpos[6] = {0, 6, 11, 15, 18, 20};  // diagonal of the packed upper triangle
    double mx = 0;
    for (int j = 0; j < np; ++j) mx = std::max(mx, std::fabs(hpp[27 * (size_t)(j / 6) + dpos[j % 6]] + (Hl ? Hl[(size_t)j * np + j] : 0.0)));
    return mx;
}
template <typename Stats>
void write_lidar_stats(const BalmTerm& lidar, Stats* out) {
    out->n_planes = lidar.n_planes; out->hessian_evaluations = lidar.hessian_evaluations;
    out->residual = lidar.error; out->chi2 = lidar.chi2();
}

// ---- lock-step batch -----------------------------------------------------------------------------------------------------
// All windows advance through the phases of the Levenberg-Marquardt loop together: one launch per kernel and one stream
// synchronisation per phase for the whole batch (a window alone is bound by launch and synchronisation latency: its kernels take
// 5-20 us each).  The arithmetic of a window is the one of tc2li_local_lv_bundle_adjustment (same kernel bodies, same host
// steps), so the results are identical to optimising the windows one by one.
// Problem: tc2li_ba_problem or tc2li_lvi_problem (the fields read here have the same names in both).
template <typename Problem>
struct WindowBase {
    const Problem* p = nullptr;
    BaWorkspace* ws = nullptr;
    VisualProblem vp;
    BalmTerm* lidar = nullptr;
    std::vector<uint8_t> extra_used;
    LmHost lm;       // the host's Levenberg-Marquardt state (device-side LM: what the device's state ended with)
    double scale = 0;
    int it = 0, rc = 0;
    int parity = 0;  // 1: the accepted estimate lives in the trial buffers of the slot (an odd number of accepted steps)
    bool ok2 = true, need_diag = false, want_maxdiag = false;
    void bind(const Problem& problem, BaWorkspace* workspace) { p = &problem; ws = workspace; }
    bool wants_hpp() const { return need_diag; }
    bool stopped() const { return p->stop_flag && *p->stop_flag; }
    bool wants_iteration() const { return rc >= 0 && it < p->iterations && !stopped() && lm.ok; }
    void begin_linearize() { want_maxdiag = it == 0 && !(p->lambda_init > 0); }
};
struct LockstepWindow : WindowBase<tc2li_ba_problem> {
    std::vector<double> Swork, x;
    double *Hl = nullptr, *bl_ = nullptr;  // the LiDAR term's (6K)^2 Hessian and 6K gradient (pinned: ws->h_Hl)
    double max_pose_diag = 0;
};
// The set-up of a LocalBA / LocalLVBA window as the batch and the engine share it: the argument check (a prepared window's edges may stay on
// the device), ...
inline bool lv_window_args_ok(const tc2li_ba_problem& p, bool prepared) {
    return p.poses7 && p.fixed && p.points3 && (p.edges || prepared) && p.n_poses > 0 && p.n_points > 0 && p.n_edges > 0 && p.iterations >= 0;
}
// ... the structure with the keyframes of the LiDAR window counted as used (prep: the structure is the device's -- no host structure, no upload), ...
inline int lv_window_structure(LockstepWindow& w, const BaPrepared* prep, const tc2li_camera* cam, hipStream_t st) {
    const tc2li_ba_problem& p = *w.p;
    if (prep) return w.vp.adopt(*w.ws, *prep, cam, st);
    if (p.lidar) {
        w.extra_used.assign(p.n_poses, 0);
        for (int k = 0; k < p.lidar->n_keyframes; ++k) w.extra_used[p.lidar->pose_index[k]] = 1;
    }
    return w.vp.setup(*w.ws, p.poses7, p.fixed, p.n_poses, p.points3, p.n_points, p.edges, p.n_edges, cam, w.extra_used.empty() ? nullptr : w.extra_used.data(), st);
}
// ... and what the solve kernel and the device-side LM keep in device memory: S, [b_s | b_p], the step, the sums; the LiDAR term's block and records
inline bool lv_window_device_buffers(LockstepWindow& w) {
    BaWorkspace& ws = *w.ws;
    const size_t nn = (size_t)std::max(w.vp.np * w.vp.np, 1), n1 = (size_t)std::max(w.vp.np, 1);
    if (ws.d_S.ensure(nn) != hipSuccess || ws.d_bs.ensure(2 * n1) != hipSuccess || ws.d_xp.ensure(n1) != hipSuccess || ws.d_scal.ensure(8) != hipSuccess) return false;
    if (!w.p->lidar) return true;
    const size_t nl = 6 * (size_t)w.p->lidar->n_keyframes;
    return ws.d_Hl.ensure(nn + n1) == hipSuccess && ws.d_balm_out.ensure((size_t)balm_out_size(w.p->lidar->n_keyframes)) == hipSuccess && ws.d_lidar_JH.ensure(nl + nl * nl) == hipSuccess;
}

// The windows `list[c0 .. c1)` of a phase as kernel arguments (ba_device.hpp BaPhase): table index, parity / request bits, lambda --
// and, beside them on the host, each window's own sizes, from which a launch wrapper cuts the compact grid of its kernel.
template <typename Win>
BaPhaseHost make_phase(const BaBatchSlot* d_table, const double* xp_area, const std::vector<Win>& W, const std::vector<int>& list, size_t c0, size_t c1, int expect = 0) {
    BaPhaseHost ph;
    ph.table = d_table; ph.xp_area = xp_area; ph.first = (int32_t)c0; ph.pad_ = 0; ph.expect = expect; ph.n = (int32_t)(c1 - c0);
    ph.first_block[0] = 0;
    for (size_t k = c0; k < c1; ++k) {
        const Win& w = W[list[k]];
        ph.win[k - c0] = (uint16_t)list[k];
        ph.flags[k - c0] = (uint8_t)((w.parity ? kBaAcceptedInTrial : 0u) | (w.want_maxdiag ? kBaWantMaxdiag : 0u) | (w.wants_hpp() ? kBaWantHpp : 0u));
        ph.lambda[k - c0] = w.lm.lambda;
        BaWindowExtent& e = ph.own[k - c0];
        e = BaWindowExtent{};
        if (w.rc < 0) continue;  // (its slot is empty: no kernel has work for it)
        const BaProblemDev& pb = w.vp.pb;
        e.n_groups = pb.n_groups; e.n_free_edges = pb.n_free_edges; e.n_edges = pb.n_edges; e.n_points = pb.n_points; e.n_poses = pb.n_poses; e.n_free = pb.n_free;
        if (pb.sparse_schur && pb.n_free > 0) e.schur_lean_blocks = w.vp.n_slices * (pb.n_free > kSchurBlocksMaxFree ? 2 : 1);
        e.trial_fused = pb.trial_fused;
        if (w.lidar) { e.has_lidar = 1; e.lidar_chunks = w.lidar->dev.n_chunks; e.lidar_W = w.lidar->W; }
    }
    return ph;
}
// fn(phase, windows in it) for every piece of at most kBaPhaseMax windows of `list`
template <typename Win, typename Fn>
void for_phase_pieces(const BaBatchSlot* d_table, const double* xp_area, const std::vector<Win>& W, const std::vector<int>& list, Fn&& fn, int expect = 0) {
    for (size_t c0 = 0; c0 < list.size(); c0 += kBaPhaseMax) {
        const size_t c1 = std::min(list.size(), c0 + (size_t)kBaPhaseMax);
        const BaPhaseHost ph = make_phase(d_table, xp_area, W, list, c0, c1, expect);
        fn(ph, (int)(c1 - c0));
    }
}

struct LockstepContext {
    std::mutex mu;
    std::vector<std::unique_ptr<BaWorkspace>> ws;
    // slot table and, behind it, the steps x_p of a trial phase (pinned half: the trial kernels read them there)
    DevBuf<uint8_t> d_table;
    PinnedBuf<uint8_t> h_table;
    PinnedBuf<CopyTask> h_tasks;  // the uploads / operand fills of a batch's setup, then its result copies: one launch each (copy_kernels.hip)
    PinnedBuf<BasOutlierTask> h_outliers;  // prepared windows: the outlier rule after the BA, a task per window (ba_structure_kernels.hip), two where a device copy is asked for
    PinnedBuf<CopyTask> h_write_back;      // prepared windows with BaPrepared::write_back: the final estimate back over the caller's device arrays (h_tasks is still being read)
    // plane extraction of the batch's LiDAR windows on the device (balm_cut_kernels.hip): a task per window, those with points to cut
    // compacted into the list the kernels read, and the uploads the LiDAR tasks deferred (the clouds)
    PinnedBuf<BalmCutTask> h_cut, h_cut_list;
    DevBuf<BalmCutTask> d_cut_list;
    PinnedBuf<CopyTask> h_cut_copies;
    // device-side LM: the windows' states (device), their initial values and the mirror the decide kernel writes (pinned), the stop words
    DevBuf<BaLmState> d_lm;
    PinnedBuf<BaLmState> h_lm_init, h_lm;
    PinnedBuf<int32_t> h_stop;
    hipEvent_t round_done[2] = {nullptr, nullptr};
    hipStream_t st = nullptr;
    ~LockstepContext() {
        for (hipEvent_t e : round_done) if (e) (void)hipEventDestroy(e);
        if (st) (void)hipStreamDestroy(st);
    }
};
struct LockstepContexts { LockstepContext c[kMaxLockstepGroups]; };
inline LockstepContext& lockstep_ctx(int group) { return shutdown_owned<LockstepContexts, 0>().c[group]; }

// The stream of a lock-step loop.  The loop is a chain of ~140 short dependent launches: on a GPU shared with the front-end kernels they go
// first.  (Round 6 also tried compute units of their own -- hipExtStreamCreateWithCUMask: the lock-step groups on 32 / 64 / 96 of the 256,
// every other stream of the loop on the rest.  A chain of tiny kernels beside GEMMs gains 25x from that; this one does not: its large kernels
// want the whole chip -- 512 sequences 9.6 / 14.7 / 16.8 k frames/s against 20.2 k unpartitioned, 64 sequences 8.3 / 12.0 k against 15.1 k.
// Removed.)
inline bool create_priority_stream(hipStream_t* st) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    if (hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi) == hipSuccess || hipStreamCreateWithFlags(st, hipStreamNonBlocking) == hipSuccess) return true;
    *st = nullptr;
    return false;
}

// The LiDAR half of a lock-step batch's setup, after its tasks (the odd entries of `deferred`) have staged the clouds and described the
// extractions in C.h_cut[0..n): the uploads and the extraction kernels of all windows are queued in one go, so that they run while the
// host builds the visual structure.  plane_extraction_finish (after that) waits for them and gives every window its planes.
inline bool plane_extraction_begin(LockstepContext& C, std::vector<std::vector<CopyTask>>& deferred, int n, hipStream_t st) {
    int m = 0, max_points = 0, max_table = 0;
    if (C.h_cut_list.ensure(std::max(n, 1)) != hipSuccess || C.d_cut_list.ensure(std::max(n, 1)) != hipSuccess) return false;
    for (int i = 0; i < n; ++i) {
        const BalmCutTask& t = C.h_cut.p[i];
        if (t.n_points <= 0) continue;
        C.h_cut_list.p[m++] = t;
        max_points = std::max(max_points, t.n_points);
        max_table = std::max(max_table, 1 << t.table_bits);
    }
    if (!m) return true;
    size_t n_copies = 1, max_bytes = (size_t)m * sizeof(BalmCutTask);
    for (int i = 0; i < n; ++i) n_copies += deferred[2 * (size_t)i + 1].size();
    if (C.h_cut_copies.ensure(n_copies) != hipSuccess) return false;
    size_t at = 0;
    C.h_cut_copies.p[at++] = CopyTask{C.d_cut_list.p, C.h_cut_list.p, (size_t)m * sizeof(BalmCutTask)};
    for (int i = 0; i < n; ++i) {
        for (const CopyTask& t : deferred[2 * (size_t)i + 1]) { C.h_cut_copies.p[at++] = t; max_bytes = std::max(max_bytes, t.bytes); }
        deferred[2 * (size_t)i + 1].clear();
    }
    launch_copy_tasks(C.h_cut_copies.p, (int)n_copies, max_bytes, st);
    launch_balm_cut(C.d_cut_list.p, m, max_points, max_table, st);
    return hipGetLastError() == hipSuccess;
}
// rc per window (0, or the error of a window whose planes could not be set up)
inline bool plane_extraction_finish(LockstepContext& C, int n, std::vector<int>& rc_lidar, hipStream_t st) {
    bool any = false;
    for (int i = 0; i < n; ++i) any |= C.h_cut.p[i].n_points > 0;
    if (!any) return true;
    if (stream_wait_blocking(st) != hipSuccess) return false;
    for (int i = 0; i < n; ++i) {
        if (C.h_cut.p[i].n_points <= 0 || rc_lidar[i] < 0) continue;
        rc_lidar[i] = C.ws[i]->lidar.finish_cut(st);
    }
    return true;
}

// What the launches of a phase have to cover: the largest sizes among the listed windows and which kernel families they need.  Taken over
// the whole batch once (the fusion switches follow from it) and, with the device-side LM loop, again over the windows still alive whenever that
// list shrinks: the rounds a few stragglers need after the bulk has finished are launched for THEIR sizes and families only (no dense-path
// kernels once the last window of more than 21 free keyframes is done, the narrow solve kernel for narrow systems).
template <typename Win>
BaBatchExtent batch_extent(const std::vector<Win>& W, const std::vector<int>& list, bool* all_block_parts_out = nullptr) {
    BaBatchExtent X{};
    bool all_block_parts = true;
    for (int i : list) {
        if (W[i].rc < 0) continue;
        const BaProblemDev& pb = W[i].vp.pb;
        X.max_edges = std::max(X.max_edges, pb.n_edges); X.max_points = std::max(X.max_points, pb.n_points); X.max_poses = std::max(X.max_poses, pb.n_poses);
        X.max_free = std::max(X.max_free, pb.n_free); X.max_free_edges = std::max(X.max_free_edges, pb.n_free_edges); X.max_groups = std::max(X.max_groups, pb.n_groups);
        if (!(pb.sparse_schur && pb.schur_blocks && pb.n_free > 0 && W[i].vp.n_slices > 0)) all_block_parts = false;
        if (pb.trial_fused) X.any_trial_fused = 1; else X.any_trial_unfused = 1;
        if (pb.n_dups) X.any_dups = 1;
        if (pb.sparse_schur && pb.schur_blocks) {
            if (pb.n_free > 0 && W[i].vp.n_slices > 0) {
                X.min_block_free = X.max_block_parts ? std::min(X.min_block_free, pb.n_free) : pb.n_free;
                X.max_block_parts = std::max(X.max_block_parts, W[i].vp.n_slices); X.max_block_free = std::max(X.max_block_free, pb.n_free);
                X.any_block_lean = 1;
                if (pb.n_free > kSchurBlocksMaxFree) X.any_block_wide = 1;
            }
        } else if (!pb.sparse_schur) {
            X.any_dense = 1; X.max_np_pad = std::max(X.max_np_pad, pb.np_pad); X.max_slices = std::max(X.max_slices, W[i].vp.n_slices);
        }
        if (W[i].lidar) {
            X.max_planes = std::max(X.max_planes, W[i].lidar->n_planes); X.max_chunks = std::max(X.max_chunks, W[i].lidar->dev.n_chunks);
            X.max_W = std::max(X.max_W, W[i].lidar->W);
        }
    }
    if (all_block_parts_out) *all_block_parts_out = all_block_parts;
    return X;
}

// ---- the slot of a window ------------------------------------------------------------------------------------------------------------------
// The table's memory is reused from call to call and from driver to driver (a group's LV and LVI batches, the engine's slots): a slot always
// starts from BaBatchSlot{}, so what a form of the loop does not use is NULL / 0 -- never what an earlier call left (lm, lm_host, stop_host).
// Here: what every form has, in the form whose decisions and reduced systems are the host's (sums and S / b_s to the window's pinned buffers).
template <typename Win>
BaBatchSlot lockstep_slot(const Win& w) {
    BaBatchSlot s{};
    s.pb = w.vp.pb;
    s.n_slices = w.vp.n_slices; s.k_per_slice = w.vp.k_per_slice; s.has_lidar = w.lidar != nullptr;
    double* sc = w.ws->h_scal.p;
    s.chi_out = sc; s.maxdiag_out = sc + 1; s.scale_out = sc + 3; s.chi_trial_out = sc + 4;
    s.S_out = w.ws->h_S.p; s.bs_out = w.ws->h_bs.p; s.xp = w.ws->h_xp.p; s.depth_out = w.ws->d_depth.p;
    if (w.lidar) s.balm = w.lidar->dev;
    return s;
}
// the reduced system solved on the device, the decisions on the host: Schur product, solve and trial in one queue -- S and b_s stay on the
// device, b_p, the step and whether the factorisation went through come back
template <typename Win>
void slot_device_solve(BaBatchSlot& s, const Win& w) {
    s.S_out = w.ws->d_S.p; s.bs_out = w.ws->d_bs.p; s.bp_host = w.ws->h_bs.p + w.vp.np;
    s.xp = s.x_dev = w.ws->d_xp.p; s.x_host = w.ws->h_xp.p; s.ok_host = w.ws->h_ok.p;
}

// ---- what the device-side Levenberg-Marquardt loop's two drivers share (ba_batch_lockstep's device-LM form, tc2li_ba_engine) ----
// The table entry and the initial optimiser state of window w in slot i of context C: everything a phase leaves for the next one stays in
// device memory, the decide kernel mirrors the window's state into C.h_lm[i].  The entry goes up with the caller's next copy launch
// (C.d_table + i), the state from C.h_lm_init[i] to C.d_lm[i].
inline void fill_device_lm_slot(BaBatchSlot& s, const LockstepWindow& w, LockstepContext& C, int i) {
    s = lockstep_slot(w);
    s.lambda_init = w.p->lambda_init; s.iterations = w.p->iterations;
    const size_t nn = (size_t)w.vp.np * w.vp.np;
    double* sc = w.ws->d_scal.p;
    s.chi_out = sc; s.maxdiag_out = sc + 1; s.scale_out = sc + 3; s.chi_trial_out = sc + 4;
    s.S_out = w.ws->d_S.p; s.bs_out = w.ws->d_bs.p; s.xp = s.x_dev = w.ws->d_xp.p;
    s.lm = C.d_lm.p + i; s.lm_host = C.h_lm.p + i; s.stop_host = C.h_stop.p + i; s.ok_host = &s.lm->solve_ok;
    if (w.lidar) {
        s.Hl = w.ws->d_Hl.p; s.bl_lidar = w.ws->d_Hl.p + nn; s.balm.out = w.ws->d_balm_out.p; s.lidar_JH = w.ws->d_lidar_JH.p;
        s.lidar_information = w.lidar->information;
    }
    BaLmState& m = C.h_lm_init.p[i];
    m = BaLmState{};
    m.lambda = -1; m.ni = 2; m.r1 = 1000; m.r2 = 1000; m.is_calc_hess = 1; m.ok = 1; m.solve_ok = 1;
    m.status = w.wants_iteration() ? kLmIterate : kLmDone;
    C.h_lm.p[i] = m;
    C.h_stop.p[i] = 0;
}
// One round of the windows in `live` queued on st as ONE sequence without a host decision in it: linearise (windows whose status is
// kLmIterate) + the plane term + begin, then Schur + solve + trial estimate + errors + decide (windows in kLmTrial).  live_lidar: those of
// `live` with a LiDAR edge; lidar_first: those of them whose plane residual at the current estimate is not in place yet (their first
// linearisation: later the accepted estimate is the last trial, whose residual and decompositions are).
inline void queue_lm_round(const BaBatchSlot* d_table, const std::vector<LockstepWindow>& W, const std::vector<int>& live, const std::vector<int>& live_lidar,
                           const std::vector<int>& lidar_first, const BaBatchExtent& XL, bool want_maxdiag, hipStream_t st) {
    auto pieces_for = [&](const std::vector<int>& list, int expect, auto&& fn) { for_phase_pieces(d_table, (const double*)nullptr, W, list, fn, expect); };
    pieces_for(live, kLmIterate, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_linearize(ph, cnt, XL, want_maxdiag, st); });
    pieces_for(lidar_first, kLmIterate, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, false, st); });
    pieces_for(live_lidar, kLmIterate, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_hessian(ph, cnt, XL, st); });
    pieces_for(live, kLmIterate, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_lm_begin(ph, cnt, st); });
    pieces_for(live, kLmTrial, [&](const BaPhaseHost& ph, int cnt) {
        ba_batch_launch_schur(ph, cnt, XL, st);
        ba_batch_launch_solve(ph, cnt, XL, st);
        ba_batch_launch_trial(ph, cnt, XL, st);
    });
    if (XL.any_trial_unfused) pieces_for(live_lidar, kLmTrial, [&](const BaPhaseHost& ph, int cnt) { balm_batch_launch_residual(ph, cnt, true, st); });  // (windows with pb.trial_fused: inside the trial kernel)
    pieces_for(live, kLmTrial, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_lm_decide(ph, cnt, st); });
}

// ---- a window's results on their way to the caller: [poses | points | per-edge chi2 | depth flags] in ws->h_result (poses: LV windows only) ----
// add(dst, src, bytes) for every piece, from the buffers of pb that hold the accepted estimate
template <typename Win, typename Add>
void queue_result_copies(const Win& w, const BaProblemDev& pb, bool with_poses, Add&& add) {
    const size_t E = pb.n_edges, P = pb.n_points, pose_bytes = with_poses ? pb.n_poses * sizeof(Se3) : 0;
    uint8_t* h = w.ws->h_result.p;
    uint8_t* hc = h + pose_bytes + 3 * P * sizeof(double);
    if (with_poses) add(h, pb.poses, pose_bytes);
    add(h + pose_bytes, pb.points, 3 * P * sizeof(double));
    if (w.p->edge_chi2) add(hc, w.ws->d_chi2.p, E * sizeof(double));
    if (w.p->edge_depth_positive) add(hc + E * sizeof(double), w.ws->d_depth.p, E);
}
inline size_t result_bytes(const BaProblemDev& pb, bool with_poses) {
    return (with_poses ? pb.n_poses * sizeof(Se3) : 0) + 3 * (size_t)pb.n_points * sizeof(double) + (size_t)pb.n_edges * sizeof(double) + (size_t)pb.n_edges;
}
// ... and from there into the caller's arrays (poses: into w.vp.poses and on as poses7 rows)
template <typename Win>
void scatter_results(Win& w, bool with_poses) {
    const auto& p = *w.p;
    const BaProblemDev& pb = w.vp.pb;
    const size_t E = pb.n_edges, P = pb.n_points, pose_bytes = with_poses ? pb.n_poses * sizeof(Se3) : 0;
    const uint8_t* h = w.ws->h_result.p;
    const uint8_t* hc = h + pose_bytes + 3 * P * sizeof(double);
    if (with_poses) memcpy(w.vp.poses.data(), h, pose_bytes);
    memcpy(p.points3, h + pose_bytes, 3 * P * sizeof(double));
    if (p.edge_chi2) memcpy(p.edge_chi2, hc, E * sizeof(double));
    if (p.edge_depth_positive) memcpy(p.edge_depth_positive, hc + E * sizeof(double), E);
}
inline void write_poses7(const std::vector<Se3>& poses, double* poses7) {
    for (size_t k = 0; k < poses.size(); ++k) { memcpy(poses7 + 7 * k, poses[k].q, 4 * sizeof(double)); memcpy(poses7 + 7 * k + 4, poses[k].t, 3 * sizeof(double)); }
}

// ---- one call of a lock-step driver ---------------------------------------------------------------------------------------------------------
// The context of its group, acquired; the slot table (one slot per window, filled once after the setup and uploaded with the windows' input
// blocks; what a phase changes -- which windows take part, lambda, which of a slot's two buffers holds the accepted estimate -- travels in the
// kernels' arguments, BaPhase) and behind it the steps x_p of the windows of a trial phase (kBaXpStride doubles each; a window with more free
// keyframes than that keeps reading the solver's pinned buffer); the extent of the batch; the laps of TC2LI_BA_TIMING.
struct LockstepRun {
    LockstepContext& C;
    WorkerPool& pool;
    const BaOptions opt = BaOptions::read();
    const int n;
    hipStream_t st = nullptr;
    size_t table_bytes = 0;
    BaBatchSlot* h_slots = nullptr;
    const BaBatchSlot* d_table = nullptr;
    double* h_xp_area = nullptr;   // pinned: no upload launch for the steps -- the trial kernels read a window's step (<= 1.5 KB, once per workgroup) from
                                   // here over the bus: ten launches fewer per call at the same speed (BA stage alone 15.3 / 15.4 ms per 128 windows, the loop
                                   // 28.5-28.7 / 28.6-29.1 ms per step against the one-entry k_copy_tasks launch of rounds 3-4)
    std::vector<int> rc_lidar;
    std::vector<std::vector<CopyTask>> deferred;   // what the setup tasks would have queued as copies / fills of their own: two lists per window
    BaBatchExtent X{};
    BaGridTally tally{};   // TC2LI_BA_TIMING: the launch wrappers count workgroups here
    bool failed = false;
    bool sleeping_sync = false;   // device-side LM: the waits are sleeping ones
    double tm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t_begin = 0, t_mark = 0;

    LockstepRun(LockstepContext& C_, WorkerPool& pool_, int n_) : C(C_), pool(pool_), n(n_) {}
    LockstepRun(const LockstepRun&) = delete;
    static double now() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
    void lap(int k) { if (opt.timing) { const double t = now(); tm[k] += t - t_mark; t_mark = t; } }

    // the caller holds C.mu.  false: the batch goes through the one-window path
    bool acquire() {
        if (opt.timing) t_begin = t_mark = now();
        if (!C.st && !create_priority_stream(&C.st)) return false;
        st = C.st;
        while ((int)C.ws.size() < n) C.ws.emplace_back(new BaWorkspace());
        if (n > 65535) return false;  // BaPhase names a window by 16 bits
        table_bytes = (size_t)n * sizeof(BaBatchSlot);
        const size_t xp_bytes = (size_t)n * kBaXpStride * sizeof(double);
        if (C.d_table.ensure(table_bytes) != hipSuccess || C.h_table.ensure(table_bytes + xp_bytes) != hipSuccess || C.h_cut.ensure(std::max(n, 1)) != hipSuccess) return false;
        h_slots = (BaBatchSlot*)C.h_table.p;
        h_xp_area = (double*)(C.h_table.p + table_bytes);
        d_table = (const BaBatchSlot*)C.d_table.p;
        for (int i = 0; i < n; ++i) C.h_cut.p[i].n_points = 0;
        rc_lidar.assign(n, 0);
        deferred.assign(2 * (size_t)n, {});
        return true;
    }
    // (the group's thread spins on its stream between the phases: sleeping on a blocking event instead was measured in round 4 -- the same host
    // CPU time, 13.7 of the 16 CPUs a one-GPU box's cgroup grants, and a step 0.3 ms longer)
    void sync() { if (hipGetLastError() != hipSuccess || (sleeping_sync ? stream_wait_blocking(st) : hipStreamSynchronize(st)) != hipSuccess) failed = true; }
    template <typename Win, typename Fn>
    void pieces(const std::vector<Win>& W, const std::vector<int>& list, const double* xp_area, Fn&& fn) const { for_phase_pieces(d_table, xp_area, W, list, fn); }
};

// a LiDAR window outside the batched kernels' range sends the whole batch through the one-window path
template <typename Problem>
bool lidar_windows_in_range(const Problem* problems, int n) {
    for (int i = 0; i < n; ++i)
        if (problems[i].lidar && problems[i].lidar->n_keyframes > kLockstepMaxLidarKeyframes) return false;
    return true;
}

// The setup in two passes over the windows, setup_task(2 i + 1) = the LiDAR window of window i, setup_task(2 i) = its structure + uploads (each
// under a CopySink on its entry of R.deferred): the plane extraction on the device is queued between the passes and runs while the host builds
// the visual structure.  Then every window has its planes (W[i].lidar) or the error of its LiDAR task.  false: the batch goes through the
// one-window path (an allocation failed, or a window has more planes than the batched LiDAR kernels take).  print_laps: the passes' times on stderr.
template <typename Win, typename Task>
bool lockstep_setup(LockstepRun& R, std::vector<Win>& W, Task&& setup_task, bool print_laps) {
    const int n = R.n;
    auto run = [&](int task) { CopySink sink(&R.deferred[task]); setup_task(task); };
    R.pool.parallel_for(n, [&](int i) { run(2 * i + 1); });
    if (!plane_extraction_begin(R.C, R.deferred, n, R.st)) { (void)hipStreamSynchronize(R.st); return false; }
    if (print_laps) fprintf(stderr, "  lidar tasks + queueing the extraction: %.3f ms\n", R.now() - R.t_begin);
    R.pool.parallel_for(n, [&](int i) { run(2 * i); });
    if (print_laps) fprintf(stderr, "  + visual tasks: %.3f ms\n", R.now() - R.t_begin);
    if (!plane_extraction_finish(R.C, n, R.rc_lidar, R.st)) return false;
    if (print_laps) fprintf(stderr, "  + extraction back: %.3f ms\n", R.now() - R.t_begin);
    for (int i = 0; i < n; ++i) {
        if (W[i].rc < 0 || !W[i].p->lidar) continue;
        if (R.rc_lidar[i] < 0) W[i].rc = R.rc_lidar[i]; else W[i].lidar = &R.C.ws[i]->lidar;
    }
    for (int i = 0; i < n; ++i)
        if (W[i].rc >= 0 && W[i].lidar && W[i].lidar->n_planes > 2048) {  // outside the batched LiDAR kernels: per-window path for this batch
            (void)hipStreamSynchronize(R.st);
            return false;
        }
    return true;
}

// The extent of the whole batch and the fusion switches that follow from it.
template <typename Win>
void lockstep_extent(LockstepRun& R, const std::vector<Win>& W) {
    std::vector<int> all_windows(R.n);
    for (int i = 0; i < R.n; ++i) all_windows[i] = i;
    bool all_block_parts = true;
    R.X = batch_extent(W, all_windows, &all_block_parts);
    R.X.tally = R.opt.timing ? &R.tally : nullptr;
    // The sums behind a trial's errors (k_ba_trial_reduce_b: two workgroups per window) are taken by the LAST workgroup of the window's
    // error pass (a ticket per window, ba_kernels.hip: ba_last_of): one launch fewer per LM trial -- BA stage alone 15.0-15.2 against 15.2-15.6 ms
    // per 128 windows, the loop 28.3 / 28.7 against 28.4 / 28.9 ms.  (The same for the Schur product's closing sums measured SLOWER, 29.5-29.8
    // against 28.4-28.6 ms: one workgroup adding ten parts of 2 700 values is a longer tail than the 21 workgroups of k_ba_schur_finish_b
    // are a launch; removed.)
    R.X.fuse_trial = all_block_parts ? 1 : 0;
    // round 5: the linearisation's closing sums (pose blocks, robust cost, largest diagonals) and the plane Hessian's
    // chunk sums the same way -- an iteration's linearisation phase is then two launches instead of four or five.  Built, bit-identical
    // (the same sums in the same order), and measured in the whole loop, three A/B pairs in one call: 26.24 / 26.26 / 26.27 ms per step fused
    // against 26.08 / 25.95 / 26.03 separate (mapping workers 25.1-25.7 against 24.5-25.3): the loop is bound by the kernels' combined
    // throughput, not by the number of launches in a chain, and one workgroup's tail is longer than the small launch it replaces.  Off by
    // default; TC2LI_BA_FUSE_LIN=1 (read per call) switches it on.
    R.X.fuse_linearize = R.opt.fuse_linearize ? 1 : 0;
}

// The table (slot i from fill_slot(i) for the windows that were set up, empty for the others) and everything the setup deferred (uploads, operand
// fills) in one launch; the windows' megabyte input blocks go through the copy engines (launch_copy_tasks).  extra: one more copy of that
// launch (the device-side LM states), or NULL.
template <typename Win, typename Fill>
bool lockstep_upload(LockstepRun& R, const std::vector<Win>& W, Fill&& fill_slot, const CopyTask* extra = nullptr) {
    LockstepContext& C = R.C;
    for (int i = 0; i < R.n; ++i)
        if (W[i].rc >= 0) R.h_slots[i] = fill_slot(i); else R.h_slots[i] = BaBatchSlot{};
    size_t n_tasks = extra ? 2 : 1, max_bytes = std::max(R.table_bytes, extra ? extra->bytes : (size_t)0);
    for (const auto& d : R.deferred) n_tasks += d.size();
    if (C.h_tasks.ensure(n_tasks) != hipSuccess) return false;
    size_t at = 0;
    C.h_tasks.p[at++] = CopyTask{C.d_table.p, C.h_table.p, R.table_bytes};
    if (extra) C.h_tasks.p[at++] = *extra;
    for (const auto& d : R.deferred) for (const CopyTask& t : d) { C.h_tasks.p[at++] = t; max_bytes = std::max(max_bytes, t.bytes); }
    launch_copy_tasks(C.h_tasks.p, (int)n_tasks, max_bytes, R.st);
    return true;
}

// the steps of a trial phase: window k of `step` at h_xp_area + k * kBaXpStride, where the trial kernels read them
template <typename Win>
void stage_steps(LockstepRun& R, const std::vector<Win>& W, const std::vector<int>& step) {
    for (size_t k = 0; k < step.size(); ++k) {
        const Win& w = W[step[k]];
        if (w.vp.np <= 0 || w.vp.np > kBaXpStride) continue;
        memcpy(R.h_xp_area + k * kBaXpStride, w.ws->h_xp.p, (size_t)w.vp.np * sizeof(double));
    }
}

// The depth flags, then device -> pinned staging: one launch writes every window's results (the setup's copy list is done with: the stream
// has been synchronised many times since); also_queue() may add launches behind it; then the copies into the caller's arrays run in parallel,
// scatter(w) after the common ones of window w.
template <typename Win, typename Queue, typename Scatter>
void lockstep_results(LockstepRun& R, std::vector<Win>& W, bool with_poses, Queue&& also_queue, Scatter&& scatter) {
    LockstepContext& C = R.C;
    std::vector<int> all;
    for (int i = 0; i < R.n; ++i) if (W[i].rc >= 0) all.push_back(i);
    if (R.failed || all.empty()) return;
    R.pieces(W, all, nullptr, [&](const BaPhaseHost& ph, int cnt) { ba_batch_launch_depth(ph, cnt, R.X, R.st); });
    size_t n_tasks = 0, max_bytes = 0;
    if (C.h_tasks.ensure(4 * all.size()) != hipSuccess) R.failed = true;
    for (int i : all) {
        if (R.failed) break;
        Win& w = W[i];
        if (w.ws->h_result.ensure(result_bytes(w.vp.pb, with_poses)) != hipSuccess) { R.failed = true; break; }
        queue_result_copies(w, w.vp.pb, with_poses, [&](void* dst, const void* src, size_t nbytes) { C.h_tasks.p[n_tasks++] = CopyTask{dst, src, nbytes}; max_bytes = std::max(max_bytes, nbytes); });
    }
    if (!R.failed) launch_copy_tasks(C.h_tasks.p, (int)n_tasks, max_bytes, R.st);
    if (!R.failed) also_queue(all);
    R.sync();
    if (!R.failed)
        R.pool.parallel_for((int)all.size(), [&](int k) {
            Win& w = W[all[k]];
            scatter_results(w, with_poses);
            scatter(w);
        });
}

// results[i] and the statistics of the windows: the error of a window's setup, TC2LI_ERR_HIP for all after a HIP error in the loop (entry: the
// entry point's name for the message), or the iterations done; also(w) after the common statistics of a window that succeeded
template <typename Win, typename Also>
void lockstep_write_stats(const LockstepRun& R, std::vector<Win>& W, const char* entry, int32_t* results, Also&& also) {
    for (int i = 0; i < R.n; ++i) {
        Win& w = W[i];
        if (w.rc < 0) { results[i] = w.rc; continue; }
        if (R.failed) { set_error("%s: HIP error in the lock-step loop: %s", entry, hipGetErrorString(hipGetLastError())); results[i] = TC2LI_ERR_HIP; continue; }
        const auto& p = *w.p;
        if (p.stats) { p.stats->iterations = w.lm.done; p.stats->trials = w.lm.trials_total; p.stats->n_free_poses = w.vp.n_free; }
        if (w.lidar && p.lidar_stats) write_lidar_stats(*w.lidar, p.lidar_stats);
        also(w);
        results[i] = w.lm.done;
    }
}

// the lock-step drivers (ba_lockstep.cpp, lvi_host.cpp): false = the batch goes through the one-window path
// prepared: NULL, or one record per window (a window with sizes.n_poses == 0 in it is set up from its host arrays as ever)
bool ba_batch_lockstep(const tc2li_ba_problem* problems, int n, const tc2li_camera* cam, WorkerPool& pool, int32_t* results, int group = 0,
                       const BaPrepared* prepared = nullptr);

}  // namespace ba_detail
}  // namespace tc2li

// Internal to the bundle-adjustment host code (ba_host.cpp, ba_lockstep.cpp, ba_engine.cpp, lvi_host.cpp): the options, the per-thread and
// per-window work spaces, the visual problem's structure and the inertial term (what the lock-step drivers share: lockstep_host.hpp).  Not part of the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <limits>
#include <map>
#include <mutex>
#include <thread>
#include <pthread.h>
#include "common.hpp"
#include "ba_device.hpp"
#include "ba_structure.hpp"
#include "ba_structure_device.hpp"
#include "balm_host.hpp"
#include "inertial_host.hpp"
#include "reduced_solve.hpp"
#include "pose_opt_device.hpp"

namespace tc2li {
namespace ba_detail {


// The environment switches of the bundle-adjustment entry points, parsed in ONE place at the start of every call (the tests flip some of
// them between two calls of one process) and reported by tc2li_ba_options (bench.py logs it in its detail file).  Round 6 retired the
// switches whose A/B measurements are in DESIGN.md and whose losing form was only kept as a fall-back: TC2LI_BA_SCHUR_LEAN / _MFMA / _GROUP
// (the lean Schur product is the only block-by-block form), TC2LI_BA_FUSE, TC2LI_BA_XP_PINNED, TC2LI_BA_PRE_SCHUR, TC2LI_BA_PHASE_SERIAL,
// TC2LI_BA_DENSE_SLICES.
struct BaOptions {
    bool device_lm = true;        // TC2LI_BA_DEVICE_LM=0: the LM decisions on the host between the phases (rounds 2-5)
    bool device_solve = false;    // TC2LI_BA_DEVICE_SOLVE=1: host-driven loop with the reduced systems solved by k_ba_solve_b
    bool fuse_linearize = false;  // TC2LI_BA_FUSE_LIN=1: the linearisation's closing sums by the window's last workgroup
    bool fuse_trial = false;      // TC2LI_BA_FUSE_TRIAL=1: a trial as one launch over the landmark groups (pb.trial_fused)
    bool lvi_device_solve = true; // TC2LI_LVI_DEVICE_SOLVE=0: the inertial windows' reduced systems on the host's envelope solver
    bool lockstep = true;         // TC2LI_BA_NO_LOCKSTEP: every window through the one-window path
    bool timing = false;          // TC2LI_BA_TIMING: per-call laps on stderr
    int groups = 3;               // TC2LI_BA_LOCKSTEP_GROUPS: lock-step groups of the batch entry points
    std::string shard_fail;       // TC2LI_TEST_SHARD_FAIL: "<rank>:setup" / "<rank>:trial" (tests of the sharded window's failure protocol)
    static BaOptions read() {
        auto flag = [](const char* name, bool dflt) { const char* e = getenv(name); return e ? atoi(e) != 0 : dflt; };
        BaOptions o;
        o.device_lm = flag("TC2LI_BA_DEVICE_LM", true); o.device_solve = flag("TC2LI_BA_DEVICE_SOLVE", false);
        o.fuse_linearize = flag("TC2LI_BA_FUSE_LIN", false); o.fuse_trial = flag("TC2LI_BA_FUSE_TRIAL", false);
        o.lvi_device_solve = flag("TC2LI_LVI_DEVICE_SOLVE", true);
        o.lockstep = getenv("TC2LI_BA_NO_LOCKSTEP") == nullptr; o.timing = getenv("TC2LI_BA_TIMING") != nullptr;
        if (const char* e = getenv("TC2LI_BA_LOCKSTEP_GROUPS")) o.groups = atoi(e);
        o.groups = std::max(1, std::min(kMaxLockstepGroups, o.groups));
        if (const char* e = getenv("TC2LI_TEST_SHARD_FAIL")) o.shard_fail = e;
        return o;
    }
};

// result of a window a lock-step group hands back to the one-window path (never seen by a caller: the batch entry points run that path at once)
constexpr int kLockstepDeclined = -1000000;

struct PoseOptWorkspace {
    DevBuf<PoseProblem> d_probs;
    DevBuf<double> d_Xw, d_poses, d_chi2;
    DevBuf<BaEdge> d_edges;
    DevBuf<uint8_t> d_outlier;
    DevBuf<int> d_inliers, d_exact;  // d_exact [1]: launch_pose_inputs_float_exact's answer
    std::mutex mu;
};
inline PoseOptWorkspace& po_ws() { static thread_local PoseOptWorkspace w; return w; }

// The inertial reduced system on its way to the device solve (k_lvi_solve*, ba_kernels.hip): one blob per window and linearisation --
// [first n | rowoff n + 1] ints, then [bi n | the envelope's entries] doubles -- and the kernel's scratch.
struct LviSolveBuffers {
    DevBuf<uint8_t> d_blob;
    PinnedBuf<uint8_t> h_blob;
    DevBuf<double> d_LB, d_Lband;
    size_t ints_bytes = 0;
    LviSolveDev dev{};
    hipError_t ensure(int np, int ni) {
        const size_t n = (size_t)np + ni;
        ints_bytes = ((n + 2 * (size_t)np + 1) * sizeof(int32_t) + 15) / 16 * 16;
        const size_t max_pose = (size_t)np * ni + (size_t)np * (np + 1) / 2;  // pose rows against the band (worst case: every column), pose block
        const size_t bytes = ints_bytes + (n + (size_t)ni * 32 + max_pose) * sizeof(double);
        hipError_t e;
        if ((e = d_blob.ensure(bytes)) != hipSuccess || (e = h_blob.ensure(bytes)) != hipSuccess || (e = d_LB.ensure(std::max<size_t>((size_t)ni * np, 1))) != hipSuccess ||
            (e = d_Lband.ensure(std::max<size_t>((size_t)ni * 32, 1))) != hipSuccess) return e;
        dev.n = (int32_t)n; dev.np = np; dev.ni = ni; dev.pad_ = 0;
        dev.first = reinterpret_cast<const int32_t*>(d_blob.p);
        dev.span_end = dev.first + n;
        dev.rowoff = dev.span_end + np;
        dev.bi = reinterpret_cast<const double*>(d_blob.p + ints_bytes);
        dev.hband = dev.bi + n;
        dev.hpose = dev.hband + (size_t)ni * 32;
        dev.LB = d_LB.p; dev.Lband = d_Lband.p;
        return hipSuccess;
    }
    // after ReducedSolver::set_pattern: the blob of this linearisation; returns the bytes to copy (h_blob -> d_blob)
    size_t pack(const ReducedSolver& rs, const double* Hi, const double* bi) {
        const size_t n = (size_t)rs.n;
        int32_t* ints = reinterpret_cast<int32_t*>(h_blob.p);
        double* dbl = reinterpret_cast<double*>(h_blob.p + ints_bytes);
        memcpy(ints, rs.first.data(), n * sizeof(int32_t));
        memcpy(dbl, bi, n * sizeof(double));
        std::vector<int32_t> span_first(std::max(rs.np, 1));  // (= first[ni + r]: already in the blob)
        const size_t entries = rs.pack_for_device(Hi, span_first.data(), ints + n, ints + n + rs.np, dbl + n, dbl + n + (size_t)rs.ni * 32);
        return ints_bytes + (n + (size_t)rs.ni * 32 + entries) * sizeof(double);
    }
};
struct BaWorkspace {
    LviSolveBuffers lvi;
    DevBuf<Se3> d_poses, d_poses_trial;  // d_poses: tc2li_lidar_window_evaluate only; a window's poses live in d_in
    DevBuf<double> d_points_trial, d_chi2, d_rho0, d_cp, d_W, d_Hll, d_bl, d_diag_l, d_Hpp, d_diag_p,
        d_coef_e, d_coef, d_Y, d_Spart, d_scale_part, d_chi_part, d_red;
    // the window as the caller hands it over -- poses, points, edges and the index arrays -- goes up in ONE copy: a stream operation
    // costs about as much as one of the loop's kernels, and a batch has one such set per window
    DevBuf<uint8_t> d_in;
    PinnedBuf<uint8_t> h_in;
    DevBuf<uint8_t> d_depth;
    PinnedBuf<double> h_S, h_bs, h_xp, h_scal, h_Hpp, h_stat;
    DevBuf<ImuPose> d_iposes, d_iposes_trial;
    PinnedBuf<ImuPose> h_iposes, h_iposes_up;  // trial states on their way back; the initial states on their way up (lock-step batch)
    PinnedBuf<uint8_t> h_result;  // lock-step batch: poses, points, per-edge chi2 and depth flags on their way to the caller
    // lock-step batch with the reduced system solved on the device: S, [b_s | b_p], the step; the LiDAR term's Hessian | gradient on both sides
    DevBuf<double> d_S, d_bs, d_xp, d_Hl;
    // device-side LM (round 6): the kernels' scalar sums, the LiDAR term's output record and its camera-se3 Jacobian / Hessian stay in device memory
    DevBuf<double> d_scal, d_balm_out, d_lidar_JH;
    PinnedBuf<double> h_Hl;
    PinnedBuf<int32_t> h_ok;
    BalmTerm lidar;
    std::mutex mu;
};
// one workspace per host thread: windows optimised from different threads (tc2li_local_bundle_adjustment_batch) do not
// share device buffers
inline BaWorkspace& ba_ws() { static thread_local BaWorkspace w; return w; }

// A window whose structure the device built (tc2li_ba_window_solve_batch): its sizes, the downloaded numbering of the poses, and where the
// pieces of its input block lie in device memory -- poses as poses7 rows (the layout of Se3), edges as tc2li_ba_edge (the layout of BaEdge).
// After the BA the lock-step batch evaluates the outlier rule of OptimizerWithLidar.cc:402-449 for it on the device: erase_pose /
// erase_point [erase_capacity] and n_erase are pinned host memory.
struct BaPrepared {
    BaStructureSizes sizes;
    const int32_t* pose_var_host = nullptr;
    const void *poses = nullptr, *points = nullptr, *edges = nullptr, *pose_var = nullptr, *pt_off = nullptr, *pt_edges = nullptr, *pv_off = nullptr,
               *fl_off = nullptr, *fl_pose = nullptr, *fl_lm = nullptr, *fl_place = nullptr, *slice_off = nullptr, *fl_edge = nullptr, *grp_k0 = nullptr,
               *grp_l0 = nullptr, *blk_off = nullptr, *blk_rows = nullptr;
    int32_t *erase_pose = nullptr, *erase_point = nullptr, *n_erase = nullptr;
    int32_t erase_capacity = 0;
    // tc2li_ba_window_solve_graph_commit_batch, which goes on from the device copy of the result after the batch has returned and the
    // windows' workspaces belong to the next caller of the group: with write_back the final estimate is also copied over `poses` and
    // `points` (device to device; they are the caller's to write), and with erase_dev the outlier rule is evaluated a second time into
    // device memory, laid out as the pinned block: [n_erase | 3 words | erase_pose | erase_point], each list erase_capacity long.
    bool write_back = false;
    int32_t* erase_dev = nullptr;
};

// Structure and device state of the projection-edge part of a local BA (shared by the visual / LiDAR and the inertial
// entry points): free-pose numbering, CSR of the edges by landmark and by free pose, workspace sizing, uploads, and the
// BaProblemDev handed to the kernels.  poses7 == NULL: the caller uploads ImuPose states itself (inertial mode).
struct VisualProblem {
    BaProblemDev pb{};
    std::vector<int> pose_var;
    std::vector<Se3> poses;
    int n_free = 0, np = 0, n_slices = 1, k_per_slice = 4;
    int max_group_landmarks = 0;
    // pb.trial_fused (ba_device.hpp): whether the window's trials run as the one fused launch -- a property of the window (it fixes the order
    // of two sums), decided here and again by a caller that switches the vertices to ImuCamPose records.  OFF unless TC2LI_BA_FUSE_TRIAL=1:
    // built for VERDICT r4 item 2 ("a trial <= 3 launches"), parity-green in both forms (tests/test_ba_gpu.py, test_balm_gpu.py,
    // test_inertial_ba_gpu.py run whichever the environment selects) and measured SLOWER in the whole loop -- 27.1 / 27.3 ms per step against
    // 26.1 / 25.8 in two A/B pairs of one call, the camera threads 26.6-27.3 against 25.4-26.1; local BA alone 13.0-13.7 against 12.1-13.9 ms
    // per 128 windows.  A workgroup of the fused launch runs six dependent trips to memory (step, poses, slots, W blocks, edge list, edges)
    // while it holds 28 KB of LDS; the three launches it replaces are thin kernels of two or three trips each that start and finish quickly
    // beside the other stages' wavefronts.  In a loop bound by the kernels' combined occupancy, fewer launches is not the lever; shorter
    // residency is.
    void decide_trial_fused() {
        const size_t pose_bytes = (size_t)pb.n_poses * (pb.inertial ? sizeof(ImuPose) : sizeof(Se3));
        pb.trial_fused = BaOptions::read().fuse_trial && np <= kBacksubMaxNp && pose_bytes <= (size_t)kTrialPoseBytes && max_group_landmarks <= 256 ? 1 : 0;
    }

    // The workspace of a window of these sizes: a per-thread workspace that only grows (hipMalloc per call would dominate the run time).
    int reserve(BaWorkspace& ws, const BaStructureSizes& s) {
    const int n_poses = s.n_poses, n_free_edges = s.n_free_edges, n_blocks = s.n_blocks, n_groups = s.n_groups, np_pad = s.np_pad;
    const bool sparse = s.sparse != 0;
    auto& d_poses_trial = ws.d_poses_trial;
    auto &d_points_trial = ws.d_points_trial, &d_chi2 = ws.d_chi2, &d_rho0 = ws.d_rho0,
         &d_cp = ws.d_cp, &d_W = ws.d_W, &d_Hll = ws.d_Hll, &d_bl = ws.d_bl, &d_diag_l = ws.d_diag_l, &d_Hpp = ws.d_Hpp,
         &d_diag_p = ws.d_diag_p, &d_coef_e = ws.d_coef_e, &d_coef = ws.d_coef,
         &d_Spart = ws.d_Spart, &d_scale_part = ws.d_scale_part, &d_chi_part = ws.d_chi_part;
    auto& d_depth = ws.d_depth;
    auto &h_S = ws.h_S, &h_bs = ws.h_bs, &h_xp = ws.h_xp, &h_scal = ws.h_scal;
    const size_t E = s.n_edges, P = s.n_points;
    TC2LI_HIP_CHECK(d_poses_trial.ensure(n_poses));
    TC2LI_HIP_CHECK(d_points_trial.ensure(3 * P));
    TC2LI_HIP_CHECK(d_chi2.ensure(E)); TC2LI_HIP_CHECK(d_rho0.ensure(E)); TC2LI_HIP_CHECK(d_cp.ensure(kContribP * (size_t)std::max(n_blocks * n_free, 1)));
    TC2LI_HIP_CHECK(d_W.ensure(18 * (size_t)std::max(n_free_edges, 1))); TC2LI_HIP_CHECK(d_Hll.ensure(6 * P)); TC2LI_HIP_CHECK(d_bl.ensure(3 * P)); TC2LI_HIP_CHECK(d_diag_l.ensure(P));
    TC2LI_HIP_CHECK(d_Hpp.ensure(27 * (size_t)std::max(n_free, 1))); TC2LI_HIP_CHECK(d_diag_p.ensure(std::max(n_free, 1)));
    if (!sparse) { TC2LI_HIP_CHECK(d_coef_e.ensure(6 * E)); TC2LI_HIP_CHECK(ws.d_Y.ensure(18 * (size_t)std::max(n_free_edges, 1))); }
    TC2LI_HIP_CHECK(d_coef.ensure(6 * (size_t)std::max(n_free, 1)));
    TC2LI_HIP_CHECK(d_Spart.ensure((size_t)std::max(n_slices, 1) * np_pad * np_pad)); TC2LI_HIP_CHECK(d_scale_part.ensure(P / 256 + 1)); TC2LI_HIP_CHECK(d_chi_part.ensure(std::max(E / 256 + 1, (size_t)n_groups)));
    TC2LI_HIP_CHECK(d_depth.ensure(E));
    TC2LI_HIP_CHECK(h_S.ensure((size_t)std::max(np * np, 1))); TC2LI_HIP_CHECK(h_bs.ensure(2 * (size_t)std::max(np, 1)));
    TC2LI_HIP_CHECK(h_xp.ensure(std::max(np, 1))); TC2LI_HIP_CHECK(h_scal.ensure(8));
    memset(h_S.p, 0, (size_t)std::max(np * np, 1) * sizeof(double));  // the finish kernel writes the lower triangle only; the rest stays defined
        return TC2LI_OK;
    }
    // pb: the sizes, the parts of the input block in ws.d_in (lay), the workspace of reserve()
    void fill_pb(BaWorkspace& ws, const BaStructureSizes& s, const BaInputLayout& lay, const tc2li_camera* cam) {
    uint8_t* const d = ws.d_in.p;
    const bool sparse = s.sparse != 0;
    pb = BaProblemDev{};
    pb.n_edges = s.n_edges; pb.n_points = s.n_points; pb.n_poses = s.n_poses; pb.n_free = n_free; pb.n_free_edges = s.n_free_edges; pb.np_pad = s.np_pad;
    memcpy(&pb.cam, cam, sizeof(CameraD));
    const float dm = sqrtf(5.991f), ds = sqrtf(7.815f);  // thHuberMono / thHuberStereo are floats (OptimizerWithLidar.cc:219-220)
    pb.delta_mono = dm; pb.delta_stereo = ds;
    pb.dsqr_mono = (float)((double)dm * (double)dm); pb.dsqr_stereo = (float)((double)ds * (double)ds);
    pb.poses = (Se3*)(d + lay.o_poses); pb.poses_trial = ws.d_poses_trial.p; pb.points = (double*)(d + lay.o_points); pb.points_trial = ws.d_points_trial.p;
    pb.edges = (const BaEdge*)(d + lay.o_edges); pb.pose_var = (const int*)(d + lay.o_pose_var); pb.pt_off = (const int*)(d + lay.o_pt_off);
    pb.pt_edges = (const int*)(d + lay.o_pt_edges); pb.pv_off = (const int*)(d + lay.o_pv_off); pb.pv_edges = (const int*)(d + lay.o_pv_edges);
    pb.fl_off = (const int*)(d + lay.o_fl_off); pb.fl_pose = (const int*)(d + lay.o_fl_pose); pb.chunk_mask = (const uint32_t*)(d + lay.o_w_slot);
    pb.fl_lm = (const int*)(d + lay.o_fl_lm); pb.fl_place = (const int*)(d + lay.o_fl_place); pb.slice_off = (const int*)(d + lay.o_slice_off); pb.fl_edge = (const int*)(d + lay.o_fl_edge);
    pb.grp_k0 = (const int*)(d + lay.o_grp_k0); pb.grp_l0 = (const int*)(d + lay.o_grp_l0); pb.n_groups = s.n_groups;
    pb.blk_off = (const int*)(d + lay.o_blk_off); pb.blk_rows = (const uint8_t*)(d + lay.o_blk_rows);
    pb.ticket = (int32_t*)(d + lay.o_ticket);
    pb.n_dups = s.n_dups;
    pb.dup_off = !s.n_dups ? nullptr : (const int*)(d + lay.o_dup_off);
    pb.dup_edge = !s.n_dups ? nullptr : (const int*)(d + lay.o_dup_edge);
    pb.dup_slot = !s.n_dups ? nullptr : (const int*)(d + lay.o_dup_slot);
    pb.sparse_schur = sparse ? 1 : 0; pb.schur_blocks = sparse ? 2 : 0; pb.schur_group = s.schur_group; pb.n_schur_slices = s.n_schur_slices;  // (dense windows: the chunks of d_ba_schur_units)
    pb.schur_rd = s.schur_rd; pb.schur_ro = s.schur_ro;
    decide_trial_fused();
    pb.chi2 = ws.d_chi2.p; pb.rho0 = ws.d_rho0.p; pb.cp_part = ws.d_cp.p; pb.W = ws.d_W.p; pb.Hll = ws.d_Hll.p; pb.bl = ws.d_bl.p;
    pb.diag_l = ws.d_diag_l.p; pb.Hpp = ws.d_Hpp.p; pb.diag_p = ws.d_diag_p.p; pb.coef_e = ws.d_coef_e.p; pb.coef = ws.d_coef.p; pb.Y = sparse ? nullptr : ws.d_Y.p;
    pb.S_part = ws.d_Spart.p; pb.scale_part = ws.d_scale_part.p; pb.chi_part = ws.d_chi_part.p;
    }

    int setup(BaWorkspace& ws, const double* poses7, const uint8_t* fixed, int n_poses, const double* points3, int n_points,
              const tc2li_ba_edge* edges, int n_edges, const tc2li_camera* cam, const uint8_t* extra_used, hipStream_t st) {
    // ---- structure: free-pose numbering, CSR by landmark and by free pose, slots, slices, blocks, groups (ba_structure.hpp) ----
    BaStructure s;
    {
        const int rc = ba_build_structure(fixed, n_poses, n_points, edges, n_edges, extra_used, s);
        if (rc != TC2LI_OK) return rc;
    }
    pose_var = s.pose_var;
    n_free = s.n_free; np = s.np; n_slices = s.n_slices; k_per_slice = s.k_per_slice; max_group_landmarks = s.max_group_landmarks;
    const bool sparse = s.sparse != 0;
    const size_t E = n_edges, P = n_points;
    // ---- device memory ----
    {
        const int rc = reserve(ws, s);
        if (rc != TC2LI_OK) return rc;
    }
    // ---- the input block (ba_input_layout, ba_structure.hpp), every part 16-byte aligned ----
    const BaInputLayout lay = ba_input_layout(s);
    TC2LI_HIP_CHECK(ws.d_in.ensure(lay.in_bytes)); TC2LI_HIP_CHECK(ws.h_in.ensure(lay.in_bytes));
    uint8_t* const h = ws.h_in.p;
    if (poses7) {
        poses.resize(n_poses);
        for (int k = 0; k < n_poses; ++k) { memcpy(poses[k].q, poses7 + 7 * k, 4 * sizeof(double)); memcpy(poses[k].t, poses7 + 7 * k + 4, 3 * sizeof(double)); }
        memcpy(h + lay.o_poses, poses.data(), n_poses * sizeof(Se3));
    }
    memcpy(h + lay.o_points, points3, 3 * P * sizeof(double));
    memcpy(h + lay.o_edges, edges, E * sizeof(BaEdge));
    memcpy(h + lay.o_pose_var, pose_var.data(), n_poses * sizeof(int));
    memcpy(h + lay.o_pt_off, s.pt_off.data(), (P + 1) * sizeof(int));
    memcpy(h + lay.o_pt_edges, s.pt_edges.data(), E * sizeof(int));
    memcpy(h + lay.o_pv_off, s.pv_off.data(), (n_free + 1) * sizeof(int));
    if (!sparse) memcpy(h + lay.o_pv_edges, s.pv_edges.data(), s.pv_edges.size() * sizeof(int));  // pv_edges, w_slot: the dense Schur path's
    memcpy(h + lay.o_fl_off, s.fl_off.data(), 2 * P * sizeof(int));
    memcpy(h + lay.o_fl_pose, s.fl_pose.data(), s.fl_pose.size() * sizeof(int));
    if (!sparse) memcpy(h + lay.o_w_slot, s.chunk_mask.data(), s.chunk_mask.size() * sizeof(uint32_t));  // (the region held w_slot for the dense form's prepare kernel)
    memcpy(h + lay.o_fl_lm, s.fl_lm.data(), s.fl_lm.size() * sizeof(int));
    memcpy(h + lay.o_fl_place, s.fl_place.data(), s.fl_place.size() * sizeof(int));
    memcpy(h + lay.o_slice_off, s.slice_off.data(), s.slice_off.size() * sizeof(int));
    memcpy(h + lay.o_fl_edge, s.fl_edge.data(), s.fl_edge.size() * sizeof(int));
    memcpy(h + lay.o_grp_k0, s.grp_k0.data(), s.grp_k0.size() * sizeof(int));
    memcpy(h + lay.o_grp_l0, s.grp_l0.data(), s.grp_l0.size() * sizeof(int));
    memcpy(h + lay.o_blk_off, s.blk_off.data(), s.blk_off.size() * sizeof(int));
    memcpy(h + lay.o_blk_rows, s.blk_rows.data(), s.blk_rows.size());
    memset(h + lay.o_ticket, 0, 4 * sizeof(int32_t));  // (the kernels that use them leave them at zero again)
    if (s.n_dups) {
        memcpy(h + lay.o_dup_off, s.dup_off.data(), s.dup_off.size() * sizeof(int));
        memcpy(h + lay.o_dup_edge, s.dup_edge.data(), (size_t)s.n_dups * sizeof(int));
        memcpy(h + lay.o_dup_slot, s.dup_slot.data(), (size_t)s.n_dups * sizeof(int));
    }
    // inertial mode (poses7 == NULL) uploads ImuPose states itself and does not read the Se3 block
    const size_t first = poses7 ? 0 : lay.o_points;
    TC2LI_HIP_CHECK(upload_or_defer(ws.d_in.p + first, h + first, lay.in_bytes - first, st));  // h is pinned
    fill_pb(ws, s, lay, cam);
        return TC2LI_OK;
    }

    // The same state for a window whose structure was built on the device (ba_structure_kernels.hip): the workspace from the sizes, the
    // input block filled device to device from the pieces, no structure on the host and no upload.  pose_var_host [n_poses] is the
    // downloaded numbering (the LiDAR term's host steps read it).
    int adopt(BaWorkspace& ws, const BaPrepared& pr, const tc2li_camera* cam, hipStream_t st) {
    const BaStructureSizes& s = pr.sizes;
    pose_var.assign(pr.pose_var_host, pr.pose_var_host + s.n_poses);
    poses.resize(s.n_poses);
    n_free = s.n_free; np = s.np; n_slices = s.n_slices; k_per_slice = s.k_per_slice; max_group_landmarks = s.max_group_landmarks;
    {
        const int rc = reserve(ws, s);
        if (rc != TC2LI_OK) return rc;
    }
    const BaInputLayout lay = ba_input_layout(s);
    TC2LI_HIP_CHECK(ws.d_in.ensure(lay.in_bytes));
    uint8_t* const d = ws.d_in.p;
    const size_t K = s.n_poses, P = s.n_points, E = s.n_edges, F = s.n_free_edges;
    const struct { size_t at; const void* src; size_t bytes; } piece[] = {
        {lay.o_poses, pr.poses, K * sizeof(Se3)}, {lay.o_points, pr.points, 3 * P * sizeof(double)}, {lay.o_edges, pr.edges, E * sizeof(BaEdge)},
        {lay.o_pose_var, pr.pose_var, K * 4}, {lay.o_pt_off, pr.pt_off, (P + 1) * 4}, {lay.o_pt_edges, pr.pt_edges, E * 4},
        {lay.o_pv_off, pr.pv_off, ((size_t)s.n_free + 1) * 4}, {lay.o_fl_off, pr.fl_off, 2 * P * 4}, {lay.o_fl_pose, pr.fl_pose, F * 4},
        {lay.o_fl_lm, pr.fl_lm, F * 4}, {lay.o_fl_place, pr.fl_place, F * 4}, {lay.o_slice_off, pr.slice_off, lay.n_slice_off * 4},
        {lay.o_fl_edge, pr.fl_edge, F * 4}, {lay.o_grp_k0, pr.grp_k0, lay.n_grp * 4}, {lay.o_grp_l0, pr.grp_l0, lay.n_grp * 4},
        {lay.o_blk_off, pr.blk_off, lay.n_blk_off * 4}, {lay.o_blk_rows, pr.blk_rows, lay.n_blk_rows}};
    for (const auto& q : piece) {
        if (!q.bytes) continue;
        // device to device: the batch's copy kernel takes any global pointer; without a batch, the runtime's copy
        if (copy_sink_active()) { TC2LI_HIP_CHECK(upload_or_defer(d + q.at, q.src, q.bytes, st)); }
        else { TC2LI_HIP_CHECK(hipMemcpyAsync(d + q.at, q.src, q.bytes, hipMemcpyDeviceToDevice, st)); }
    }
    TC2LI_HIP_CHECK(zero_or_defer(d + lay.o_ticket, 4 * sizeof(int32_t), st));
    fill_pb(ws, s, lay, cam);
        return TC2LI_OK;
    }
};


// The inertial edges of a window (EdgeInertial + EdgeGyroRW + EdgeAccRW per link, SF/src/OptimizerWithLidar.cc:729-800) on the host:
// their robust cost at a state and, when asked, their dense normal equations in the numbering [6 per free pose | 9 per free
// keyframe with IMU state].  Shared by the one-window entry point and the lock-step batch.
struct InertialTerm {
    std::vector<InertialLinkHost> L;
    std::vector<int> imu_var;
    const std::vector<int>* pose_var = nullptr;
    int np = 0, n = 0, n_imu = 0;
    std::vector<double> Hi, bi;
    // The row segments of Hi a linearisation writes (the blocks of the inertial edges; the caller adds those of the LiDAR term): from the second
    // linearisation on only they are cleared -- Hi is n x n (1.1 MB at 375 unknowns) and almost empty, and clearing it whole was half of what
    // the inertial edges of a window cost the host.
    std::vector<uint32_t> seg_at;
    std::vector<uint8_t> seg_len;
    bool segs_ready = false;
    void note_segment(size_t at, int len) {  // (a length is a byte: longer runs are recorded in pieces)
        if (segs_ready) return;
        for (; len > 0; at += 255, len -= 255) { seg_at.push_back((uint32_t)at); seg_len.push_back((uint8_t)std::min(len, 255)); }
    }
    void note_block(int row0, int col0, int rows, int cols) { for (int r = 0; r < rows; ++r) note_segment((size_t)(row0 + r) * n + col0, cols); }
    double d_imu = 0;
    float dsqr_imu = 0;

    // links -> L; extra_used / imu_used [n_kfs]: keyframes an inertial edge touches
    int prepare(const tc2li_inertial_link* links, int n_links, const uint8_t* has_imu, int n_kfs, std::vector<uint8_t>& extra_used) {
        L.resize(n_links);
        extra_used.assign(n_kfs, 0);
        for (int l = 0; l < n_links; ++l) {
            const tc2li_inertial_link& in = links[l];
            if (in.kf1 < 0 || in.kf1 >= n_kfs || in.kf2 < 0 || in.kf2 >= n_kfs || !in.preintegrated) { set_error("inertial link %d: invalid keyframe index or null pre-integration", l); return TC2LI_ERR_INVALID; }
            if (!has_imu[in.kf1] || !has_imu[in.kf2]) { set_error("inertial link %d joins a keyframe without IMU state", l); return TC2LI_ERR_INVALID; }
            L[l].kf1 = in.kf1; L[l].kf2 = in.kf2; L[l].robust = in.robust != 0; L[l].pre = in.preintegrated;
            if (!L[l].prepare(in.info_scale)) { set_error("inertial link %d: the pre-integration covariance is not positive definite", l); return TC2LI_ERR_INVALID; }
            extra_used[in.kf1] = extra_used[in.kf2] = 1;
        }
        const float d_imu_f = sqrtf(16.92f);
        d_imu = d_imu_f;
        dsqr_imu = (float)((double)d_imu_f * (double)d_imu_f);
        return TC2LI_OK;
    }
    // imu_used: keyframes whose velocity / bias vertices an inertial edge touches (extra_used before the LiDAR window was added)
    void number(const uint8_t* fixed, const uint8_t* has_imu, const std::vector<uint8_t>& imu_used, int n_kfs, const std::vector<int>& pose_var_, int np_) {
        pose_var = &pose_var_; np = np_;
        imu_var.assign(n_kfs, -1);
        n_imu = 0;
        for (int k = 0; k < n_kfs; ++k) if (!fixed[k] && has_imu[k] && imu_used[k]) imu_var[k] = n_imu++;
        n = np + 9 * n_imu;
        Hi.assign((size_t)n * n, 0.0); bi.assign(n, 0.0);
        seg_at.clear(); seg_len.clear(); segs_ready = false;
    }
    // whether k_lvi_solve* takes this window's reduced system: velocity / bias unknowns present, the pose block and the rings fit a CU's LDS
    // (25 free keyframes: the reference's largest window), every inertial edge joins keyframes at most two places apart in the numbering
    // (band <= kLviBand).  The decision depends on the window alone: the same alone and in a batch.  TC2LI_LVI_DEVICE_SOLVE=0: the host's
    // envelope LDL^T (reduced_solve.hpp) for every window.
    bool device_solve_ok() const {
        if (!BaOptions::read().lvi_device_solve || n_imu <= 0 || np <= 0 || np > kLviMaxPoseRows || !lvi_device_solve_available()) return false;
        for (const InertialLinkHost& lk_ : L) {
            const int i1 = imu_var[lk_.kf1], i2 = imu_var[lk_.kf2];
            if (i1 >= 0 && i2 >= 0 && std::abs(i1 - i2) > 2) return false;
        }
        return true;
    }
    double cost(const std::vector<ImuPose>& Pz, const std::vector<ImuVertexState>& Sz, bool linearize) {
        const std::vector<int>& pv = *pose_var;
        double chi = 0;
        if (linearize) {
            if (segs_ready) {
                for (size_t k = 0; k < seg_at.size(); ++k) std::fill_n(Hi.data() + seg_at[k], seg_len[k], 0.0);
                // TC2LI_TEST_HI_CLEAR (tests): every writer of Hi must have registered its blocks during the first linearisation -- after the
                // segment-wise clear the matrix has to be zero everywhere, or a term added later is accumulating stale entries
                static const bool kCheck = getenv("TC2LI_TEST_HI_CLEAR") != nullptr;
                if (kCheck) for (double v : Hi) if (v != 0.0) { fprintf(stderr, "tc2li: InertialTerm: Hi holds an entry outside the registered segments\n"); abort(); }
            } else std::fill(Hi.begin(), Hi.end(), 0.0);
            std::fill(bi.begin(), bi.end(), 0.0);
        }
        for (const InertialLinkHost& lk_ : L) {
            double er[9], J[9 * 24];
            lk_.evaluate(Pz[lk_.kf1], Sz[lk_.kf1], Pz[lk_.kf2], Sz[lk_.kf2], er, linearize ? J : nullptr);
            double Oe[9], c2 = 0;
            for (int r = 0; r < 9; ++r) { double s = 0; for (int k = 0; k < 9; ++k) s += lk_.info[9 * r + k] * er[k]; Oe[r] = s; c2 += er[r] * s; }
            double rho0 = c2, rho1 = 1.0;
            if (lk_.robust) huber(c2, d_imu, dsqr_imu, rho0, rho1);
            chi += rho0;
            double eg[3], ea[3], Og[3], Oa[3];
            for (int k = 0; k < 3; ++k) { eg[k] = Sz[lk_.kf2].bg[k] - Sz[lk_.kf1].bg[k]; ea[k] = Sz[lk_.kf2].ba[k] - Sz[lk_.kf1].ba[k]; }
            for (int r = 0; r < 3; ++r) {
                Og[r] = lk_.infoG[3 * r] * eg[0] + lk_.infoG[3 * r + 1] * eg[1] + lk_.infoG[3 * r + 2] * eg[2];
                Oa[r] = lk_.infoA[3 * r] * ea[0] + lk_.infoA[3 * r + 1] * ea[1] + lk_.infoA[3 * r + 2] * ea[2];
                chi += eg[r] * Og[r] + ea[r] * Oa[r];
            }
            if (!linearize) continue;
            const int i1 = imu_var[lk_.kf1], i2 = imu_var[lk_.kf2], p1 = pv[lk_.kf1], p2 = pv[lk_.kf2];
            const int off[6] = {p1 >= 0 ? 6 * p1 : -1, i1 >= 0 ? np + 9 * i1 : -1, i1 >= 0 ? np + 9 * i1 + 3 : -1, i1 >= 0 ? np + 9 * i1 + 6 : -1,
                                p2 >= 0 ? 6 * p2 : -1, i2 >= 0 ? np + 9 * i2 : -1};
            const int col[6] = {0, 6, 9, 12, 15, 21}, sz[6] = {6, 3, 3, 3, 6, 3};
            double OJ[9 * 24];  // (rho' Omega) J
            for (int r = 0; r < 9; ++r)
                for (int c = 0; c < 24; ++c) { double t = 0; for (int k = 0; k < 9; ++k) t += rho1 * lk_.info[9 * r + k] * J[24 * k + c]; OJ[24 * r + c] = t; }
            for (int a = 0; a < 6; ++a) {
                if (off[a] < 0) continue;
                for (int r = 0; r < sz[a]; ++r) {
                    double s = 0;
                    for (int k = 0; k < 9; ++k) s += J[24 * k + col[a] + r] * (rho1 * Oe[k]);
                    bi[off[a] + r] -= s;
                    for (int b2 = 0; b2 < 6; ++b2) {
                        if (off[b2] < 0) continue;
                        note_segment((size_t)(off[a] + r) * n + off[b2], sz[b2]);
                        for (int c = 0; c < sz[b2]; ++c) {
                            double h = 0;
                            for (int k = 0; k < 9; ++k) h += J[24 * k + col[a] + r] * OJ[24 * k + col[b2] + c];
                            Hi[(size_t)(off[a] + r) * n + off[b2] + c] += h;
                        }
                    }
                }
            }
            for (int which = 0; which < 2; ++which) {  // EdgeGyroRW / EdgeAccRW: J = (-I, I)
                const double* Om = which == 0 ? lk_.infoG : lk_.infoA;
                const double* Oe3 = which == 0 ? Og : Oa;
                const int o1 = i1 >= 0 ? np + 9 * i1 + 3 + 3 * which : -1, o2 = i2 >= 0 ? np + 9 * i2 + 3 + 3 * which : -1;
                for (int r = 0; r < 3; ++r) {
                    if (o1 >= 0) { note_segment((size_t)(o1 + r) * n + o1, 3); if (o2 >= 0) note_segment((size_t)(o1 + r) * n + o2, 3); }
                    if (o2 >= 0) { note_segment((size_t)(o2 + r) * n + o2, 3); if (o1 >= 0) note_segment((size_t)(o2 + r) * n + o1, 3); }
                    if (o1 >= 0) bi[o1 + r] += Oe3[r];
                    if (o2 >= 0) bi[o2 + r] -= Oe3[r];
                    for (int c = 0; c < 3; ++c) {
                        if (o1 >= 0) Hi[(size_t)(o1 + r) * n + o1 + c] += Om[3 * r + c];
                        if (o2 >= 0) Hi[(size_t)(o2 + r) * n + o2 + c] += Om[3 * r + c];
                        if (o1 >= 0 && o2 >= 0) { Hi[(size_t)(o1 + r) * n + o2 + c] -= Om[3 * r + c]; Hi[(size_t)(o2 + r) * n + o1 + c] -= Om[3 * r + c]; }
                    }
                }
            }
        }
        if (linearize) segs_ready = true;
        return chi;
    }
};


}  // namespace ba_detail
}  // namespace tc2li

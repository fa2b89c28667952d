// The optimiser's index structure of a local-BA window on gfx950: what ba_build_structure (ba_structure.hpp) makes on the host, from the
// gather's device output.  Integer work only; no float arithmetic, no MFMA.
//   k_bas_structure  one workgroup per window.  The gather's edges are point-major in listed order and a point has at most one edge per
//                    keyframe, so pt_off is the gather's edge_start, pt_edges the identity, and there are no duplicate pairs.
//                    used / pose_var   an atomicOr of 1 per edge on its pose (and per LiDAR keyframe), then a block prefix sum over the poses.
//                    slots             a thread per point counts its edges with a free pose; a block prefix sum in point order gives the
//                                      point its first slot (fl_off), and the thread writes fl_pose / fl_lm / fl_edge of its slots in edge
//                                      order.  pv_off: per-pose counts by atomicAdd (a count does not depend on the order), summed by one thread.
//                    slices, groups    the two greedy partitions are sequential over the points: lane 0 of wavefront 0 walks the first-slot
//                                      prefix sums for the slices, lane 0 of wavefront 1 the first-edge prefix sums for the groups, both in LDS
//                                      and both at once (DESIGN.md says what that costs and why the chained wavefront form was not needed).
//   k_bas_blocks     one workgroup per block of 256 slots: the block's slots sorted by pose, stable.  A slot's place is the number of slots
//                    with a smaller pose plus the number of earlier slots with the same pose, counted over the 256 poses in LDS (a
//                    broadcast read each).  The grid is cut from the capacities; a workgroup beyond the window's blocks returns at once.
// Helpers with a barrier inside (block_scan_excl, __syncthreads_or) are only called where all 256 threads arrive: every loop around them runs
// to a bound that is the same in all threads, and every early return is taken by the whole workgroup.
#include <algorithm>

#include "ba_structure_device.hpp"
#include "ba_device.hpp"
#include "launch.hpp"

namespace tc2li {

static_assert(kBasMaxFree == kSchurLeanMaxFree, "the device range is the lean sparse path");
static_assert(kBasThreads == 256 && kBasMaxFree < 255, "a block's rows are bytes; 255 marks a thread past the end");

__global__ __launch_bounds__(kBasThreads) void k_bas_structure(BasBatch B) {
    __shared__ int s_pose[kBasMaxPoses];         // a pose's mark, then its number among the free poses
    __shared__ int s_pt[kBasMaxPoints + 1];      // pt_off
    __shared__ int s_sb[kBasMaxPoints + 1];      // the first slot of every point
    __shared__ uint8_t s_place[kBasMaxPoints];   // the point's number within its slice (below 64)
    __shared__ int s_hist[kBasMaxFree + 2];
    __shared__ int scan[kBasThreads / 64];
    __shared__ int sh[4];                        // [1] slices, [2] groups, [3] the most points of a group
    const int w = blockIdx.x, tid = threadIdx.x;
    const BawProblemDev& P = B.problems[w];
    const BasWindowDev& W = B.windows[w];
    const int32_t* counts = B.counts + (size_t)w * TC2LI_BA_WINDOW_COUNTS;
    const int K = counts[TC2LI_BA_WINDOW_N_POSES], NP = counts[TC2LI_BA_WINDOW_N_POINTS], E = counts[TC2LI_BA_WINDOW_N_EDGES];
    BasSizes out{};
    // nothing to build (the host answers from the counts), or outside the range: decided from values that are the same in all threads
    if (counts[TC2LI_BA_WINDOW_STATUS] != TC2LI_BA_WINDOW_OK || K > P.pose_cap || NP > P.point_cap || E > P.edge_cap) out.status = kBasNone;
    else if (K > kBasMaxPoses || NP > kBasMaxPoints) out.status = kBasDeclined;
    else out.status = kBasBuilt;
    if (out.status != kBasBuilt) {
        if (tid == 0) B.sizes[w] = out;
        return;
    }
    const uint8_t* fixed = B.fixed + P.pose_off;
    const int32_t* est = B.edge_start + P.point_off;
    const tc2li_ba_edge* edges = B.edges + P.edge_off;
    int32_t* g_pose_var = B.scratch + W.pose_var;
    int32_t* g_pt_off = B.scratch + W.pt_off;
    int32_t* g_pt_edges = B.scratch + W.pt_edges;
    int32_t* g_pv_off = B.scratch + W.pv_off;
    int32_t* g_fl_off = B.scratch + W.fl_off;
    int32_t* g_fl_pose = B.scratch + W.fl_pose;
    int32_t* g_fl_lm = B.scratch + W.fl_lm;
    int32_t* g_fl_place = B.scratch + W.fl_place;
    int32_t* g_fl_edge = B.scratch + W.fl_edge;
    int32_t* g_slice_off = B.scratch + W.slice_off;
    int32_t* g_grp_k0 = B.scratch + W.grp_k0;
    int32_t* g_grp_l0 = B.scratch + W.grp_l0;

    for (int k = tid; k < K; k += kBasThreads) s_pose[k] = 0;
    if (tid < kBasMaxFree + 2) s_hist[tid] = 0;
    if (tid < 4) sh[tid] = 0;
    __syncthreads();
    // used: a pose an edge names, and the keyframes of the LiDAR edge
    int bad = 0;
    for (int e = tid; e < E; e += kBasThreads) {
        const int k = edges[e].pose;
        if (k >= 0 && k < K) atomicOr(&s_pose[k], 1);
        else bad = 1;
        g_pt_edges[e] = e;
    }
    if (W.use_lidar && tid < TC2LI_BA_WINDOW_MAX_LIDAR) {
        const int k = B.lidar_pose_index[(size_t)w * TC2LI_BA_WINDOW_MAX_LIDAR + tid];
        if (k >= 0 && k < K) atomicOr(&s_pose[k], 1);
    }
    __syncthreads();
    // pose_var: the free poses that are used, numbered in pose order
    int n_free = 0;
    for (int base = 0; base < K; base += kBasThreads) {
        const int k = base + tid;
        const bool fr = k < K && !fixed[k] && s_pose[k] != 0;
        int tot;
        const int at = block_scan_excl<kBasThreads>(fr ? 1 : 0, scan, &tot);
        if (k < K) {
            const int v = fr ? n_free + at : -1;
            s_pose[k] = v;
            g_pose_var[k] = v;
        }
        n_free += tot;
    }
    __syncthreads();
    if (n_free > kBasMaxFree) {
        out.status = kBasDeclined;
        if (tid == 0) B.sizes[w] = out;
        return;
    }
    // slots: a point's edges with a free pose, in point order then edge order
    int n_slots = 0;
    for (int base = 0; base < NP; base += kBasThreads) {
        const int l = base + tid;
        int e0 = 0, e1 = 0, nf = 0;
        if (l < NP) {
            e0 = est[l];
            e1 = l + 1 < NP ? est[l + 1] : E;
            if (e0 < 0 || e1 > E || e1 <= e0 || e1 - e0 > 256) { bad = 1; e1 = e0; }   // no edge, or more than 256 of them
            for (int e = e0; e < e1; ++e) {
                const int k = edges[e].pose;
                nf += (k >= 0 && k < K && s_pose[k] >= 0) ? 1 : 0;
            }
        }
        int tot;
        const int at = block_scan_excl<kBasThreads>(nf, scan, &tot);
        if (l < NP) {
            int s = n_slots + at;
            s_pt[l] = e0; s_sb[l] = s;
            g_pt_off[l] = e0;
            g_fl_off[2 * (size_t)l] = s; g_fl_off[2 * (size_t)l + 1] = s + nf;
            for (int e = e0; e < e1; ++e) {
                const int k = edges[e].pose;
                const int i = (k >= 0 && k < K) ? s_pose[k] : -1;
                if (i < 0) continue;
                g_fl_pose[s] = i; g_fl_lm[s] = l; g_fl_edge[s] = e;
                atomicAdd(&s_hist[i + 1], 1);
                ++s;
            }
        }
        n_slots += tot;
    }
    if (tid == 0) { s_pt[NP] = E; s_sb[NP] = n_slots; g_pt_off[NP] = E; }
    if (__syncthreads_or(bad)) {
        out.status = kBasInvalid;
        if (tid == 0) B.sizes[w] = out;
        return;
    }
    if (tid == 0) {
        // pv_off, then the slices: whole points, at most 64 of them and at most kSchurLeanSlots slots
        int a = 0;
        for (int i = 0; i <= n_free; ++i) { a += s_hist[i]; g_pv_off[i] = a; }
        int n_sl = 0, slice_start = 0, lms = 0;
        g_slice_off[0] = 0;
        for (int l = 0; l < NP; ++l) {
            const int b = s_sb[l], e = s_sb[l + 1];
            if (e == b) continue;
            if (lms == 64 || e - slice_start > kSchurLeanSlots) { g_slice_off[++n_sl] = b; slice_start = b; lms = 0; }
            s_place[l] = (uint8_t)lms;
            ++lms;
        }
        if (n_slots > slice_start) g_slice_off[++n_sl] = n_slots;
        sh[1] = n_sl;
    } else if (tid == 64) {
        // the groups: whole points, at most 256 edges
        int ng = 0, k0 = 0, l0 = 0, most = 0;
        g_grp_k0[0] = 0; g_grp_l0[0] = 0;
        for (int l = 0; l < NP; ++l)
            if (s_pt[l + 1] - k0 > 256) {
                most = max(most, l - l0);
                k0 = s_pt[l]; l0 = l;
                ++ng;
                g_grp_k0[ng] = k0; g_grp_l0[ng] = l0;
            }
        most = max(most, NP - l0);
        ++ng;
        g_grp_k0[ng] = E; g_grp_l0[ng] = NP;
        sh[2] = ng; sh[3] = most;
    }
    __syncthreads();
    for (int l = tid; l < NP; l += kBasThreads) {
        const int place = s_place[l];
        for (int s = s_sb[l]; s < s_sb[l + 1]; ++s) g_fl_place[s] = place;
    }
    if (tid == 0) {
        out.status = sh[3] > 256 ? kBasInvalid : kBasBuilt;
        out.n_free = n_free; out.n_free_edges = n_slots; out.n_schur_slices = sh[1]; out.n_groups = sh[2];
        out.n_blocks = (n_slots + 255) / 256; out.max_group_landmarks = sh[3];
        B.sizes[w] = out;
    }
}

__global__ __launch_bounds__(kBasThreads) void k_bas_blocks(BasBatch B) {
    __shared__ int sp[kBasThreads];
    const int w = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const BasSizes S = B.sizes[w];
    const BasWindowDev& W = B.windows[w];
    if (S.status != kBasBuilt || b >= max(S.n_blocks, 1) || b >= W.max_blocks) return;
    const int n_free = S.n_free, s = 256 * b + tid;
    const int mine = s < S.n_free_edges ? B.scratch[W.fl_pose + s] : 255;
    sp[tid] = mine;
    __syncthreads();
    int below = 0, rank = 0, below_tid = 0;
    for (int j = 0; j < kBasThreads; ++j) {
        const int v = sp[j];
        below += v < mine ? 1 : 0;
        rank += (v == mine && j < tid) ? 1 : 0;
        below_tid += v < tid ? 1 : 0;
    }
    uint8_t* rows = B.scratch_rows + W.blk_rows + (size_t)b * 256;
    rows[mine != 255 ? below + rank : tid] = mine != 255 ? (uint8_t)tid : (uint8_t)0;   // the threads past the end hold the places past the end
    if (tid <= n_free) B.scratch[W.blk_off + (size_t)b * (n_free + 1) + tid] = below_tid;
}

// One workgroup per window; a flagged compaction in two passes (monocular, then stereo), each a block prefix sum over chunks of 256 edges.
__global__ __launch_bounds__(kBasThreads) void k_bas_outliers(const BasOutlierTask* __restrict__ tasks) {
    __shared__ int scan[kBasThreads / 64];
    const BasOutlierTask T = tasks[blockIdx.x];
    const int tid = threadIdx.x;
    int n = 0;
    for (int stereo = 0; stereo < 2; ++stereo) {
        const double limit = stereo ? 7.815 : 5.991;                                    // :414, :444
        for (int base = 0; base < T.n_edges; base += kBasThreads) {
            const int i = base + tid;
            bool erased = false;
            int pose = 0, point = 0;
            if (i < T.n_edges) {
                const tc2li_ba_edge e = T.edges[i];
                pose = e.pose; point = e.point;
                erased = ((e.u_right >= 0) == (stereo != 0)) && (T.chi2[i] > limit || !T.depth_positive[i]);
            }
            int tot;
            const int at = n + block_scan_excl<kBasThreads>(erased ? 1 : 0, scan, &tot);
            if (erased && at < T.capacity) { T.erase_pose[at] = pose; T.erase_point[at] = point; }   // :417, :447
            n += tot;
        }
    }
    if (tid == 0) *T.n_erase = n;
}

void launch_ba_outliers(const BasOutlierTask* tasks, int n, hipStream_t st) {
    if (n <= 0) return;
    TC2LI_LAUNCH(k_bas_outliers, dim3(n), dim3(kBasThreads), 0, st, tasks);
}

void launch_ba_structure(const BasBatch& B, hipStream_t st) {
    if (B.n_windows <= 0) return;
    TC2LI_LAUNCH(k_bas_structure, dim3(B.n_windows), dim3(kBasThreads), 0, st, B);
    TC2LI_LAUNCH(k_bas_blocks, dim3(B.n_windows, std::max(B.max_blocks, 1)), dim3(kBasThreads), 0, st, B);
}

}  // namespace tc2li

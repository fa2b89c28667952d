// The window of the local BA on gfx950: the graph walk of OptimizerWithLidar::LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:63-130,
// :157-187, :226-253, :263-384) on the flat graph.  Integer work and copies; no float arithmetic, no MFMA.
//   k_baw_gather   one workgroup per problem, everything whose order matters:
//                  local keyframes   cov_kf compacted in its order by a block prefix sum; every keyframe's marks are one int, in LDS up to
//                                    kWinLdsKeyframes keyframes and in global memory beyond.
//                  local points      window_list_points over the local keyframes (:78-104): first occurrences by an integer atomicMin on the
//                                    point's key (LDS up to kWinLdsPoints points, global memory beyond) and a block prefix sum.
//                  fixed cameras     a thread per listed point walks its observations: atomicOr of the fixed bit on every observer that is
//                                    not marked local (:115-119), and the point's edges counted; a prefix sum gives every point its first edge.
//                  poses             the marked rows compacted, then ranked by (kf_id, row) (window_compact_members, window_rank_members).
//   k_window_edges kWinEdgeBlocks workgroups per problem, a thread per listed point: its row and position, and one edge per observation
//                  from the first edge on (:277-345), the pixel read from the observer's slot of the keyframe store.  The inertial gather
//                  (inertial_window_kernels.hip) ends with the same kernel.
// The listing, the compaction, the ranking and the LDS / global dispatch are window_gather_device.hpp's, shared with the inertial gather.
// Helpers with a barrier inside are only called where all 256 threads arrive (block_scan_excl in launch.hpp says what that takes).
#include "ba_window_device.hpp"

namespace tc2li {

// marks / first: the problem's keyframe marks and first-occurrence keys, LDS or global (the address space is known after inlining)
// sh: [0] a local keyframe is the initial one (:85-88), [1 .. 6] vOptKeyFrames of :227-233 as rows
__device__ __forceinline__ void baw_problem(const BawBatch& B, const BawProblemDev& P, int* marks, int* first, int* scan, int* sh) {
    const int tid = threadIdx.x;
    const uint8_t* flags = B.kf_flags + P.t_kf;
    const int64_t* kf_id = B.kf_id + P.t_kf;
    const int32_t* slot_row = B.slot_offsets + P.slot_row;
    const int32_t* slot_point = B.slot_point + P.t_slot;
    const int32_t* cov = B.cov_kf + P.cov_off;
    int n_cov = P.n_cov;
    if (P.cov_row1) {   // GetVectorCovisibleKeyFrames() as it is resident: the ordered row of the current keyframe, in its order
        const int row = P.cov_row1 - 1;
        const int o0 = B.ord_offsets[row];
        n_cov = min(B.ord_offsets[row + 1] - o0, P.n_cov);
        cov = B.ord_kf + (size_t)(row / B.ord_rows) * B.ord_cap + o0;
    }
    const uint8_t* pflags = B.point_flags + P.t_point;
    const int32_t* obs_row = B.obs_offsets + P.obs_row;
    const int32_t* obs_kf = B.obs_kf + P.t_obs;
    const int32_t* obs_index = B.obs_index + P.t_obs;
    int32_t* list_kf = B.list_kf + P.cov_off + 2 * blockIdx.x;
    int32_t* listed = B.listed + P.point_off;
    int32_t* edge_start = B.edge_start + P.point_off;
    int32_t* kf_pose = B.vertex_of + P.kf_off;
    int32_t* members = B.members + P.kf_off;
    int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_BA_WINDOW_COUNTS;
    const int cur = P.current;
    const int64_t init_id = P.init_kf_id;

    for (int k = tid; k < P.n_kf; k += kWinThreads) marks[k] = 0;
    for (int p = tid; p < P.n_points; p += kWinThreads) first[p] = 0x7fffffff;
    if (tid < 8) sh[tid] = tid == 0 ? 0 : -1;
    __syncthreads();

    // local keyframes (:63-76); cov_kf names no row twice and not the current one, so every marks[] entry below has one writer
    int n_local = 1, n_cloud = (flags[cur] & 4) ? 1 : 0;
    if (tid == 0) {
        marks[cur] = kBawMarkedLocal | kBawLocal;                                    // :65-66
        list_kf[0] = cur;
        if (n_cloud) sh[1] = cur;
        if (kf_id[cur] == init_id) atomicOr(&sh[0], 1);
    }
    for (int base = 0; base < n_cov; base += kWinThreads) {
        const int i = base + tid;
        const int k = i < n_cov ? cov[i] : -1;
        const int f = k >= 0 ? flags[k] : 3;
        const bool local = !(f & 3);                                                 // :74
        const bool cloud = local && (f & 4);                                         // :231
        if (k >= 0) marks[k] = kBawMarkedLocal | (local ? kBawLocal : 0);            // :73, :75
        int tot;
        const int at = block_scan_excl<kWinThreads>((local ? 1 : 0) | (cloud ? 1 << 16 : 0), scan, &tot);   // at most 256 of each
        if (local) {
            list_kf[n_local + (at & 0xffff)] = k;
            if (kf_id[k] == init_id) atomicOr(&sh[0], 1);                            // :85-88
        }
        if (cloud && n_cloud + (at >> 16) < TC2LI_BA_WINDOW_MAX_LIDAR) sh[1 + n_cloud + (at >> 16)] = k;
        n_local += tot & 0xffff;
        n_cloud += tot >> 16;
    }
    __syncthreads();

    // local points (:78-104): a point that is bad or of another map is passed over (:93-94), the others are listed once (:97-101)
    const int n_listed = window_list_points(list_kf, n_local, slot_row, slot_point, pflags, 3, first, listed, scan);
    __syncthreads();

    // fixed cameras (:107-122), and the edges of every listed point counted (:277-345)
    int n_edges = 0, n_without = 0;
    for (int base = 0; base < n_listed; base += kWinThreads) {
        const int i = base + tid;
        int ne = 0;
        if (i < n_listed) {
            const int p = listed[i];
            const int o1 = obs_row[p + 1];
            for (int o = obs_row[p]; o < o1; ++o) {
                const int k = obs_kf[o];
                if (flags[k] & 3) continue;                                          // :118, :281
                if (!(marks[k] & kBawMarkedLocal)) atomicOr(&marks[k], kBawFixed);   // :115-119
                ne += obs_index[o] >= 0 ? 1 : 0;                                     // :286, :313
            }
        }
        int tot;
        const int at = block_scan_excl<kWinThreads>(ne, scan, &tot);
        if (i < n_listed) edge_start[i] = n_edges + at;
        n_edges += tot;
        n_without += __syncthreads_count(i < n_listed && ne == 0);
    }
    __syncthreads();

    // the rows that get a pose vertex (:157-187), compacted, and the fixed cameras among them counted
    int n_fixed;
    const int n_members = window_compact_members(marks, P.n_kf, members, kf_pose, scan, &n_fixed, [](int m) {
        return ((m & (kBawLocal | kBawFixed)) ? 1 : 0) | ((m & kBawFixed) ? 1 << 16 : 0);
    });
    const int num_fixed = n_fixed + sh[0];                                           // :123
    if (num_fixed == 0) {                                                            // :126-130
        if (tid < TC2LI_BA_WINDOW_COUNTS) counts[tid] = tid == TC2LI_BA_WINDOW_STATUS ? TC2LI_BA_WINDOW_ABORTED : 0;
        if (tid < TC2LI_BA_WINDOW_MAX_LIDAR) B.lidar_pose_index[(size_t)blockIdx.x * TC2LI_BA_WINDOW_MAX_LIDAR + tid] = -1;
        if (tid == 0) B.n_emit[blockIdx.x] = 0;
        return;
    }
    // vertex-id order
    int32_t* pose_row = B.pose_row + P.pose_off;
    double* poses7_out = B.poses7_out + (size_t)P.pose_off * 7;
    uint8_t* fixed_out = B.fixed + P.pose_off;
    const double* poses7 = B.poses7 + (size_t)P.t_kf * 7;
    window_rank_members(kf_id, members, n_members, kf_pose, P.pose_cap, [&](int k, int r, int64_t id) {
        pose_row[r] = k;
#pragma unroll
        for (int c = 0; c < 7; ++c) poses7_out[(size_t)r * 7 + c] = poses7[(size_t)k * 7 + c];
        fixed_out[r] = ((marks[k] & kBawFixed) || id == init_id) ? 1 : 0;            // :181, :164
    });
    const int n_lidar = n_cloud > 2 ? (n_cloud < TC2LI_BA_WINDOW_MAX_LIDAR ? n_cloud : TC2LI_BA_WINDOW_MAX_LIDAR) : 0;   // :235, :244-245
    if (tid < TC2LI_BA_WINDOW_MAX_LIDAR)
        B.lidar_pose_index[(size_t)blockIdx.x * TC2LI_BA_WINDOW_MAX_LIDAR + tid] = tid < n_lidar ? kf_pose[sh[1 + tid]] : -1;   // :249-252
    if (tid == 0) {
        counts[TC2LI_BA_WINDOW_STATUS] = TC2LI_BA_WINDOW_OK;
        counts[TC2LI_BA_WINDOW_NUM_FIXED_KF] = num_fixed;
        counts[TC2LI_BA_WINDOW_NUM_OPT_KF] = n_local;                                // :171
        counts[TC2LI_BA_WINDOW_N_POSES] = n_members;
        counts[TC2LI_BA_WINDOW_N_POINTS] = n_listed;
        counts[TC2LI_BA_WINDOW_N_EDGES] = n_edges;
        counts[TC2LI_BA_WINDOW_N_LIDAR] = n_lidar;
        counts[TC2LI_BA_WINDOW_N_POINTS_WITHOUT_EDGE] = n_without;
        B.n_emit[blockIdx.x] = (n_members <= P.pose_cap && n_listed <= P.point_cap && n_edges <= P.edge_cap) ? n_listed : 0;
    }
}

__global__ __launch_bounds__(kWinThreads) void k_baw_gather(BawBatch B) {
    __shared__ int marks[kWinLdsKeyframes];
    __shared__ int first[kWinLdsPoints];
    __shared__ int scan[kWinThreads / 64];
    __shared__ int sh[8];
    const BawProblemDev& P = window_problem<BawProblemDev>(B, blockIdx.x);
    window_dispatch(B, P, marks, first, [&](int* m, int* f) __attribute__((always_inline)) { baw_problem(B, P, m, f, scan, sh); });
}

// The points and edges of every problem that the gather before it let through (n_emit), for both gathers.  An observation gives an edge
// when its keyframe has a vertex, is neither bad nor of another map, and sees the point at a keypoint (visual :281, :286, :313; inertial
// :862, :865, :872, :902).  The first term is the inertial gather's: there a keyframe has a vertex exactly when it carries one of the two
// marks.  In the visual gather it is always true where the second term lets an observation pass: every observer of a listed point that is
// neither bad nor of another map is either marked local -- and then in lLocalKeyFrames, because it is not "other" -- or was given the
// fixed bit by the gather's walk over the same observations; either way it is a member and has its place among the poses.  (A window
// that ended ABORTED has n_emit 0.)  The tests that compare both device entries byte for byte with their host entries check this.
__global__ __launch_bounds__(kWinThreads) void k_window_edges(WindowBatch B) {
    const WindowProblemDev& P = window_problem<WindowProblemDev>(B, blockIdx.x);
    const int n_listed = B.n_emit[blockIdx.x];
    const uint8_t* flags = B.kf_flags + P.t_kf;
    const int32_t* kf_slot = B.kf_slot + P.t_kf;
    const int32_t* vertex_of = B.vertex_of + P.kf_off;
    const int32_t* obs_row = B.obs_offsets + P.obs_row;
    const int32_t* obs_kf = B.obs_kf + P.t_obs;
    const int32_t* obs_index = B.obs_index + P.t_obs;
    const int32_t* listed = B.listed + P.point_off;
    const int32_t* edge_start = B.edge_start + P.point_off;
    const double* positions = B.positions + (size_t)P.t_point * 3;
    int32_t* point_row = B.point_row + P.pointo_off;
    double* points3_out = B.points3_out + (size_t)P.pointo_off * 3;
    tc2li_ba_edge* edges = B.edges + P.edge_off;
    for (int i = blockIdx.y * kWinThreads + threadIdx.x; i < n_listed; i += kWinEdgeBlocks * kWinThreads) {
        const int p = listed[i];
        point_row[i] = p;
#pragma unroll
        for (int c = 0; c < 3; ++c) points3_out[(size_t)i * 3 + c] = positions[(size_t)p * 3 + c];   // :267 / :849
        int e = edge_start[i];
        const int o1 = obs_row[p + 1];
        for (int o = obs_row[p]; o < o1; ++o) {
            const int k = obs_kf[o], idx = obs_index[o];
            // vertex_of[k] < 0 || (flags[k] & 3) || idx < 0, with both loads in flight before the one branch
            const int vertex = vertex_of[k], f = flags[k];
            if ((vertex < 0) | ((f & 3) != 0) | (idx < 0)) continue;
            const uint8_t* slot = B.store.slots + (size_t)kf_slot[k] * B.store.stride;
            const tc2li_keypoint kp = reinterpret_cast<const tc2li_keypoint*>(slot + B.store.keys)[idx];
            const float ur = reinterpret_cast<const float*>(slot + B.store.u_right)[idx];
            tc2li_ba_edge E;
            E.point = i;
            E.pose = vertex;
            E.u = (double)kp.x;                                                      // :290, :318 / :876-878, :904-909
            E.v = (double)kp.y;
            E.u_right = ur >= 0.f ? (double)ur : -1.0;
            E.inv_sigma2 = (double)B.inv_level_sigma2[kp.octave];                    // :297, :325 / :889, :920
            edges[e++] = E;
        }
    }
}

void launch_window_edges(const WindowBatch& B, hipStream_t st) {
    TC2LI_LAUNCH(k_window_edges, dim3(B.n_problems, kWinEdgeBlocks), dim3(kWinThreads), 0, st, B);
}

void launch_ba_window(const BawBatch& B, hipStream_t st) {
    if (B.n_problems <= 0) return;
    TC2LI_LAUNCH(k_baw_gather, dim3(B.n_problems), dim3(kWinThreads), 0, st, B);
    launch_window_edges(B, st);
}

}  // namespace tc2li

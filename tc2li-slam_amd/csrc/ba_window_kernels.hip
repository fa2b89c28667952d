// The window of the local BA on gfx950: the graph walk of OptimizerWithLidar::LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:63-130,
// :157-187, :226-253, :263-384) on the flat graph.  Integer work and copies; no float arithmetic, no MFMA.
//   k_baw_gather   one workgroup per problem, everything whose order matters:
//                  local keyframes   cov_kf compacted in its order by a block prefix sum; every keyframe's marks are one int, in LDS up to
//                                    kBawLdsKeyframes keyframes and in global memory beyond.
//                  local points      the slots of the local keyframes, concatenated in list order, are numbered q = 0, 1, ...; every slot does
//                                    an integer atomicMin of q on its point's key (LDS up to kBawLdsPoints points, global memory beyond), the
//                                    slot whose q is the minimum is the point's first occurrence (:97-101), and a block prefix sum over the
//                                    flags in q order is the point's place in lLocalMapPoints -- no sort, and minima do not depend on their order.
//                  fixed cameras     a thread per listed point walks its observations: atomicOr of the fixed bit on every observer that is
//                                    not marked local (:115-119), and the point's edges counted; a prefix sum gives every point its first edge.
//                  poses             the marked rows compacted, then ranked by (kf_id, row): a pose's place is the number of smaller keys
//                                    (a few hundred keyframes at most: members^2 / 256 compares per thread).
//   k_baw_edges    kBawEdgeBlocks workgroups per problem, a thread per listed point: its row and position, and one edge per observation
//                  from the first edge on (:277-345), the pixel read from the observer's slot of the keyframe store.
// Helpers with a barrier inside (block_scan_excl, __syncthreads_count) are only called where all 256 threads arrive: every loop around them
// runs to a bound that is the same in all threads, and a thread past the end takes part with a zero.
#include "ba_window_device.hpp"
#include "launch.hpp"

namespace tc2li {

// Exclusive prefix sum of v over the workgroup's kBawThreads threads, the total in *total.  lds: 4 ints.
__device__ __forceinline__ int baw_scan_excl(int v, int* lds, int* total) {
    const int lane = threadIdx.x & 63, w = wave_in_block();
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
    if (lane == 63) lds[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < kBawThreads / 64; ++k) {
        const int s = lds[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// marks / first: the problem's keyframe marks and first-occurrence keys, LDS or global (the address space is known after inlining)
// sh: [0] a local keyframe is the initial one (:85-88), [1 .. 6] vOptKeyFrames of :227-233 as rows
__device__ __forceinline__ void baw_problem(const BawBatch& B, const BawProblemDev& P, int* marks, int* first, int* scan, int* sh) {
    const int tid = threadIdx.x;
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int64_t* kf_id = B.kf_id + P.kf_off;
    const int32_t* slot_row = B.slot_offsets + P.kf_off + blockIdx.x;
    const int32_t* slot_point = B.slot_point + P.slot_off;
    const int32_t* cov = B.cov_kf + P.cov_off;
    const uint8_t* pflags = B.point_flags + P.point_off;
    const int32_t* obs_row = B.obs_offsets + P.point_off + blockIdx.x;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int32_t* obs_index = B.obs_index + P.obs_off;
    int32_t* list_kf = B.list_kf + P.cov_off + 2 * blockIdx.x;
    int32_t* list_start = B.list_start + P.cov_off + 2 * blockIdx.x;
    int32_t* listed = B.listed + P.point_off;
    int32_t* edge_start = B.edge_start + P.point_off;
    int32_t* kf_pose = B.kf_pose + P.kf_off;
    int32_t* members = B.members + P.kf_off;
    int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_BA_WINDOW_COUNTS;
    const int cur = P.current;
    const int64_t init_id = P.init_kf_id;

    for (int k = tid; k < P.n_kf; k += kBawThreads) marks[k] = 0;
    for (int p = tid; p < P.n_points; p += kBawThreads) first[p] = 0x7fffffff;
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
    for (int base = 0; base < P.n_cov; base += kBawThreads) {
        const int i = base + tid;
        const int k = i < P.n_cov ? cov[i] : -1;
        const int f = k >= 0 ? flags[k] : 3;
        const bool local = !(f & 3);                                                 // :74
        const bool cloud = local && (f & 4);                                         // :231
        if (k >= 0) marks[k] = kBawMarkedLocal | (local ? kBawLocal : 0);            // :73, :75
        int tot;
        const int at = baw_scan_excl((local ? 1 : 0) | (cloud ? 1 << 16 : 0), scan, &tot);   // at most 256 of each
        if (local) {
            list_kf[n_local + (at & 0xffff)] = k;
            if (kf_id[k] == init_id) atomicOr(&sh[0], 1);                            // :85-88
        }
        if (cloud && n_cloud + (at >> 16) < TC2LI_BA_WINDOW_MAX_LIDAR) sh[1 + n_cloud + (at >> 16)] = k;
        n_local += tot & 0xffff;
        n_cloud += tot >> 16;
    }
    __syncthreads();

    // where the slots of every local keyframe start in the concatenation
    int n_slots = 0;
    for (int base = 0; base < n_local; base += kBawThreads) {
        const int i = base + tid;
        int len = 0;
        if (i < n_local) { const int k = list_kf[i]; len = slot_row[k + 1] - slot_row[k]; }
        int tot;
        const int at = baw_scan_excl(len, scan, &tot);
        if (i < n_local) list_start[i] = n_slots + at;
        n_slots += tot;
    }
    __syncthreads();

    // local points (:78-104): the least slot number of every point ...
    for (int li = 0; li < n_local; ++li) {
        const int k = list_kf[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0, q0 = list_start[li];
        for (int s = tid; s < len; s += kBawThreads) {
            const int p = slot_point[s0 + s];
            if (p >= 0 && !(pflags[p] & 3)) atomicMin(&first[p], q0 + s);            // :93-94
        }
    }
    __syncthreads();
    // ... and the slots that hold it, counted in order (:97-101)
    int n_listed = 0;
    for (int li = 0; li < n_local; ++li) {
        const int k = list_kf[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0, q0 = list_start[li];
        for (int base = 0; base < len; base += kBawThreads) {
            const int s = base + tid;
            const int p = s < len ? slot_point[s0 + s] : -1;
            const bool take = p >= 0 && first[p] == q0 + s;                          // only a point that passed :93-94 has a key
            int tot;
            const int at = baw_scan_excl(take ? 1 : 0, scan, &tot);
            if (take) listed[n_listed + at] = p;
            n_listed += tot;
        }
    }
    __syncthreads();

    // fixed cameras (:107-122), and the edges of every listed point counted (:277-345)
    int n_edges = 0, n_without = 0;
    for (int base = 0; base < n_listed; base += kBawThreads) {
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
        const int at = baw_scan_excl(ne, scan, &tot);
        if (i < n_listed) edge_start[i] = n_edges + at;
        n_edges += tot;
        n_without += __syncthreads_count(i < n_listed && ne == 0);
    }
    __syncthreads();

    // the rows that get a pose vertex (:157-187), compacted
    int n_members = 0, n_fixed = 0;
    for (int base = 0; base < P.n_kf; base += kBawThreads) {
        const int k = base + tid;
        const int m = k < P.n_kf ? marks[k] : 0;
        const bool member = (m & (kBawLocal | kBawFixed)) != 0, fixed = (m & kBawFixed) != 0;
        int tot;
        const int at = baw_scan_excl((member ? 1 : 0) | (fixed ? 1 << 16 : 0), scan, &tot);
        if (member) members[n_members + (at & 0xffff)] = k;
        if (k < P.n_kf) kf_pose[k] = -1;
        n_members += tot & 0xffff;
        n_fixed += tot >> 16;
    }
    __syncthreads();
    const int num_fixed = n_fixed + sh[0];                                           // :123
    if (num_fixed == 0) {                                                            // :126-130
        if (tid < TC2LI_BA_WINDOW_COUNTS) counts[tid] = tid == TC2LI_BA_WINDOW_STATUS ? TC2LI_BA_WINDOW_ABORTED : 0;
        if (tid < TC2LI_BA_WINDOW_MAX_LIDAR) B.lidar_pose_index[(size_t)blockIdx.x * TC2LI_BA_WINDOW_MAX_LIDAR + tid] = -1;
        return;
    }
    // vertex-id order: a pose's place is the number of members with a smaller (kf_id, row); members ascend by row
    int32_t* pose_row = B.pose_row + P.pose_off;
    double* poses7_out = B.poses7_out + (size_t)P.pose_off * 7;
    uint8_t* fixed_out = B.fixed + P.pose_off;
    const double* poses7 = B.poses7 + (size_t)P.kf_off * 7;
    for (int i = tid; i < n_members; i += kBawThreads) {
        const int k = members[i];
        const int64_t id = kf_id[k];
        int r = 0;
        for (int j = 0; j < n_members; ++j) {
            const int64_t idj = kf_id[members[j]];
            r += (idj < id || (idj == id && j < i)) ? 1 : 0;
        }
        kf_pose[k] = r;
        if (r < P.pose_cap) {
            pose_row[r] = k;
#pragma unroll
            for (int c = 0; c < 7; ++c) poses7_out[(size_t)r * 7 + c] = poses7[(size_t)k * 7 + c];
            fixed_out[r] = ((marks[k] & kBawFixed) || id == init_id) ? 1 : 0;        // :181, :164
        }
    }
    __syncthreads();   // kf_pose of the BALM keyframes was written by other threads
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
    }
}

__global__ __launch_bounds__(kBawThreads) void k_baw_gather(BawBatch B) {
    __shared__ int marks[kBawLdsKeyframes];
    __shared__ int first[kBawLdsPoints];
    __shared__ int scan[kBawThreads / 64];
    __shared__ int sh[8];
    const BawProblemDev& P = B.problems[blockIdx.x];
    if (P.mark_off < 0 && P.first_off < 0) baw_problem(B, P, marks, first, scan, sh);
    else if (P.mark_off < 0) baw_problem(B, P, marks, B.first_global + P.first_off, scan, sh);
    else if (P.first_off < 0) baw_problem(B, P, B.marks_global + P.mark_off, first, scan, sh);
    else baw_problem(B, P, B.marks_global + P.mark_off, B.first_global + P.first_off, scan, sh);
}

__global__ __launch_bounds__(kBawThreads) void k_baw_edges(BawBatch B) {
    const BawProblemDev& P = B.problems[blockIdx.x];
    const int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_BA_WINDOW_COUNTS;
    const int n_listed = counts[TC2LI_BA_WINDOW_N_POINTS];
    // nothing to write, or a list of the problem does not fit (the host answers TC2LI_ERR_CAPACITY from the counts)
    if (counts[TC2LI_BA_WINDOW_STATUS] != TC2LI_BA_WINDOW_OK || counts[TC2LI_BA_WINDOW_N_POSES] > P.pose_cap || n_listed > P.point_cap ||
        counts[TC2LI_BA_WINDOW_N_EDGES] > P.edge_cap)
        return;
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int32_t* kf_slot = B.kf_slot + P.kf_off;
    const int32_t* kf_pose = B.kf_pose + P.kf_off;
    const int32_t* obs_row = B.obs_offsets + P.point_off + blockIdx.x;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int32_t* obs_index = B.obs_index + P.obs_off;
    const int32_t* listed = B.listed + P.point_off;
    const int32_t* edge_start = B.edge_start + P.point_off;
    const double* positions = B.positions + (size_t)P.point_off * 3;
    int32_t* point_row = B.point_row + P.pointo_off;
    double* points3_out = B.points3_out + (size_t)P.pointo_off * 3;
    tc2li_ba_edge* edges = B.edges + P.edge_off;
    for (int i = blockIdx.y * kBawThreads + threadIdx.x; i < n_listed; i += kBawEdgeBlocks * kBawThreads) {
        const int p = listed[i];
        point_row[i] = p;
#pragma unroll
        for (int c = 0; c < 3; ++c) points3_out[(size_t)i * 3 + c] = positions[(size_t)p * 3 + c];   // :267
        int e = edge_start[i];
        const int o1 = obs_row[p + 1];
        for (int o = obs_row[p]; o < o1; ++o) {
            const int k = obs_kf[o], idx = obs_index[o];
            if ((flags[k] & 3) || idx < 0) continue;                                 // :281, :286, :313
            const uint8_t* slot = B.store.slots + (size_t)kf_slot[k] * B.store.stride;
            const tc2li_keypoint kp = reinterpret_cast<const tc2li_keypoint*>(slot + B.store.keys)[idx];
            const float ur = reinterpret_cast<const float*>(slot + B.store.u_right)[idx];
            tc2li_ba_edge E;
            E.point = i;
            E.pose = kf_pose[k];
            E.u = (double)kp.x;                                                      // :290, :318
            E.v = (double)kp.y;
            E.u_right = ur >= 0.f ? (double)ur : -1.0;
            E.inv_sigma2 = (double)B.inv_level_sigma2[kp.octave];                    // :297, :325
            edges[e++] = E;
        }
    }
}

void launch_ba_window(const BawBatch& B, hipStream_t st) {
    if (B.n_problems <= 0) return;
    TC2LI_LAUNCH(k_baw_gather, dim3(B.n_problems), dim3(kBawThreads), 0, st, B);
    TC2LI_LAUNCH(k_baw_edges, dim3(B.n_problems, kBawEdgeBlocks), dim3(kBawThreads), 0, st, B);
}

}  // namespace tc2li

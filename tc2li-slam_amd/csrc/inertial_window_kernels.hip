// The window of the inertial local BA on gfx950: the graph walk of OptimizerWithLidar::LocalLVIBA (SF/src/OptimizerWithLidar.cc:489-607,
// :632-727, :729-800, :832-969; the same text in Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512-1631 and on) on the flat graph.
// Integer work and copies; no float arithmetic, no MFMA.
//   k_iw_gather    one workgroup per problem, everything whose order matters:
//                  temporal window   one lane follows prev_kf (at most 25 dependent loads, :508-519); every keyframe's marks are one int, in
//                                    LDS up to kIwLdsKeyframes keyframes and in global memory beyond.
//                  points            as in k_baw_gather: the slots of the window keyframes are numbered q = 0, 1, ... in list order, every
//                                    slot does an integer atomicMin of q on its point's key (LDS up to kIwLdsPoints points, global memory
//                                    beyond), the slot that holds the minimum is the first occurrence (:533-537), a block prefix sum over those
//                                    in q order is the place in lLocalMapPoints.
//                  fixed keyframe    :542-554, one lane.
//                  fixed observers   :586-607 is sequential -- a point's pick depends on the marks every earlier point left.  Wavefront 0
//                                    takes the listed points 64 at a time: every lane finds its point's first unmarked observer under the marks
//                                    as they stand (the loads of 64 points in flight together); the chunk is then resolved in lane order: the
//                                    lowest lane that still has a pick marks it (ballot, readlane), the lanes whose pick was that keyframe
//                                    move on to their next unmarked observer.  A lane's pick is therefore always its first unmarked observer
//                                    under the marks of all earlier points, which is what the sequential walk sees.  A bad pick is marked and
//                                    its lane, still the lowest, comes again with the next observer (:598 fails, no break).  The count stops
//                                    the walk at 200 after the point that reached it (:605).
//                  edges counted     a thread per listed point (:862-865); the keyframe's mVisEdges by atomicAdd in its marks.
//                  vertices          the marked rows compacted, then ranked by (kf_id, row) (at most 225).
//                  links, LiDAR      wavefront 0, a lane per window keyframe, placed by ballot (:734-800, :710-721).
//   k_iw_edges     kIwEdgeBlocks workgroups per problem, a thread per listed point: its row and position, and one edge per observation
//                  from the first edge on, the pixel read from the observer's slot of the keyframe store.
// Helpers with a barrier inside (iw_scan_excl, __syncthreads_count) are only called where all 256 threads arrive.
#include "inertial_window_device.hpp"
#include "launch.hpp"

namespace tc2li {

static_assert(sizeof(tc2li_inertial_keyframe) == 33 * sizeof(double), "keyframes are copied as 33 doubles");
constexpr int kIwStateDoubles = 33;
constexpr int kIwMaxFixed = TC2LI_INERTIAL_WINDOW_MAX_FIXED;

// Exclusive prefix sum of v over the workgroup's kIwThreads threads, the total in *total.  lds: 4 ints.
__device__ __forceinline__ int iw_scan_excl(int v, int* lds, int* total) {
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
    for (int k = 0; k < kIwThreads / 64; ++k) {
        const int s = lds[k];
        if (k < w) base += s;
        tot += s;
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// a mark as the other lanes of the wavefront left it
__device__ __forceinline__ int iw_mark(const int* m) { return __hip_atomic_load(m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

// :586-607 by wavefront 0, all 64 lanes active.  n_fixed: lFixedKeyFrames.size() on entry (1).  Returns it on exit.
__device__ __forceinline__ int iw_fixed_observers(int* marks, const uint8_t* flags, const int32_t* obs_row, const int32_t* obs_kf,
                                                  const int32_t* listed, int n_listed, int n_fixed) {
    const int lane = threadIdx.x;
    for (int base = 0; base < n_listed && n_fixed < kIwMaxFixed; base += 64) {
        const int i = base + lane;
        int o = 0, o1 = 0;
        if (i < n_listed) {
            const int p = listed[i];
            o = obs_row[p];
            o1 = obs_row[p + 1];
        }
        int pick = -1, pick_bad = 0;
        // the lane's first observer from o on that carries neither mark (:595)
        auto next_unmarked = [&]() {
            pick = -1;
            for (; o < o1; ++o) {
                const int k = obs_kf[o];
                if (!(iw_mark(&marks[k]) & (kIwLocal | kIwFixedMark))) {
                    pick = k;
                    pick_bad = flags[k] & 1;
                    break;
                }
            }
        };
        next_unmarked();
        unsigned long long pending = __ballot(pick >= 0);
        while (pending) {
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(pending));   // the earliest point that still has an observer to mark
            const int k = __builtin_amdgcn_readlane(pick, l), bad = __builtin_amdgcn_readlane(pick_bad, l);
            if (lane == l) atomicOr(&marks[k], kIwFixedMark | (bad ? 0 : kIwFixedList));   // :597, :598-600
            __threadfence_block();
            n_fixed += bad ? 0 : 1;
            const bool mine = pick == k;
            if (mine && lane == l && !bad) pick = -1;                                  // :601: the point is done
            else if (mine) next_unmarked();                                            // its pick is marked now: the point's next observer
            if (n_fixed >= kIwMaxFixed) break;                                         // :605, after the point that reached it
            pending = __ballot(pick >= 0);
        }
    }
    return n_fixed;
}

// marks / first: the problem's keyframe marks and first-occurrence keys, LDS or global (the address space is known after inlining)
// sh: [0 .. 25) vpOptimizableKFs as rows, [25] its size before :553, [26] N after, [27] lFixedKeyFrames.size()
__device__ __forceinline__ void iw_problem(const IwBatch& B, const IwProblemDev& P, int* marks, int* first, int* scan, int* sh) {
    const int tid = threadIdx.x;
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int64_t* kf_id = B.kf_id + P.kf_off;
    const int32_t* prev = B.prev_kf + P.kf_off;
    const int32_t* slot_row = B.slot_offsets + P.kf_off + blockIdx.x;
    const int32_t* slot_point = B.slot_point + P.slot_off;
    const uint8_t* pflags = B.point_flags + P.point_off;
    const int32_t* obs_row = B.obs_offsets + P.point_off + blockIdx.x;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int32_t* obs_index = B.obs_index + P.obs_off;
    int32_t* listed = B.listed + P.point_off;
    int32_t* edge_start = B.edge_start + P.point_off;
    int32_t* kf_vertex = B.kf_vertex + P.kf_off;
    int32_t* members = B.members + P.kf_off;
    int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_INERTIAL_WINDOW_COUNTS;
    int32_t* lidar = B.lidar_pose_index + (size_t)blockIdx.x * TC2LI_INERTIAL_WINDOW_MAX_LIDAR;
    int* win = sh;

    for (int k = tid; k < P.n_kf; k += kIwThreads) marks[k] = 0;
    for (int p = tid; p < P.n_points; p += kIwThreads) first[p] = 0x7fffffff;
    __syncthreads();

    // temporal window (:508-519); the host has made sure that the chain names no row twice
    if (tid == 0) {
        int n = 0;
        win[n++] = P.current;                                                        // :508
        marks[P.current] = kIwLocal;                                                 // :509
        for (int i = 1; i < P.nd; ++i) {                                             // :510
            const int pr = prev[win[n - 1]];
            if (pr < 0) break;                                                       // :512, :518
            win[n++] = pr;                                                           // :514
            marks[pr] = kIwLocal;                                                    // :515
        }
        sh[25] = n;
    }
    __syncthreads();
    const int n_win = sh[25];

    // points (:524-539): the least slot number of every point ...
    int q0 = 0;
    for (int li = 0; li < n_win; ++li) {
        const int k = win[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0;
        for (int s = tid; s < len; s += kIwThreads) {
            const int p = slot_point[s0 + s];
            if (p >= 0 && !(pflags[p] & 1)) atomicMin(&first[p], q0 + s);            // :531-532
        }
        q0 += len;
    }
    __syncthreads();
    // ... and the slots that hold it, counted in order (:533-537)
    int n_listed = 0;
    q0 = 0;
    for (int li = 0; li < n_win; ++li) {
        const int k = win[li];
        const int s0 = slot_row[k], len = slot_row[k + 1] - s0;
        for (int base = 0; base < len; base += kIwThreads) {
            const int s = base + tid;
            const int p = s < len ? slot_point[s0 + s] : -1;
            const bool take = p >= 0 && first[p] == q0 + s;                          // only a point that passed :531-532 has a key
            int tot;
            const int at = iw_scan_excl(take ? 1 : 0, scan, &tot);
            if (take) listed[n_listed + at] = p;
            n_listed += tot;
        }
        q0 += len;
    }

    // fixed keyframe (:542-554)
    if (tid == 0) {
        const int last = win[n_win - 1], pr = prev[last];
        if (pr >= 0) {
            marks[pr] = kIwFixedMark | kIwFixedList;                                 // :545-546
            sh[26] = n_win;
        } else {
            marks[last] = kIwFixedMark | kIwFixedList;                               // :550-552
            sh[26] = n_win - 1;                                                      // :553
        }
    }
    __syncthreads();   // and `listed` is complete
    const int N = sh[26];
    if (N == 0) {
        if (tid < TC2LI_INERTIAL_WINDOW_COUNTS)
            counts[tid] = tid == TC2LI_INERTIAL_WINDOW_STATUS ? TC2LI_INERTIAL_WINDOW_EMPTY : tid == TC2LI_INERTIAL_WINDOW_N_FIXED_KF ? 1 : 0;
        if (tid < TC2LI_INERTIAL_WINDOW_MAX_LIDAR) lidar[tid] = -1;
        return;
    }

    // fixed observers (:586-607)
    if (tid < 64) {
        const int n = iw_fixed_observers(marks, flags, obs_row, obs_kf, listed, n_listed, 1);
        if (tid == 0) sh[27] = n;
    }
    __syncthreads();
    const int n_fixed = sh[27];

    // the edges of every listed point counted (:858-931), and mVisEdges of every keyframe
    int n_edges = 0, n_without = 0;
    for (int base = 0; base < n_listed; base += kIwThreads) {
        const int i = base + tid;
        int ne = 0;
        if (i < n_listed) {
            const int p = listed[i];
            const int o1 = obs_row[p + 1];
            for (int o = obs_row[p]; o < o1; ++o) {
                const int k = obs_kf[o];
                if (!(marks[k] & (kIwLocal | kIwFixedMark)) || (flags[k] & 3) || obs_index[o] < 0) continue;   // :862, :865, :872, :902
                atomicAdd(&marks[k], 1 << kIwEdgeShift);                             // :874, :905
                ++ne;
            }
        }
        int tot;
        const int at = iw_scan_excl(ne, scan, &tot);
        if (i < n_listed) edge_start[i] = n_edges + at;
        n_edges += tot;
        n_without += __syncthreads_count(i < n_listed && ne == 0);
    }
    __syncthreads();

    // the rows that get a vertex (:632-696), compacted
    int n_members = 0, n_under3 = 0;
    for (int base = 0; base < P.n_kf; base += kIwThreads) {
        const int k = base + tid;
        const int m = k < P.n_kf ? marks[k] : 0;
        const bool member = (m & (kIwLocal | kIwFixedList)) != 0;
        int tot;
        const int at = iw_scan_excl(member ? 1 : 0, scan, &tot);
        if (member) members[n_members + at] = k;
        if (k < P.n_kf) kf_vertex[k] = -1;
        n_members += tot;
        n_under3 += __syncthreads_count(member && (m >> kIwEdgeShift) < 3);           // :972-975
    }
    __syncthreads();
    // vertex-id order: a vertex's place is the number of members with a smaller (kf_id, row); members ascend by row
    int32_t* kf_row = B.kf_row + P.vertex_off;
    uint8_t* fixed_out = B.fixed + P.vertex_off;
    uint8_t* has_imu = B.has_imu + P.vertex_off;
    for (int i = tid; i < n_members; i += kIwThreads) {
        const int k = members[i];
        const int64_t id = kf_id[k];
        int r = 0;
        for (int j = 0; j < n_members; ++j) {
            const int64_t idj = kf_id[members[j]];
            r += (idj < id || (idj == id && j < i)) ? 1 : 0;
        }
        kf_vertex[k] = r;
        if (r < P.vertex_cap) {
            kf_row[r] = k;
            fixed_out[r] = (marks[k] & kIwFixedList) ? 1 : 0;                        // :640, :678
            has_imu[r] = (flags[k] & 4) ? 1 : 0;                                     // :643, :681
        }
    }
    __syncthreads();   // kf_vertex was written by other threads
    const double* states = B.states + (size_t)P.kf_off * kIwStateDoubles;
    double* states_out = B.keyframes_out + (size_t)P.vertex_off * kIwStateDoubles;
    for (int e = tid; e < n_members * kIwStateDoubles; e += kIwThreads) {
        const int i = e / kIwStateDoubles, c = e - i * kIwStateDoubles;
        const int k = members[i], r = kf_vertex[k];
        if (r < P.vertex_cap) states_out[(size_t)r * kIwStateDoubles + c] = states[(size_t)k * kIwStateDoubles + c];
    }
    const int n_lidar = (P.with_lidar && N > 5) ? TC2LI_INERTIAL_WINDOW_MAX_LIDAR : 0;   // :710-712
    if (tid < TC2LI_INERTIAL_WINDOW_MAX_LIDAR) lidar[tid] = tid < n_lidar ? kf_vertex[win[tid]] : -1;   // :717-720
    // links (:734-800): a lane per window keyframe, kept in order
    if (tid < 64) {
        bool ok = false;
        int k = -1, pr = -1;
        if (tid < N) {
            k = win[tid];
            pr = prev[k];                                                            // :738
            ok = pr >= 0 && (flags[k] & 4) && (flags[pr] & 4) && (flags[k] & 8);     // :743
        }
        const unsigned long long mask = __ballot(ok);
        const int at = __popcll(mask & ((1ull << tid) - 1));
        if (ok && at < P.link_cap) {
            tc2li_inertial_link L;
            L.kf1 = kf_vertex[pr];                                                   // :746
            L.kf2 = kf_vertex[k];                                                    // :750
            L.robust = (tid == N - 1 || P.rec_init) ? 1 : 0;                         // :770
            L.pad_ = 0;
            L.info_scale = tid == N - 1 ? 1e-2 : 1.0;                                // :778-779
            L.preintegrated = nullptr;
            B.links[(size_t)blockIdx.x * kIwMaxOpt + at] = L;
            B.link_kf2_row[(size_t)blockIdx.x * kIwMaxOpt + at] = k;
        }
        if (tid == 0) {
            counts[TC2LI_INERTIAL_WINDOW_STATUS] = TC2LI_INERTIAL_WINDOW_OK;
            counts[TC2LI_INERTIAL_WINDOW_N_FIXED_KF] = n_fixed;
            counts[TC2LI_INERTIAL_WINDOW_N_OPT_KF] = N;
            counts[TC2LI_INERTIAL_WINDOW_N_VERTICES] = n_members;
            counts[TC2LI_INERTIAL_WINDOW_N_POINTS] = n_listed;
            counts[TC2LI_INERTIAL_WINDOW_N_EDGES] = n_edges;
            counts[TC2LI_INERTIAL_WINDOW_N_LINKS] = __popcll(mask);
            counts[TC2LI_INERTIAL_WINDOW_N_LIDAR] = n_lidar;
            counts[TC2LI_INERTIAL_WINDOW_N_POINTS_WITHOUT_EDGE] = n_without;
            counts[TC2LI_INERTIAL_WINDOW_N_VERTICES_UNDER_3_EDGES] = n_under3;
        }
    }
}

__global__ __launch_bounds__(kIwThreads) void k_iw_gather(IwBatch B) {
    __shared__ int marks[kIwLdsKeyframes];
    __shared__ int first[kIwLdsPoints];
    __shared__ int scan[kIwThreads / 64];
    __shared__ int sh[32];
    const IwProblemDev& P = B.problems[blockIdx.x];
    if (P.mark_off < 0 && P.first_off < 0) iw_problem(B, P, marks, first, scan, sh);
    else if (P.mark_off < 0) iw_problem(B, P, marks, B.first_global + P.first_off, scan, sh);
    else if (P.first_off < 0) iw_problem(B, P, B.marks_global + P.mark_off, first, scan, sh);
    else iw_problem(B, P, B.marks_global + P.mark_off, B.first_global + P.first_off, scan, sh);
}

__global__ __launch_bounds__(kIwThreads) void k_iw_edges(IwBatch B) {
    const IwProblemDev& P = B.problems[blockIdx.x];
    const int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_INERTIAL_WINDOW_COUNTS;
    const int n_listed = counts[TC2LI_INERTIAL_WINDOW_N_POINTS];
    // nothing to write, or a list of the problem does not fit (the host answers TC2LI_ERR_CAPACITY from the counts)
    if (counts[TC2LI_INERTIAL_WINDOW_STATUS] != TC2LI_INERTIAL_WINDOW_OK || counts[TC2LI_INERTIAL_WINDOW_N_VERTICES] > P.vertex_cap ||
        n_listed > P.point_cap || counts[TC2LI_INERTIAL_WINDOW_N_EDGES] > P.edge_cap || counts[TC2LI_INERTIAL_WINDOW_N_LINKS] > P.link_cap)
        return;
    const uint8_t* flags = B.kf_flags + P.kf_off;
    const int32_t* kf_slot = B.kf_slot + P.kf_off;
    const int32_t* kf_vertex = B.kf_vertex + P.kf_off;
    const int32_t* obs_row = B.obs_offsets + P.point_off + blockIdx.x;
    const int32_t* obs_kf = B.obs_kf + P.obs_off;
    const int32_t* obs_index = B.obs_index + P.obs_off;
    const int32_t* listed = B.listed + P.point_off;
    const int32_t* edge_start = B.edge_start + P.point_off;
    const double* positions = B.positions + (size_t)P.point_off * 3;
    int32_t* point_row = B.point_row + P.pointo_off;
    double* points3_out = B.points3_out + (size_t)P.pointo_off * 3;
    tc2li_ba_edge* edges = B.edges + P.edge_off;
    for (int i = blockIdx.y * kIwThreads + threadIdx.x; i < n_listed; i += kIwEdgeBlocks * kIwThreads) {
        const int p = listed[i];
        point_row[i] = p;
#pragma unroll
        for (int c = 0; c < 3; ++c) points3_out[(size_t)i * 3 + c] = positions[(size_t)p * 3 + c];   // :849
        int e = edge_start[i];
        const int o1 = obs_row[p + 1];
        for (int o = obs_row[p]; o < o1; ++o) {
            const int k = obs_kf[o], idx = obs_index[o];
            // a keyframe that is neither bad nor of another map has a vertex exactly when it carries one of the two marks (:862, :865)
            if (kf_vertex[k] < 0 || (flags[k] & 3) || idx < 0) continue;
            const uint8_t* slot = B.store.slots + (size_t)kf_slot[k] * B.store.stride;
            const tc2li_keypoint kp = reinterpret_cast<const tc2li_keypoint*>(slot + B.store.keys)[idx];
            const float ur = reinterpret_cast<const float*>(slot + B.store.u_right)[idx];
            tc2li_ba_edge E;
            E.point = i;
            E.pose = kf_vertex[k];
            E.u = (double)kp.x;                                                      // :876-878, :904-909
            E.v = (double)kp.y;
            E.u_right = ur >= 0.f ? (double)ur : -1.0;                               // :872, :902
            E.inv_sigma2 = (double)B.inv_level_sigma2[kp.octave];                    // :889, :920
            edges[e++] = E;
        }
    }
}

void launch_inertial_window(const IwBatch& B, hipStream_t st) {
    if (B.n_problems <= 0) return;
    TC2LI_LAUNCH(k_iw_gather, dim3(B.n_problems), dim3(kIwThreads), 0, st, B);
    TC2LI_LAUNCH(k_iw_edges, dim3(B.n_problems, kIwEdgeBlocks), dim3(kIwThreads), 0, st, B);
}

}  // namespace tc2li

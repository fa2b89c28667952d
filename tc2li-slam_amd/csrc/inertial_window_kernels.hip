// The window of the inertial local BA on gfx950: the graph walk of OptimizerWithLidar::LocalLVIBA (SF/src/OptimizerWithLidar.cc:489-607,
// :632-727, :729-800, :832-969; the same text in Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512-1631 and on) on the flat graph.
// Integer work and copies; no float arithmetic, no MFMA.
//   k_iw_gather    one workgroup per problem, everything whose order matters:
//                  temporal window   one lane follows prev_kf (at most 25 dependent loads, :508-519); every keyframe's marks are one int, in
//                                    LDS up to kWinLdsKeyframes keyframes and in global memory beyond.
//                  points            window_list_points over the window keyframes (:524-539): first occurrences by an integer atomicMin on
//                                    the point's key (LDS up to kWinLdsPoints points, global memory beyond) and a block prefix sum.
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
//                  vertices          the marked rows compacted, then ranked by (kf_id, row) (at most 225; window_compact_members,
//                                    window_rank_members).
//                  links, LiDAR      wavefront 0, a lane per window keyframe, placed by ballot (:734-800, :710-721).
//   k_window_edges the points and edges, by the kernel that also ends the visual gather (ba_window_kernels.hip).
// The listing, the compaction, the ranking and the LDS / global dispatch are window_gather_device.hpp's, shared with the visual gather.
// Helpers with a barrier inside are only called where all 256 threads arrive (block_scan_excl in launch.hpp says what that takes).
#include "inertial_window_device.hpp"

namespace tc2li {

static_assert(sizeof(tc2li_inertial_keyframe) == 33 * sizeof(double), "keyframes are copied as 33 doubles");
constexpr int kIwStateDoubles = 33;
constexpr int kIwMaxFixed = TC2LI_INERTIAL_WINDOW_MAX_FIXED;

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
    const uint8_t* flags = B.kf_flags + P.t_kf;
    const int64_t* kf_id = B.kf_id + P.t_kf;
    const int32_t* prev = B.prev_kf + P.kf_off;
    const int32_t* slot_row = B.slot_offsets + P.slot_row;
    const int32_t* slot_point = B.slot_point + P.t_slot;
    const uint8_t* pflags = B.point_flags + P.t_point;
    const int32_t* obs_row = B.obs_offsets + P.obs_row;
    const int32_t* obs_kf = B.obs_kf + P.t_obs;
    const int32_t* obs_index = B.obs_index + P.t_obs;
    int32_t* listed = B.listed + P.point_off;
    int32_t* edge_start = B.edge_start + P.point_off;
    int32_t* kf_vertex = B.vertex_of + P.kf_off;
    int32_t* members = B.members + P.kf_off;
    int32_t* counts = B.counts + (size_t)blockIdx.x * TC2LI_INERTIAL_WINDOW_COUNTS;
    int32_t* lidar = B.lidar_pose_index + (size_t)blockIdx.x * TC2LI_INERTIAL_WINDOW_MAX_LIDAR;
    int* win = sh;

    for (int k = tid; k < P.n_kf; k += kWinThreads) marks[k] = 0;
    for (int p = tid; p < P.n_points; p += kWinThreads) first[p] = 0x7fffffff;
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

    // points (:524-539): a bad point is passed over (:531-532), the others are listed once (:533-537)
    const int n_listed = window_list_points(win, n_win, slot_row, slot_point, pflags, 1, first, listed, scan);

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
        if (tid == 0) B.n_emit[blockIdx.x] = 0;
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
    for (int base = 0; base < n_listed; base += kWinThreads) {
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
        const int at = block_scan_excl<kWinThreads>(ne, scan, &tot);
        if (i < n_listed) edge_start[i] = n_edges + at;
        n_edges += tot;
        n_without += __syncthreads_count(i < n_listed && ne == 0);
    }
    __syncthreads();

    // the rows that get a vertex (:632-696), compacted, and those with mVisEdges < 3 counted (:972-975)
    int n_under3;
    const int n_members = window_compact_members(marks, P.n_kf, members, kf_vertex, scan, &n_under3, [](int m) {
        const bool member = (m & (kIwLocal | kIwFixedList)) != 0;
        return (member ? 1 : 0) | ((member && (m >> kIwEdgeShift) < 3) ? 1 << 16 : 0);
    });
    // vertex-id order
    int32_t* kf_row = B.kf_row + P.vertex_off;
    uint8_t* fixed_out = B.fixed + P.vertex_off;
    uint8_t* has_imu = B.has_imu + P.vertex_off;
    window_rank_members(kf_id, members, n_members, kf_vertex, P.vertex_cap, [&](int k, int r, int64_t) {
        kf_row[r] = k;
        fixed_out[r] = (marks[k] & kIwFixedList) ? 1 : 0;                            // :640, :678
        has_imu[r] = (flags[k] & 4) ? 1 : 0;                                         // :643, :681
    });
    const double* states = B.states + (size_t)P.kf_off * kIwStateDoubles;
    double* states_out = B.keyframes_out + (size_t)P.vertex_off * kIwStateDoubles;
    for (int e = tid; e < n_members * kIwStateDoubles; e += kWinThreads) {
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
            B.n_emit[blockIdx.x] =
                (n_members <= P.vertex_cap && n_listed <= P.point_cap && n_edges <= P.edge_cap && __popcll(mask) <= P.link_cap) ? n_listed : 0;
        }
    }
}

__global__ __launch_bounds__(kWinThreads) void k_iw_gather(IwBatch B) {
    __shared__ int marks[kWinLdsKeyframes];
    __shared__ int first[kWinLdsPoints];
    __shared__ int scan[kWinThreads / 64];
    __shared__ int sh[32];
    const IwProblemDev& P = window_problem<IwProblemDev>(B, blockIdx.x);
    window_dispatch(B, P, marks, first, [&](int* m, int* f) __attribute__((always_inline)) { iw_problem(B, P, m, f, scan, sh); });
}

void launch_inertial_window(const IwBatch& B, hipStream_t st) {
    if (B.n_problems <= 0) return;
    TC2LI_LAUNCH(k_iw_gather, dim3(B.n_problems), dim3(kWinThreads), 0, st, B);
    launch_window_edges(B, st);
}

}  // namespace tc2li

// MLPnP RANSAC on gfx950: every iteration a batch of iterate() calls may run is evaluated at once, then each problem picks in order.
//   k_mlpnp_solve    one lane per (problem, iteration): computePose on the six drawn points in f64.  The two 12 x 12 matrices of the
//                    decomposition and every other array indexed at run time sit in the lane's column of an LDS tile (288 doubles per
//                    lane, lane-fastest: a wavefront's access to one element is 512 contiguous bytes, no bank conflict), so the kernel
//                    uses no private memory; one wavefront per workgroup, one workgroup per CU.  Fewer lanes per wavefront with more
//                    wavefronts per CU (32, 16, 8 lanes measured) take the same time: the kernel is bound by the number of LDS
//                    instructions, and each moves most with all 64 lanes active.
//   k_mlpnp_inliers  one wavefront per (problem, iteration): CheckInliers over the problem's N correspondences, 64 per step, flags kept as
//                    ballot words, the count by popcount.
//   k_mlpnp_select   one workgroup per problem: the loop of iterate() over the counts, then the state, the flags scattered to frame
//                    keypoints and the pose.
#include "mlpnp_device.hpp"
#include "mlpnp_math.hpp"
#include "launch.hpp"

namespace tc2li {

constexpr int kSolveLanes = 64;
constexpr int kSolveLds = kSolveLanes * mlpnp::kWsDoubles * (int)sizeof(double);

__global__ __launch_bounds__(kSolveLanes) void k_mlpnp_solve(MlpnpBatch B) {
    extern __shared__ double mlpnp_tile[];
    const int g = blockIdx.x * kSolveLanes + threadIdx.x;
    if (g >= B.n_solves) return;
    const MlpnpProblemDev& P = B.problems[B.problem_of_solve[g]];
    const mlpnp::Corr c = {B.p2d + 2 * (size_t)P.corr_off, B.Xw + 3 * (size_t)P.corr_off, B.fx, B.fy, B.cx, B.cy};
    double Rt[12];
    mlpnp::compute_pose6(c, B.idx6 + 6 * (size_t)g, mlpnp::Ws{mlpnp_tile + threadIdx.x, kSolveLanes}, Rt);
#pragma unroll
    for (int i = 0; i < 12; ++i) B.Rt[12 * (size_t)g + i] = Rt[i];
}

__global__ __launch_bounds__(256) void k_mlpnp_inliers(MlpnpBatch B) {
    const int g = blockIdx.x * 4 + wave_in_block();
    if (g >= B.n_solves) return;
    const int lane = threadIdx.x & 63;
    const MlpnpProblemDev& P = B.problems[B.problem_of_solve[g]];
    const mlpnp::Corr c = {B.p2d + 2 * (size_t)P.corr_off, B.Xw + 3 * (size_t)P.corr_off, B.fx, B.fy, B.cx, B.cy};
    const float* max_error = B.max_error + P.corr_off;
    double Rt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Rt[i] = B.Rt[12 * (size_t)g + i];
    int count = 0;
    for (int base = 0, w = 0; base < P.n_corr; base += 64, ++w) {
        const int i = base + lane;
        const bool in = i < P.n_corr && mlpnp::is_inlier(c, i, Rt, max_error[i]);
        const unsigned long long m = __ballot(in);
        count += __popcll(m);
        if (lane == 0) B.mask[(size_t)g * B.mask_words + w] = m;
    }
    if (lane == 0) B.count[g] = count;
}

__global__ __launch_bounds__(64) void k_mlpnp_select(MlpnpBatch B) {
    const int p = blockIdx.x, lane = threadIdx.x;
    const MlpnpProblemDev& P = B.problems[p];
    __shared__ mlpnp::Selection sel;
    if (lane == 0) {
        const int32_t* count = B.count + P.it_off;
        sel = mlpnp::select(P.n_corr, P.min_inliers, P.max_its, P.n_iterations, P.st_iterations, P.st_best, [count](int j) { return count[j]; });
    }
    __syncthreads();
    const mlpnp::Selection s = sel;
    uint8_t* inlier = B.inlier + (size_t)p * B.capacity;
    uint8_t* best = B.best_inlier + (size_t)p * B.capacity;
    const int32_t* kp = B.kp_index + P.corr_off;
    for (int k = lane; k < B.capacity; k += 64) inlier[k] = 0;
    if (s.best >= 0)
        for (int k = lane; k < P.n_keypoints; k += 64) best[k] = 0;
    __syncthreads();
    if (s.best >= 0) {
        const unsigned long long* m = B.mask + (size_t)(P.it_off + s.best) * B.mask_words;
        for (int i = lane; i < P.n_corr; i += 64)
            if ((m[i >> 6] >> (i & 63)) & 1ull) best[kp[i]] = 1;
    }
    if (s.ret >= 0) {
        const unsigned long long* m = B.mask + (size_t)(P.it_off + s.ret) * B.mask_words;
        for (int i = lane; i < P.n_corr; i += 64)
            if ((m[i >> 6] >> (i & 63)) & 1ull) inlier[kp[i]] = 1;
    }
    __syncthreads();
    if (s.ret == -1)
        for (int k = lane; k < P.n_keypoints; k += 64) inlier[k] = best[k];
    if (lane == 0) {
        MlpnpStateOut so;
        so.iterations = s.iterations; so.best_inliers = s.best_inliers;
#pragma unroll
        for (int i = 0; i < 12; ++i) so.best_Tcw[i] = s.best >= 0 ? (float)B.Rt[12 * (size_t)(P.it_off + s.best) + i] : P.st_Tcw[i];
        B.state[p] = so;
        double Rt[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};   // Tout.setIdentity() (:81)
        const int src = s.ret >= 0 ? s.ret : s.best;
        if (s.ret >= 0 || (s.ret == -1 && s.best >= 0)) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Rt[i] = B.Rt[12 * (size_t)(P.it_off + src) + i];
        } else if (s.ret == -1) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Rt[i] = (double)P.st_Tcw[i];
        }
        float pose7[7];
        mlpnp::pose7_of(Rt, pose7);
#pragma unroll
        for (int i = 0; i < 7; ++i) B.pose7[7 * (size_t)p + i] = pose7[i];
#pragma unroll
        for (int i = 0; i < 12; ++i) B.Rt12[12 * (size_t)p + i] = Rt[i];
        B.result[4 * p] = s.found; B.result[4 * p + 1] = s.no_more; B.result[4 * p + 2] = s.n_inliers; B.result[4 * p + 3] = s.ret;
    }
}

bool launch_mlpnp(const MlpnpBatch& B, hipStream_t st) {
    if (B.n_solves > 0) {
        if (!ensure_dynamic_lds(reinterpret_cast<const void*>(k_mlpnp_solve), kSolveLds)) return false;
        TC2LI_LAUNCH(k_mlpnp_solve, dim3((B.n_solves + kSolveLanes - 1) / kSolveLanes), dim3(kSolveLanes), kSolveLds, st, B);
        TC2LI_LAUNCH(k_mlpnp_inliers, dim3((B.n_solves + 3) / 4), dim3(256), 0, st, B);
    }
    if (B.n_problems > 0) TC2LI_LAUNCH(k_mlpnp_select, dim3(B.n_problems), dim3(64), 0, st, B);
    return true;
}

}  // namespace tc2li

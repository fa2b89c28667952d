// Device side of tc2li_mlpnp_ransac_batch (include/tc2li_hip.h "MLPnP RANSAC"): mlpnp_host.cpp packs the problems and draws the minimal
// sets, mlpnp_kernels.hip solves every iteration a call may run, tests every correspondence against every pose and selects in order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tc2li {

// One problem = one MLPnPsolver::iterate call.  Correspondences and iterations of all problems are concatenated.
struct MlpnpProblemDev {
    int32_t corr_off, n_corr;          // N and where its correspondences start
    int32_t it_off, n_it;              // the iterations the call may run (0 when N < min_inliers) and where they start
    int32_t min_inliers, max_its;      // mRansacMinInliers, mRansacMaxIts after SetRansacParameters
    int32_t n_iterations;              // iterate()'s argument
    int32_t n_keypoints;
    int32_t st_iterations, st_best;    // mnIterations, mnBestInliers on entry
    float st_Tcw[12];                  // mBestTcw on entry
};
struct MlpnpStateOut { int32_t iterations, best_inliers; float best_Tcw[12]; };

struct MlpnpBatch {
    int n_problems, n_solves, capacity, mask_words;
    float fx, fy, cx, cy;
    const MlpnpProblemDev* problems;
    const float* p2d;                  // [corr][2]
    const float* Xw;                   // [corr][3]
    const float* max_error;            // [corr] mvMaxError
    const int32_t* kp_index;           // [corr] mvKeyPointIndices
    const int32_t* idx6;               // [n_solves][6] the minimal set of every iteration
    const int32_t* problem_of_solve;   // [n_solves]
    double* Rt;                        // [n_solves][12]
    int32_t* count;                    // [n_solves] mnInliersi
    unsigned long long* mask;          // [n_solves][mask_words] mvbInliersi
    // out
    int32_t* result;                   // [n_problems][4] found, no_more, n_inliers, -
    MlpnpStateOut* state;              // [n_problems]
    float* pose7;                      // [n_problems][7]
    double* Rt12;                      // [n_problems][12]
    uint8_t* inlier;                   // [n_problems][capacity]
    uint8_t* best_inlier;              // [n_problems][capacity] in: the state's flags, out: the new state's
};
// false: the runtime refused the solve kernel's LDS
bool launch_mlpnp(const MlpnpBatch& B, hipStream_t st);

}  // namespace tc2li

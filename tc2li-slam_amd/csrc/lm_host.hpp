// g2o's Levenberg-Marquardt control (Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-169) with the reference's `_nBad >= 3`
// rule, as every host loop of the project runs it: ba_host.cpp, the lock-step drivers' host form (ba_lockstep.cpp, lvi_host.cpp), the
// one-window inertial entry and imu_init_host.cpp.  Host only (no .hip includes it); the device has its own copies (ba_lm_kernels.hip,
// pose_opt_kernel.hip, imu_init_kernels.hip, pose_inertial_kernel.hip), operation for operation the same.
//
//   for (it ...; lm.ok && !stopped) {
//       linearise;  lm.begin_iteration(chi, it == 0, lambda of computeLambdaInit or the caller's);
//       do { solve at lm.lambda, trial estimate;  if (lm.decide(solved, trial chi, scale)) swap the accepted and the trial buffers; }
//       while (lm.try_again(stopped));
//       lm.end_iteration();
//   }
#pragma once
#include <cfloat>
#include <cmath>
#include "ba_math.hpp"

namespace tc2li {

struct LmHost {
    double lambda = -1, ni = 2, currentChi = 0, tempChi = 0, iniChi = 0, rho = 0;
    int qmax = 0, n_bad = 0, done = 0, trials_total = 0;
    bool ok = true;   // false: the loop ends (ten rejected trials, a step that changes nothing, three iterations below 1e-3 of chi2)

    void begin_iteration(double chi, bool first, double lambda_for_first) {
        tempChi = iniChi = currentChi = chi;
        if (first) { lambda = lambda_for_first; ni = 2; n_bad = 0; }
        rho = 0;
        qmax = 0;
    }
    // the gain ratio and the damping update of one trial; scale: computeScale() without its 1e-3.  Returns whether the step was accepted
    // (the caller then swaps its buffers).  accepted: lambda after an accepted step (imu_init_host.cpp keeps libm's pow in it).
    bool decide(bool solved, double trial_chi, double scale, double (*accepted)(double, double) = lm_lambda_accepted) {
        tempChi = solved ? trial_chi : DBL_MAX;
        rho = currentChi - tempChi;
        scale += 1e-3;
        rho /= scale;
        const bool accept = rho > 0 && std::isfinite(tempChi);
        if (accept) {
            lambda = accepted(lambda, rho);
            ni = 2;
            currentChi = tempChi;
        } else {
            lambda *= ni;
            ni *= 2;
        }
        ++qmax;
        ++trials_total;
        return accept;
    }
    bool try_again(bool stopped) const { return rho < 0 && qmax < 10 && !stopped; }
    void end_iteration() {
        ++done;
        if (qmax == 10 || rho == 0) { ok = false; return; }
        if ((iniChi - currentChi) * 1e3 < iniChi) n_bad++; else n_bad = 0;
        if (n_bad >= 3) ok = false;
    }
};

}  // namespace tc2li

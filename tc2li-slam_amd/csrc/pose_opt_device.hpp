// Shared between the host orchestration and the pose-optimisation kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ba_math.hpp"

namespace tc2li {

struct PoseProblem { int32_t edge_off, n; };  // one frame: its correspondences are edges[edge_off .. edge_off + n)

// What the caller knows of the launch's values -- every map point coordinate and every u, v, ur, info: kUnknown: doubles of any kind;
// otherwise each is a float's value ((double)(float)x == x) and the correspondences may be held in LDS as floats (33 bytes each instead
// of 61; the same bits come out) -- kChecked: launch_pose_inputs_float_exact said so for these very buffers; kByConstruction: the caller's
// own kernel widened floats (the tracking batches).
enum class PoseFloats { kUnknown, kChecked, kByConstruction };

void launch_pose_optimization(const PoseProblem* probs, int nprobs, const double* Xw, const BaEdge* edges, const CameraD& cam,
                              double* poses7, uint8_t* outlier, double* chi2_scratch, int* inliers, int max_edges /* upper bound of PoseProblem::n */,
                              hipStream_t st, PoseFloats floats = PoseFloats::kUnknown);
// *exact (an int the caller set to 1 on the stream before) is cleared when one of those values of the n staged correspondences is no float's value
void launch_pose_inputs_float_exact(const double* Xw, const BaEdge* edges, int n, int* exact, hipStream_t st);

}  // namespace tc2li

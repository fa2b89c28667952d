// The rotation-consistency filter of ORBmatcher (SF/src/ORBmatcher.cc), shared by the tracking kernels (SearchByProjection) and the
// vocabulary kernels (SearchByBoW): the 30-bin histogram of the keypoint angle differences and ComputeThreeMaxima (:2021-2062).
#pragma once
#include <hip/hip_runtime.h>

namespace tc2li {

constexpr int kRotHistLength = 30;  // HISTO_LENGTH

// rot = a - b (+360 when negative), bin = round(rot * (1/30)) with roundf -- only bins 0..12 occur, a quirk kept -- and 30 -> 0
__device__ __forceinline__ int rot_hist_bin(float a, float b) {
    const float factor = 1.0f / kRotHistLength;
    float rot = a - b;
    if (rot < 0.0) rot += 360.0f;
    int bin = (int)roundf(rot * factor);
    if (bin == kRotHistLength) bin = 0;
    return bin;
}

// ORBmatcher::ComputeThreeMaxima over the bin sizes count[30] -> ind[3] (-1: not kept)
__device__ __forceinline__ void rot_hist_three_maxima(const int* count, int* ind) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < kRotHistLength; i++) {
        const int s = count[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
    ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
}

}  // namespace tc2li

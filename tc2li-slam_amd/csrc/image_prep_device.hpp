// Image ingest (include/tc2li_hip.h "image ingest"): what System::TrackStereoLidar (SF/src/System.cc:240-257: clone / cv::remap /
// cv::resize) and Tracking::GrabImageStereoLidar (SF/src/Tracking.cc:1646-1671: cvtColor to gray) do to a camera image before
// ORBextractor::operator() sees it.  image_prep_host.cpp validates, keeps the handle and runs the host twin; image_prep_kernels.hip
// holds the kernels.  The arithmetic both sides share is the inline functions at the end: all of it is integer but the one float product
// of the map conversion, so the host twin and the kernels give the same bytes.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/tc2li_hip.h"

namespace tc2li {

constexpr int kImagePrepMaxDim = 16384;
constexpr int kImagePrepMaxImages = 65535;   // the image is the launch grid's y

// One call of tc2li_image_prep_batch as the kernels see it.  Image i: src + i * src_pitch, rows src_stride bytes apart, `channels`
// interleaved bytes per pixel; gray image i: dst + i * dst_pitch, rows dst_stride bytes apart.
struct ImagePrepBatch {
    const uint8_t* src;
    uint8_t* dst;
    size_t src_pitch, dst_pitch;
    int src_stride, dst_stride;
    int sw, sh, dw, dh;
    int n_images;
    int k0, k2;                        // gray weights of channels 0 and 2 (mbRGB swaps them)
    // RECTIFY: the fixed-point maps of camera 0 / 1, rows of rec_pitch records (a multiple of 4: a lane's four records are one load)
    const uint32_t* rec_xy[2];         // ix & 0xffff | iy << 16, both saturated to int16
    const uint16_t* rec_frac[2];       // fy * 32 + fx
    int rec_pitch;
    // RESIZE: cv::resize's tables (orb_host.cpp build_resize_tables)
    const int* xofs; const short* ialpha; const int* yofs; const short* ibeta;
};
void launch_image_prep_gray(const ImagePrepBatch& B, int channels, hipStream_t st);
void launch_image_prep_rectify(const ImagePrepBatch& B, int channels, hipStream_t st);
void launch_image_prep_resize(const ImagePrepBatch& B, int channels, hipStream_t st);
// float maps (device memory, rows of w floats) -> records
void launch_image_prep_fix_maps(const float* map_x, const float* map_y, int w, int h, int rec_pitch, uint32_t* rec_xy, uint16_t* rec_frac, hipStream_t st);

namespace prep {

constexpr int kR2Y = 9798, kG2Y = 19235, kB2Y = 3735;   // cvtColor's 15-bit weights; their sum is 32768

// cvtColor RGB2GRAY / BGR2GRAY (and the RGBA / BGRA forms: the fourth channel is not read): k0 = rgb ? kR2Y : kB2Y, k2 the other one
__host__ __device__ inline int gray(int c0, int c1, int c2, int k0, int k2) { return (c0 * k0 + c1 * kG2Y + c2 * k2 + 16384) >> 15; }

// cvRound is defined for these only (and map * 32 then fits an int)
__host__ __device__ inline bool map_value_ok(float v) { return fabsf(v) < 16777216.0f; }   // false for NaN and infinities too

__host__ __device__ inline int round_half_even(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float2int_rn(v);
#else
    return (int)lrintf(v);
#endif
}
__host__ __device__ inline int sat_i16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cv::remap's conversion of a CV_32F map pair (convertMaps to fixed point, INTER_BITS = 5): the product is a float product
__host__ __device__ inline void fix_map(float mx, float my, int* ix, int* iy, int* frac) {
    const int sx = round_half_even(mx * 32.0f), sy = round_half_even(my * 32.0f);
    *ix = sat_i16(sx >> 5);
    *iy = sat_i16(sy >> 5);
    *frac = (sy & 31) * 32 + (sx & 31);
}

// cv::remap INTER_LINEAR on 8U: weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32 (their sum is 32768) and
// (sum + 16384) >> 15.  Every weight carries the factor 32, so this is (sum / 32 + 512) >> 10 exactly.
__host__ __device__ inline int remap_blend(int p00, int p01, int p10, int p11, int frac) {
    const int fx = frac & 31, fy = frac >> 5;
    const int top = (32 - fx) * p00 + fx * p01, bottom = (32 - fx) * p10 + fx * p11;
    return ((32 - fy) * top + fy * bottom + 512) >> 10;
}

// cv::resize INTER_LINEAR on 8U: the horizontal pass of one source row and the vertical combine
__host__ __device__ inline int resize_row(int p0, int p1, int a0, int a1) { return p0 * a0 + p1 * a1; }
__host__ __device__ inline int resize_combine(int r0, int r1, int b0, int b1) { return (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2; }

}  // namespace prep
}  // namespace tc2li

// gfx950 kernels of the image ingest (image_prep_device.hpp): colour to gray, cv::remap, cv::resize -- one launch per call for all images
// of the batch.  Streaming work: no LDS, no atomics.  The image is the grid's y, so the image's base addresses and its camera are scalars.
//   k_prep_gray     COPY: a lane makes 16 gray bytes from 16 * C source bytes and stores them as one 16-byte word.
//   k_prep_rectify  RECTIFY: a lane owns four neighbouring outputs; their fixed-point map records are one 16-byte and one 8-byte load of
//                   tables that the whole batch shares (k_prep_fix_maps made them once); 4 taps x C channels are gathered, a tap outside
//                   the source is not loaded; gray is formed in registers; one dword store.
//   k_prep_resize   RESIZE: the same shape with cv::resize's tables.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "launch.hpp"
// the one float operation here, map * 32, is rounded on its own like the host's
#pragma clang fp contract(off)
#include "image_prep_device.hpp"

namespace tc2li {
namespace {

// Pointers that arrive inside the by-value batch record are generic to the compiler; they are device-global by construction (orb_kernels.hip).
template <class T>
__device__ __forceinline__ const __attribute__((address_space(1))) T* as_global(const T* p) {
    return (const __attribute__((address_space(1))) T*)p;
}
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* as_global_out(T* p) {
    return (__attribute__((address_space(1))) T*)p;
}
typedef const __attribute__((address_space(1))) uint8_t* gbytes;
typedef __attribute__((address_space(1))) uint8_t* gbytes_out;
typedef uint16_t u16_unaligned __attribute__((aligned(1)));
typedef uint32_t u32_unaligned __attribute__((aligned(1)));
typedef unsigned long long u64_unaligned __attribute__((aligned(1)));
// clang's vector types (HIP's uint4 is a class: no object of it lives in a named address space)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef int32_t i32x4 __attribute__((ext_vector_type(4)));

template <int C> struct Px { static constexpr int N = C == 1 ? 1 : 3; };   // channels that are read: a fourth one is ignored

// two neighbouring pixels, 2 * C bytes from p on, all of them inside the row
template <int C>
__device__ __forceinline__ void load_pair(gbytes p, int (&a)[Px<C>::N], int (&b)[Px<C>::N]) {
    if constexpr (C == 1) {
        const uint32_t v = *reinterpret_cast<const __attribute__((address_space(1))) u16_unaligned*>(p);
        a[0] = v & 0xff; b[0] = v >> 8;
    } else if constexpr (C == 3) {
        const uint32_t lo = *reinterpret_cast<const __attribute__((address_space(1))) u32_unaligned*>(p);
        const uint32_t hi = *reinterpret_cast<const __attribute__((address_space(1))) u16_unaligned*>(p + 4);
        a[0] = lo & 0xff; a[1] = (lo >> 8) & 0xff; a[2] = (lo >> 16) & 0xff;
        b[0] = lo >> 24; b[1] = hi & 0xff; b[2] = hi >> 8;
    } else {
        const unsigned long long q = *reinterpret_cast<const __attribute__((address_space(1))) u64_unaligned*>(p);
        const uint32_t lo = (uint32_t)q, hi = (uint32_t)(q >> 32);
        a[0] = lo & 0xff; a[1] = (lo >> 8) & 0xff; a[2] = (lo >> 16) & 0xff;
        b[0] = hi & 0xff; b[1] = (hi >> 8) & 0xff; b[2] = (hi >> 16) & 0xff;
    }
}
// one pixel, or zeros without a load where it lies outside the source
template <int C>
__device__ __forceinline__ void load_px_or_zero(gbytes row, int x, bool inside, int (&a)[Px<C>::N]) {
#pragma unroll
    for (int c = 0; c < Px<C>::N; ++c) a[c] = 0;
    if (inside) {
#pragma unroll
        for (int c = 0; c < Px<C>::N; ++c) a[c] = row[(size_t)x * C + c];
    }
}
template <int C>
__device__ __forceinline__ int to_gray(const int (&v)[Px<C>::N], int k0, int k2) {
    if constexpr (C == 1) return v[0];
    else return prep::gray(v[0], v[1], v[2], k0, k2);
}
// four neighbouring output bytes: one dword where the address allows it
__device__ __forceinline__ void store4(gbytes_out D, uint32_t packed, int n_valid) {
    if (n_valid == 4 && ((uintptr_t)D & 3) == 0) {
        *reinterpret_cast<__attribute__((address_space(1))) uint32_t*>(D) = packed;
    } else {
        for (int k = 0; k < n_valid; ++k) D[k] = (uint8_t)(packed >> (8 * k));
    }
}

// ---- COPY: colour to gray (1 channel: the clone) ----------------------------------------------------------------------------------
// A wavefront owns 1024 output pixels of one row.  The row splits at the 16-byte boundaries of the OUTPUT: a head of up to 15 pixels, body
// groups of 16, a tail of up to 15; head and tail are done pixel by pixel with byte loads.  A body group's 16 * C source bytes are read
// as aligned words: 16-byte words where the group's first source byte is 16-byte aligned, else the dwords that cover it (one more dword
// than 4 * C, not loaded where the first byte is dword-aligned) shifted into place.  All groups of a row share that alignment: they are
// 16 * C = 16, 48 or 64 bytes apart.
template <int C>
__global__ __launch_bounds__(256) void k_prep_gray(ImagePrepBatch B, int chunks_per_row) {
    constexpr int ND = 4 * C;   // dwords of a group's source
    const int img = (int)blockIdx.y;
    const int unit = (int)blockIdx.x * 4 + wave_in_block();
    if (unit >= B.dh * chunks_per_row) return;
    const int y = unit / chunks_per_row, chunk = unit - y * chunks_per_row;
    const int lane = (int)(threadIdx.x & 63);
    gbytes S = as_global(B.src) + (size_t)img * B.src_pitch + (size_t)y * B.src_stride;
    gbytes_out D = as_global_out(B.dst) + (size_t)img * B.dst_pitch + (size_t)y * B.dst_stride;
    const int w = B.dw;
    int head = (int)((0 - (uintptr_t)D) & 15);
    if (head > w) head = w;
    const int n_body = (w - head) >> 4;
    const int tail_begin = head + 16 * n_body;
    const int g = chunk * 64 + lane;
    if (g < n_body) {
        const int x = head + 16 * g;
        const uintptr_t a = (uintptr_t)(S + (size_t)x * C);
        const int mis = (int)((uintptr_t)(S + (size_t)head * C) & 15);   // == a & 15, and the same in the whole row
        uint32_t d[ND + 1];
        if (mis == 0) {
            const auto* q = reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(a);
#pragma unroll
            for (int i = 0; i < C; ++i) {
                const u32x4 v = q[i];
                d[4 * i] = v.x; d[4 * i + 1] = v.y; d[4 * i + 2] = v.z; d[4 * i + 3] = v.w;
            }
        } else {
            const auto* q = reinterpret_cast<const __attribute__((address_space(1))) uint32_t*>(a & ~(uintptr_t)3);
            const int shift = 8 * (mis & 3);
#pragma unroll
            for (int i = 0; i < ND; ++i) d[i] = q[i];
            d[ND] = 0;
            if (shift) d[ND] = q[ND];   // a dword-aligned group ends with its last dword: the next one may be nobody's
#pragma unroll
            for (int i = 0; i < ND; ++i) d[i] = __builtin_amdgcn_alignbit(d[i + 1], d[i], (uint32_t)shift);   // ({d[i + 1], d[i]} >> shift) & 0xffffffff
        }
        uint32_t out[4];
        if constexpr (C == 1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = d[i];
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                out[i] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int byte0 = (4 * i + k) * C;
                    int v[3];
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[c] = (int)((d[(byte0 + c) >> 2] >> (8 * ((byte0 + c) & 3))) & 0xffu);
                    out[i] |= (uint32_t)prep::gray(v[0], v[1], v[2], B.k0, B.k2) << (8 * k);
                }
            }
        }
        const u32x4 o4 = {out[0], out[1], out[2], out[3]};
        *reinterpret_cast<__attribute__((address_space(1))) u32x4*>(D + x) = o4;
    }
    if (chunk == 0) {
        const int n_edge = head + (w - tail_begin);   // at most 30
        if (lane < n_edge) {
            const int x = lane < head ? lane : tail_begin + (lane - head);
            int v[Px<C>::N];
            load_px_or_zero<C>(S, x, true, v);
            D[x] = (uint8_t)to_gray<C>(v, B.k0, B.k2);
        }
    }
}

// ---- RECTIFY -------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_prep_fix_maps(const float* __restrict__ map_x, const float* __restrict__ map_y, int w, int h, int rec_pitch,
                                                       uint32_t* __restrict__ rec_xy, uint16_t* __restrict__ rec_frac) {
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= h * rec_pitch) return;
    const int y = t / rec_pitch, x = t - y * rec_pitch;
    int ix = 0, iy = 0, frac = 0;
    if (x < w) prep::fix_map(map_x[(size_t)y * w + x], map_y[(size_t)y * w + x], &ix, &iy, &frac);
    rec_xy[t] = ((uint32_t)ix & 0xffffu) | ((uint32_t)iy << 16);
    rec_frac[t] = (uint16_t)frac;
}

template <int C>
__global__ __launch_bounds__(256) void k_prep_rectify(ImagePrepBatch B) {
    constexpr int N = Px<C>::N;
    const int img = (int)blockIdx.y, cam = img & 1;
    const int groups = B.rec_pitch >> 2;
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= B.dh * groups) return;
    const int y = t / groups, x0 = (t - y * groups) * 4;
    const size_t r = (size_t)y * B.rec_pitch + x0;
    const u32x4 xy4 = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(as_global(B.rec_xy[cam]) + r);
    const u32x2 fr2 = *reinterpret_cast<const __attribute__((address_space(1))) u32x2*>(as_global(B.rec_frac[cam]) + r);
    const uint32_t xys[4] = {xy4.x, xy4.y, xy4.z, xy4.w};
    gbytes S = as_global(B.src) + (size_t)img * B.src_pitch;
    const int n_valid = min(4, B.dw - x0);
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < n_valid) {
            const int ix = (int)(short)(xys[k] & 0xffffu), iy = (int)xys[k] >> 16;
            const int frac = (int)(((k < 2 ? fr2.x : fr2.y) >> (16 * (k & 1))) & 0xffffu);
            const bool x0in = ix >= 0 && ix < B.sw, x1in = ix + 1 >= 0 && ix + 1 < B.sw;
            const bool y0in = iy >= 0 && iy < B.sh, y1in = iy + 1 >= 0 && iy + 1 < B.sh;
            gbytes R0 = S + (ptrdiff_t)iy * B.src_stride, R1 = R0 + B.src_stride;   // only dereferenced where the row is inside
            int p00[N], p01[N], p10[N], p11[N];
            if (x0in && x1in && y0in && y1in) {
                load_pair<C>(R0 + (size_t)ix * C, p00, p01);
                load_pair<C>(R1 + (size_t)ix * C, p10, p11);
            } else {   // BORDER_CONSTANT 0: a tap outside reads 0; it is not dereferenced and its address is not clamped
                load_px_or_zero<C>(R0, ix, x0in && y0in, p00);
                load_px_or_zero<C>(R0, ix + 1, x1in && y0in, p01);
                load_px_or_zero<C>(R1, ix, x0in && y1in, p10);
                load_px_or_zero<C>(R1, ix + 1, x1in && y1in, p11);
            }
            int v[N];
#pragma unroll
            for (int c = 0; c < N; ++c) v[c] = prep::remap_blend(p00[c], p01[c], p10[c], p11[c], frac);
            packed |= (uint32_t)to_gray<C>(v, B.k0, B.k2) << (8 * k);
        }
    }
    store4(as_global_out(B.dst) + (size_t)img * B.dst_pitch + (size_t)y * B.dst_stride + x0, packed, n_valid);
}

// ---- RESIZE --------------------------------------------------------------------------------------------------------------------------
// The tables are padded to a multiple of four columns: a lane's four offsets and eight weights are one 16-byte load each.
template <int C>
__global__ __launch_bounds__(256) void k_prep_resize(ImagePrepBatch B) {
    constexpr int N = Px<C>::N;
    const int img = (int)blockIdx.y;
    const int groups = (B.dw + 3) >> 2;
    const int t = (int)(blockIdx.x * 256 + threadIdx.x);
    if (t >= B.dh * groups) return;
    const int y = t / groups, x0 = (t - y * groups) * 4;
    const i32x4 xo = *reinterpret_cast<const __attribute__((address_space(1))) i32x4*>(as_global(B.xofs) + x0);
    const u32x4 al = *reinterpret_cast<const __attribute__((address_space(1))) u32x4*>(as_global(B.ialpha) + 2 * x0);
    const int sxs[4] = {xo.x, xo.y, xo.z, xo.w};
    const uint32_t als[4] = {al.x, al.y, al.z, al.w};
    int sy0 = as_global(B.yofs)[y], sy1 = sy0 + 1;
    sy0 = sy0 < 0 ? 0 : (sy0 >= B.sh ? B.sh - 1 : sy0);
    sy1 = sy1 < 0 ? 0 : (sy1 >= B.sh ? B.sh - 1 : sy1);
    const int b0 = as_global(B.ibeta)[2 * y], b1 = as_global(B.ibeta)[2 * y + 1];
    gbytes S = as_global(B.src) + (size_t)img * B.src_pitch;
    gbytes R0 = S + (size_t)sy0 * B.src_stride, R1 = S + (size_t)sy1 * B.src_stride;
    const int n_valid = min(4, B.dw - x0);
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (k < n_valid) {
            const int sx = sxs[k];
            const int a0 = (short)(als[k] & 0xffffu), a1 = (short)(als[k] >> 16);
            int p00[N], p01[N], p10[N], p11[N];
            if (sx + 1 < B.sw) {
                load_pair<C>(R0 + (size_t)sx * C, p00, p01);
                load_pair<C>(R1 + (size_t)sx * C, p10, p11);
            } else {   // the last column: the second tap's weight is 0
                load_px_or_zero<C>(R0, sx, true, p00);
                load_px_or_zero<C>(R1, sx, true, p10);
#pragma unroll
                for (int c = 0; c < N; ++c) { p01[c] = p00[c]; p11[c] = p10[c]; }
            }
            int v[N];
#pragma unroll
            for (int c = 0; c < N; ++c)
                v[c] = prep::resize_combine(prep::resize_row(p00[c], p01[c], a0, a1), prep::resize_row(p10[c], p11[c], a0, a1), b0, b1);
            packed |= (uint32_t)(to_gray<C>(v, B.k0, B.k2) & 0xff) << (8 * k);
        }
    }
    store4(as_global_out(B.dst) + (size_t)img * B.dst_pitch + (size_t)y * B.dst_stride + x0, packed, n_valid);
}

}  // namespace

#define TC2LI_PREP_BY_CHANNELS(kernel, grid, st, ...)                                          \
    do {                                                                                       \
        if (channels == 1) TC2LI_LAUNCH(kernel<1>, grid, dim3(256), 0, st, __VA_ARGS__);       \
        else if (channels == 3) TC2LI_LAUNCH(kernel<3>, grid, dim3(256), 0, st, __VA_ARGS__);  \
        else TC2LI_LAUNCH(kernel<4>, grid, dim3(256), 0, st, __VA_ARGS__);                     \
    } while (0)

void launch_image_prep_gray(const ImagePrepBatch& B, int channels, hipStream_t st) {
    const int chunks_per_row = ((B.dw >> 4) + 63) / 64 > 0 ? ((B.dw >> 4) + 63) / 64 : 1;
    const dim3 grid((unsigned)(((long long)B.dh * chunks_per_row + 3) / 4), (unsigned)B.n_images);
    TC2LI_PREP_BY_CHANNELS(k_prep_gray, grid, st, B, chunks_per_row);
}

void launch_image_prep_rectify(const ImagePrepBatch& B, int channels, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)B.dh * (B.rec_pitch >> 2) + 255) / 256), (unsigned)B.n_images);
    TC2LI_PREP_BY_CHANNELS(k_prep_rectify, grid, st, B);
}

void launch_image_prep_resize(const ImagePrepBatch& B, int channels, hipStream_t st) {
    const dim3 grid((unsigned)(((long long)B.dh * ((B.dw + 3) >> 2) + 255) / 256), (unsigned)B.n_images);
    TC2LI_PREP_BY_CHANNELS(k_prep_resize, grid, st, B);
}

void launch_image_prep_fix_maps(const float* map_x, const float* map_y, int w, int h, int rec_pitch, uint32_t* rec_xy, uint16_t* rec_frac, hipStream_t st) {
    TC2LI_LAUNCH(k_prep_fix_maps, dim3((unsigned)(((long long)h * rec_pitch + 255) / 256)), dim3(256), 0, st, map_x, map_y, w, h, rec_pitch, rec_xy, rec_frac);
}

}  // namespace tc2li

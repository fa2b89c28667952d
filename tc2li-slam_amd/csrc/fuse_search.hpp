// The two pieces of arithmetic that the device kernels and the host twin of SearchInNeighbors run from one text:
//   fuse_search_one   ORBmatcher::Fuse, the search of one map point (SF/src/ORBmatcher.cc:1185-1318): the body of fuse_point of
//                     mapping_kernels.hip, moved here unchanged; k_fuse_search* call it and keep their results bit for bit
//   row_median        MapPoint::ComputeDistinctiveDescriptors (SF/src/MapPoint.cc:377-406): the entry (int)(0.5 (N - 1)) of the sorted
//                     Hamming row of descriptor i, by the bisection of k_map_points_refresh (the smallest v with k + 1 entries <= v)
// Every float operation is written out in the reference's order and compiled with contraction off on both sides; sqrtf, the
// quotients, floorf and ceilf are correctly rounded on both.  Where the two sides can still differ: the log inside the predicted
// level (the device's double log and the host's libm log may differ in the last bit, which moves ceilf only where the ratio of the
// distances sits on a power of the scale factor).  Everything after it is integer work or exact.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "mapping_device.hpp"

namespace tc2li {

#define TC2LI_HD __host__ __device__ __forceinline__

TC2LI_HD int popc32(uint32_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popc(v);
#else
    return __builtin_popcount(v);
#endif
}
TC2LI_HD int imax_hd(int a, int b) { return a > b ? a : b; }
TC2LI_HD int imin_hd(int a, int b) { return a < b ? a : b; }

struct Kp { float x, y, angle; int octave; };
TC2LI_HD Kp load_kp(const float* keys, int i) {
    const float* k = keys + 6 * (size_t)i;
    Kp o;
    o.x = k[0]; o.y = k[1]; o.angle = k[3];
#if defined(__HIP_DEVICE_COMPILE__)
    o.octave = __float_as_int(k[5]);
#else
    memcpy(&o.octave, k + 5, 4);
#endif
    return o;
}

TC2LI_HD void q_rot_dev(const float q[4], const float v[3], float out[3]) {  // Eigen _transformVector
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    out[0] = v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    out[1] = v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    out[2] = v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}
constexpr int kFuseGridCols = 64, kFuseGridRows = 48;

// the map point record P (tc2li_map_point: pos 3, normal 3, min, max, max_raw, descriptor) against the keyframe of f: the keypoint of
// least descriptor distance among those that pass the gates and that distance (256: none); f.points / valid / best_* are not read
TC2LI_HD void fuse_search_one(const FuseDev& f, const float* P, int* best_idx_out, int* best_dist_out) {
    int best_idx = -1, best_dist = 256;
    {
        const float pos[3] = {P[0], P[1], P[2]};
        float pc[3];
        q_rot_dev(f.q, pos, pc);
        pc[0] += f.t[0]; pc[1] += f.t[1]; pc[2] += f.t[2];
        bool go = !(pc[2] < 0.0f);
        float u = 0, v = 0, ur = 0, dist3D = 0;
        if (go) {
            const float invz = 1 / pc[2];
            u = f.fx * pc[0] / pc[2] + f.cx; v = f.fy * pc[1] / pc[2] + f.cy;
            go = u >= f.min_x && u < f.max_x && v >= f.min_y && v < f.max_y;
            ur = u - f.bf * invz;
        }
        if (go) {
            const float PO[3] = {pos[0] - f.Ow[0], pos[1] - f.Ow[1], pos[2] - f.Ow[2]};
            dist3D = sqrtf((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]);
            go = !(dist3D < P[6] || dist3D > P[7]);
            const float dotn = (PO[0] * P[3] + PO[1] * P[4]) + PO[2] * P[5];
            go = go && !((double)dotn < 0.5 * (double)dist3D);
        }
        if (go) {
            const float ratio = P[8] / dist3D;
            int level = (int)ceilf((float)log((double)ratio) / f.log_scale_factor);  // logf of the reference, evaluated through double
            level = level < 0 ? 0 : (level >= f.n_levels ? f.n_levels - 1 : level);
            const float r = f.th * f.scale_factors[level];
            const float invW = (float)kFuseGridCols / (f.max_x - f.min_x), invH = (float)kFuseGridRows / (f.max_y - f.min_y);
            const int minCX = imax_hd(0, (int)floorf((u - f.min_x - r) * invW)), maxCX = imin_hd(kFuseGridCols - 1, (int)ceilf((u - f.min_x + r) * invW));
            const int minCY = imax_hd(0, (int)floorf((v - f.min_y - r) * invH)), maxCY = imin_hd(kFuseGridRows - 1, (int)ceilf((v - f.min_y + r) * invH));
            if (!(minCX >= kFuseGridCols || maxCX < 0 || minCY >= kFuseGridRows || maxCY < 0)) {
                const uint32_t* qd = reinterpret_cast<const uint32_t*>(P + 9);
                uint32_t q[8];
#pragma unroll
                for (int w = 0; w < 8; ++w) q[w] = qd[w];
                for (int ix = minCX; ix <= maxCX; ++ix)
                    for (int iy = minCY; iy <= maxCY; ++iy) {
                        const int c = ix * kFuseGridRows + iy;
                        for (int k = f.cell_start[c]; k < f.cell_start[c + 1]; ++k) {
                            const int idx = f.items[k];
                            const Kp kp = load_kp(f.keys, idx);
                            if (!(fabsf(kp.x - u) < r && fabsf(kp.y - v) < r)) continue;
                            if (kp.octave < level - 1 || kp.octave > level) continue;
                            const float kur = f.u_right[idx];
                            const float ex = u - kp.x, ey = v - kp.y;
                            if (kur >= 0) {
                                const float er = ur - kur;
                                const float e2 = ex * ex + ey * ey + er * er;
                                if ((double)(e2 * f.inv_level_sigma2[kp.octave]) > 7.8) continue;
                            } else {
                                const float e2 = ex * ex + ey * ey;
                                if ((double)(e2 * f.inv_level_sigma2[kp.octave]) > 5.99) continue;
                            }
                            const uint32_t* kd = reinterpret_cast<const uint32_t*>(f.desc) + 8 * (size_t)idx;
                            int dist = 0;
#pragma unroll
                            for (int w = 0; w < 8; ++w) dist += popc32(q[w] ^ kd[w]);
                            if (dist < best_dist) { best_dist = dist; best_idx = idx; }
                        }
                    }
            }
        }
    }
    *best_dist_out = best_dist;
    *best_idx_out = best_dist <= 50 ? best_idx : -1;  // TH_LOW
}

// descriptors [N] of 8 words, `stride` words apart; the median of row i as the reference takes it.  k_map_points_refresh
// (mappoint_kernels.hip) runs the same bisection over a table of distances it keeps in LDS: the two must be kept in step
// (tests/test_search_in_neighbors_gpu.py compares their choices and the values that follow, bit for bit).
TC2LI_HD int row_median(const uint32_t* descs, int stride, int N, int i) {
    uint32_t mine[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) mine[w] = descs[i * stride + w];
    const int kth = (int)(0.5 * (N - 1));
    int lo = 0, hi = 256;  // smallest v with count(row <= v) >= kth + 1
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int cnt = 0;
        for (int j = 0; j < N; ++j) {
            int d = 0;
#pragma unroll
            for (int w = 0; w < 8; ++w) d += popc32(mine[w] ^ descs[j * stride + w]);
            cnt += d <= mid ? 1 : 0;
        }
        if (cnt >= kth + 1) hi = mid; else lo = mid + 1;
    }
    return lo;
}

#undef TC2LI_HD

}  // namespace tc2li

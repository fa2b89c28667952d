// gfx950 kernels of Preprocess::velodyne_handler's feature branch (SF/include/lidar_front_end/preprocess.cpp:100-143) and
// give_feature / plane_judge / edge_jump_judge (:169-623): FAST-LIO's LOAM-style plane / edge classifier.  A batch of scans is
// bucketed by ring into lines (stable: each line keeps the scan's order), then every (scan, line) is worked on by one wavefront,
// except pass 1 (the plane walk), which is sequential along a line and runs one lane per line.  Doubles and floats as the reference
// writes them, sums left to right, no contraction (the library is built with -ffp-contract=off): results are bit-equal to the CPU.
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "lidar_device.hpp"

namespace tc2li {

// Preprocess::Preprocess (:32-58); disA is assigned twice there (0.01, then 0.1), the second one holds
constexpr int kGroupSize = 8;
constexpr double kDisA = 0.1, kP2lRatio = 225, kLimitMaxmin = 3.24, kInfBound = 10, kEdgeA = 2, kEdgeB = 0.1, kSmallpRatio = 1.2;
enum : uint8_t { kNor = 0, kPossPlane = 1, kRealPlane = 2, kEdgeJump = 3, kEdgePlane = 4, kWire = 5 };  // Feature (preprocess.h:40)
enum : int { kNrNor = 0, kNrZero = 1, kNr180 = 2, kNrInf = 3, kNrBlind = 4 };                            // E_jump (preprocess.h:42)
constexpr uint8_t kSmallPlaneBit = 0x10;  // between the edge pass and the small-plane pass: pass 3's condition holds at the point

__device__ __forceinline__ double dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double norm3(const double* a) { return sqrt(dot3(a, a)); }  // Eigen's norm on Vector3d
__device__ __forceinline__ unsigned long long mask_le(int lane) { return lane == 63 ? ~0ull : ((2ull << lane) - 1); }
__device__ __forceinline__ int msb64(unsigned long long m) { return 63 - __clzll(m); }

// The (scan, line) a wavefront of the line kernels owns; false past the last one.
struct LineRef { int scan, line, base, lb, n; };
__device__ __forceinline__ bool line_of(int w, int nscans, const FeatureParams& fp, const ScanSlot* slots, const int* line_off, LineRef& r) {
    r.scan = w / fp.n_lines; r.line = w - r.scan * fp.n_lines;
    if (r.scan >= nscans) return false;
    r.base = slots[r.scan].base;
    const int* off = line_off + (size_t)r.scan * kFeatLineStride;
    r.lb = off[r.line]; r.n = off[r.line + 1] - r.lb;
    return true;
}

// ---- bucketing (:100-122): a workgroup per scan; per-line counts, then a stable scatter in chunks of 256 points ----------------
// Rank inside a wavefront: lanes with the same ring, found by a __ballot per ring bit; per-wavefront line counts go through the LDS.
constexpr int kBucketThreads = 256, kBucketWaves = kBucketThreads / 64;
__global__ __launch_bounds__(kBucketThreads) void k_feat_bucket(const VelodynePoint* __restrict__ raw, const int* __restrict__ raw_count,
                                                                const ScanSlot* __restrict__ slots, FeatureParams fp, int* __restrict__ line_off,
                                                                float4* __restrict__ pts, float2* __restrict__ ic) {
    __shared__ int s_base[kFeatMaxLines + 1];
    __shared__ int s_wcnt[kBucketWaves][kFeatMaxLines];
    const int s = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const ScanSlot sl = slots[s];
    const int n = raw_count[s];
    const float4* __restrict__ src = reinterpret_cast<const float4*>(raw + sl.raw_base);
    for (int l = tid; l <= kFeatMaxLines; l += kBucketThreads) s_base[l] = 0;
    __syncthreads();
    // VelodynePoint: x y z pad0 | intensity time (ring, pad1) pad2 -- the ring is the low half of the third word
    for (int i = tid; i < n; i += kBucketThreads) {
        const int ring = (int)(__float_as_uint(src[2 * (size_t)i + 1].z) & 0xffffu);
        if (ring < fp.n_lines) atomicAdd(&s_base[ring + 1], 1);  // `if (layer >= N_SCANS) continue;`
    }
    __syncthreads();
    if (tid == 0)
        for (int l = 0; l < fp.n_lines; ++l) s_base[l + 1] += s_base[l];
    __syncthreads();
    for (int l = tid; l <= fp.n_lines; l += kBucketThreads) line_off[(size_t)s * kFeatLineStride + l] = s_base[l];
    for (int c0 = 0; c0 < n; c0 += kBucketThreads) {
        const int i = c0 + tid;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f), b = a;
        if (i < n) { a = src[2 * (size_t)i]; b = src[2 * (size_t)i + 1]; }
        const int ring = i < n ? (int)(__float_as_uint(b.z) & 0xffffu) : 0x10000;
        const bool valid = ring < fp.n_lines;
        unsigned long long same = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 7; ++bit) {  // n_lines <= 128: the ring of a valid point has 7 bits
            const unsigned long long set = __ballot(valid && ((ring >> bit) & 1));
            same &= ((ring >> bit) & 1) ? set : ~set;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1));
        for (int l = tid; l < kBucketWaves * kFeatMaxLines; l += kBucketThreads) (&s_wcnt[0][0])[l] = 0;
        __syncthreads();
        if (valid && rank == 0) s_wcnt[wave][ring] = __popcll(same);
        __syncthreads();
        if (valid) {
            int pos = s_base[ring] + rank;
            for (int w = 0; w < wave; ++w) pos += s_wcnt[w][ring];
            const float r = sqrtf(a.x * a.x + a.y * a.y);  // types[i].range (:135): float sqrt, widened where it is used
            pts[sl.base + pos] = make_float4(a.x, a.y, a.z, r);
            ic[sl.base + pos] = make_float2(b.x, b.y * fp.time_unit_scale);  // curvature = time * time_unit_scale (:120)
        }
        __syncthreads();
        if (tid < fp.n_lines) {
            int add = 0;
#pragma unroll
            for (int w = 0; w < kBucketWaves; ++w) add += s_wcnt[w][tid];
            s_base[tid] += add;
        }
        __syncthreads();
    }
}

// ---- dista (:133-140) and the labels' reset: a wavefront per line ---------------------------------------------------------------
// The last point's dista is never written by the reference (orgtype() leaves it indeterminate), yet plane_judge can push it into
// disarr when its walk reaches the line's end: it is 0.0 here (what freshly zeroed memory holds).
__global__ __launch_bounds__(256) void k_feat_dista(const ScanSlot* __restrict__ slots, int nscans, FeatureParams fp, const int* __restrict__ line_off,
                                                    const float4* __restrict__ pts, double* __restrict__ dista, uint8_t* __restrict__ lab) {
    LineRef r;
    if (!line_of(blockIdx.x * 4 + wave_in_block(), nscans, fp, slots, line_off, r)) return;
    const float4* P = pts + r.base + r.lb;
    for (int i = threadIdx.x & 63; i < r.n; i += 64) {
        double d = 0.0;
        if (i + 1 < r.n) {
            const float4 p = P[i], q = P[i + 1];
            const double vx = p.x - q.x, vy = p.y - q.y, vz = p.z - q.z;  // float differences, held in the double members vx, vy, vz
            d = vx * vx + vy * vy + vz * vz;
        }
        dista[r.base + r.lb + i] = d;
        lab[r.base + r.lb + i] = kNor;
    }
}

// ---- pass 1, planes (:178-293 with plane_judge :484-584): one lane per line ------------------------------------------------------
// plane_judge: 2 at a blind point (i_nex = that point), 0 / 1 otherwise; i_nex = the point that ended the walk, or n if the line did.
// disarr is needed only for its maximum (disarr[0] after the descending bubble sort) and second-smallest element (disarr[size - 2]).
__device__ int plane_judge(const float4* __restrict__ P, const double* __restrict__ D, int n, int i_cur, int& i_nex, double cd[3],
                           const FeatureParams& fp) {
    cd[0] = cd[1] = cd[2] = 0.0;
    double group_dis = kDisA * (double)P[i_cur].w + fp.dis_b;
    group_dis = group_dis * group_dis;
    double dmax = -__builtin_inf(), dmin1 = __builtin_inf(), dmin2 = __builtin_inf();
    auto push = [&](double v) {
        if (v > dmax) dmax = v;
        if (v < dmin1) { dmin2 = dmin1; dmin1 = v; } else if (v < dmin2) dmin2 = v;
    };
    // the first group_size points: all in the line (i_cur < n - group_size), loaded together
    float rg[kGroupSize];
    double dg[kGroupSize];
#pragma unroll
    for (int k = 0; k < kGroupSize; ++k) { rg[k] = P[i_cur + k].w; dg[k] = D[i_cur + k]; }
#pragma unroll
    for (int k = 0; k < kGroupSize; ++k) {
        if ((double)rg[k] < fp.blind) { i_nex = i_cur + k; return 2; }
        push(dg[k]);
    }
    const float4 pc = P[i_cur];
    double vx = 0, vy = 0, vz = 0, two_dis = 0;
    int nx = i_cur + kGroupSize;
    // the walk, a group of points requested ahead of the tests
    bool done = false;
    while (!done) {
        float4 q[kGroupSize];
        double dq[kGroupSize];
#pragma unroll
        for (int k = 0; k < kGroupSize; ++k)
            if (nx + k < n) { q[k] = P[nx + k]; dq[k] = D[nx + k]; }
#pragma unroll
        for (int k = 0; k < kGroupSize; ++k) {
            if (nx >= n) { done = true; break; }
            if ((double)q[k].w < fp.blind) { i_nex = nx; return 2; }
            vx = q[k].x - pc.x; vy = q[k].y - pc.y; vz = q[k].z - pc.z;
            two_dis = vx * vx + vy * vy + vz * vz;
            if (two_dis >= group_dis) { done = true; break; }
            push(dq[k]);
            ++nx;
        }
    }
    i_nex = nx;
    double leng_wid = 0;
    for (int j = i_cur + 1; j < nx; ++j) {
        const float4 pj = P[j];
        const double v1[3] = {(double)(pj.x - pc.x), (double)(pj.y - pc.y), (double)(pj.z - pc.z)};
        const double v2[3] = {v1[1] * vz - vy * v1[2], v1[2] * vx - v1[0] * vz, v1[0] * vy - vx * v1[1]};
        const double lw = v2[0] * v2[0] + v2[1] * v2[1] + v2[2] * v2[2];
        if (lw > leng_wid) leng_wid = lw;
    }
    if ((two_dis * two_dis / leng_wid) < kP2lRatio) return 0;  // leng_wid == 0: inf or NaN, which fails the test (IEEE)
    if (dmin2 < 1e-16) return 0;
    if (dmax / dmin2 >= kLimitMaxmin) return 0;
    cd[0] = vx; cd[1] = vy; cd[2] = vz;
    const double sq = dot3(cd, cd);  // Eigen's normalize: / sqrt(squaredNorm) when it is > 0
    if (sq > 0) { const double nrm = sqrt(sq); cd[0] /= nrm; cd[1] /= nrm; cd[2] /= nrm; }
    return 1;
}

__global__ __launch_bounds__(256) void k_feat_planes(const ScanSlot* __restrict__ slots, int nscans, FeatureParams fp, const int* __restrict__ line_off,
                                                     const float4* __restrict__ pts, const double* __restrict__ dista, uint8_t* __restrict__ lab,
                                                     int* __restrict__ line_head) {
    LineRef r;
    if (!line_of(blockIdx.x * blockDim.x + threadIdx.x, nscans, fp, slots, line_off, r)) return;
    const float4* P = pts + r.base + r.lb;
    const double* D = dista + r.base + r.lb;
    uint8_t* L = lab + r.base + r.lb;
    const int n = r.n;
    int head = 0;
    if (n >= 2)
        while (head < n && (double)P[head].w < fp.blind) ++head;  // :180, stopped at the line's end (the reference reads past it)
    line_head[(size_t)r.scan * kFeatMaxLines + r.line] = head;
    if (n < 2) return;  // `if (linesize < 2) continue;`
    const int plsize2 = n > kGroupSize ? n - kGroupSize : 0;
    double last_direct[3] = {0, 0, 0}, cd[3];
    int last_state = 0;
    for (int i = head; i < plsize2; ++i) {
        if ((double)P[i].w < fp.blind) continue;
        int i_nex;
        const int plane_type = plane_judge(P, D, n, i, i_nex, cd, fp);
        if (plane_type == 1) {
            // j == n (a walk that reached the line's end) is one past the line: the reference writes it out of bounds, dropped here
            for (int j = i; j <= i_nex && j < n; ++j) L[j] = (j != i && j != i_nex) ? kRealPlane : kPossPlane;
            if (last_state == 1 && norm3(last_direct) > 0.1) {
                const double mod = dot3(last_direct, cd);
                L[i] = (mod > -0.707 && mod < 0.707) ? kEdgePlane : kRealPlane;
            }
            i = i_nex - 1;
            last_state = 1;
        } else {
            i = i_nex;
            last_state = 0;
        }
        last_direct[0] = cd[0]; last_direct[1] = cd[1]; last_direct[2] = cd[2];
    }
}

// ---- pass 2, edges (:295-389 with edge_jump_judge :586-623), and pass 3's condition: a wavefront per line, a lane per point ------
__device__ __forceinline__ bool edge_jump_judge(const float4* P, const double* D, int i, int nor_dir, const FeatureParams& fp) {
    if (nor_dir == 0) {
        if ((double)P[i - 1].w < fp.blind || (double)P[i - 2].w < fp.blind) return false;
    } else {
        if ((double)P[i + 1].w < fp.blind || (double)P[i + 2].w < fp.blind) return false;
    }
    double d1 = D[i + nor_dir - 1], d2 = D[i + 3 * nor_dir - 2];
    if (d1 < d2) { const double d = d1; d1 = d2; d2 = d; }
    d1 = sqrt(d1);
    d2 = sqrt(d2);
    return !(d1 > kEdgeA * d2 || (d1 - d2) > kEdgeB);
}

__global__ __launch_bounds__(256) void k_feat_edges(const ScanSlot* __restrict__ slots, int nscans, FeatureParams fp, const int* __restrict__ line_off,
                                                    const int* __restrict__ line_head, const float4* __restrict__ pts, const double* __restrict__ dista,
                                                    uint8_t* __restrict__ lab) {
    LineRef r;
    if (!line_of(blockIdx.x * 4 + wave_in_block(), nscans, fp, slots, line_off, r)) return;
    const int n = r.n;
    if (n < 2) return;
    const int head = line_head[(size_t)r.scan * kFeatMaxLines + r.line];
    const float4* P = pts + r.base + r.lb;
    const double* D = dista + r.base + r.lb;
    uint8_t* L = lab + r.base + r.lb;
    for (int i = threadIdx.x & 63; i < n; i += 64) {
        const float4 p = P[i];
        const double range = p.w;
        int ft = L[i];
        double intersect = 2;  // orgtype(); left there where the pass does not reach
        if (i >= head + 3 && i < n - 3 && !(range < fp.blind || ft >= kRealPlane) && !(D[i - 1] < 1e-16 || D[i] < 1e-16)) {
            const double a[3] = {p.x, p.y, p.z};
            double vecs[2][3];
            int edj[2] = {kNrNor, kNrNor};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float4 q = P[i + (j ? 1 : -1)];
                if ((double)q.w < fp.blind) {
                    edj[j] = range > kInfBound ? kNrInf : kNrBlind;
                    continue;
                }
                vecs[j][0] = (double)q.x - a[0]; vecs[j][1] = (double)q.y - a[1]; vecs[j][2] = (double)q.z - a[2];
                const double angle = dot3(a, vecs[j]) / norm3(a) / norm3(vecs[j]);
                if (angle < fp.jump_up_limit) edj[j] = kNr180;
                else if (angle > fp.jump_down_limit) edj[j] = kNrZero;
            }
            // with a blind neighbour the reference computes it from an unset vector; nothing reads it then (pass 3 needs both neighbours)
            if (edj[0] < kNrInf && edj[1] < kNrInf) intersect = dot3(vecs[0], vecs[1]) / norm3(vecs[0]) / norm3(vecs[1]);
            if (edj[0] == kNrNor && edj[1] == kNrZero && D[i] > 0.0225 && D[i] > 4 * D[i - 1]) {
                if (intersect > fp.cos160 && edge_jump_judge(P, D, i, 0, fp)) ft = kEdgeJump;
            } else if (edj[0] == kNrZero && edj[1] == kNrNor && D[i - 1] > 0.0225 && D[i - 1] > 4 * D[i]) {
                if (intersect > fp.cos160 && edge_jump_judge(P, D, i, 1, fp)) ft = kEdgeJump;
            } else if (edj[0] == kNrNor && edj[1] == kNrInf) {
                if (edge_jump_judge(P, D, i, 0, fp)) ft = kEdgeJump;
            } else if (edj[0] == kNrInf && edj[1] == kNrNor) {
                if (edge_jump_judge(P, D, i, 1, fp)) ft = kEdgeJump;
            } else if (edj[0] > kNrNor && edj[1] > kNrNor) {
                if (ft == kNor) ft = kWire;
            }
        }
        // pass 3's test (:393-416) reads only the point's own label and intersect (as pass 2 left them) and its neighbours' range / dista
        bool small = false;
        if (i >= head + 1 && i < n - 1 && ft == kNor && !(range < fp.blind || (double)P[i - 1].w < fp.blind || (double)P[i + 1].w < fp.blind) &&
            !(D[i - 1] < 1e-8 || D[i] < 1e-8)) {
            const double ratio = D[i - 1] > D[i] ? D[i - 1] / D[i] : D[i] / D[i - 1];
            small = intersect < fp.smallp_intersect && ratio < kSmallpRatio;
        }
        L[i] = (uint8_t)(ft | (small ? kSmallPlaneBit : 0));
    }
}

// ---- pass 3 (:391-429) and pass 4 (:431-482) over chunks of 64 points of a line ------------------------------------------------
// Pass 3 is order-dependent: when point i-1 fires it relabels i as Real_Plane, and i is skipped.  So fired[i] = c[i] && !fired[i-1]:
// inside a run of consecutive c the points at even distance from the run's start fire.  A point ends up Real_Plane when it was Nor
// and it, or a neighbour, fired.
// Pass 4: a run of surface points is cut into groups of point_filter_num, the last point of a group is copied; a non-surface point
// ends the run and the points of an unfinished group are averaged; a run that reaches the line's end emits nothing more.
struct EmitChunk {
    unsigned long long emit, corner;  // lanes that emit a surface point / a corner point
    int rem;                          // lanes that average: the number of points averaged (the ones before the lane); else 0
};
__device__ __forceinline__ EmitChunk emit_chunk(uint8_t ft, bool valid, int p /* index in the line */, int lane, int pfn, int& run_start) {
    const bool surf = valid && (ft == kPossPlane || ft == kRealPlane);
    const unsigned long long S = __ballot(surf);
    EmitChunk e;
    e.corner = __ballot(valid && (ft == kEdgeJump || ft == kEdgePlane));
    // start of the surface run that contains the lane (surface) or ends just before it (other)
    const unsigned long long below = ~S & (mask_le(lane) >> 1);
    const int base = p - lane;
    const int s = below ? base + msb64(below) + 1 : run_start;
    const int k = (p - s) % pfn;
    const bool copy = surf && k == pfn - 1;
    e.rem = (valid && !surf && k != 0) ? k : 0;
    e.emit = __ballot(copy || e.rem > 0);
    if (~S) run_start = base + msb64(~S) + 1;  // the next chunk's: a run open at lane 63 carries on
    return e;
}

__global__ __launch_bounds__(256) void k_feat_small_planes(const ScanSlot* __restrict__ slots, int nscans, FeatureParams fp, const int* __restrict__ line_off,
                                                           uint8_t* __restrict__ lab, int2* __restrict__ line_cnt) {
    LineRef r;
    if (!line_of(blockIdx.x * 4 + wave_in_block(), nscans, fp, slots, line_off, r)) return;
    const int lane = threadIdx.x & 63, n = r.n;
    uint8_t* L = lab + r.base + r.lb;
    bool prev_fired = false;
    int run_start = 0, n_surf = 0, n_corn = 0;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const bool valid = i < n;
        const uint8_t v = valid ? L[i] : 0;
        const bool c = v & kSmallPlaneBit;
        const bool c_next = lane == 63 && i + 1 < n && (L[i + 1] & kSmallPlaneBit);
        const unsigned long long C = __ballot(c);
        bool fired = false;
        if (c) {
            const unsigned long long zeros = ~C & mask_le(lane);
            fired = zeros ? ((lane - (msb64(zeros) + 1)) & 1) == 0 : (!prev_fired) ^ (lane & 1);
        }
        const unsigned long long F = __ballot(fired);
        const bool fired_prev = lane ? (F >> (lane - 1)) & 1 : prev_fired;
        const bool fired_next = lane < 63 ? (F >> (lane + 1)) & 1 : (c_next && !fired);
        uint8_t ft = v & 0x0f;
        if (ft == kNor && (fired || fired_prev || fired_next)) ft = kRealPlane;
        if (valid) L[i] = ft;
        prev_fired = (F >> 63) & 1;
        const EmitChunk e = emit_chunk(ft, valid, i, lane, fp.point_filter_num, run_start);
        n_surf += __popcll(e.emit);
        n_corn += __popcll(e.corner);
    }
    if (lane == 0) line_cnt[(size_t)r.scan * kFeatMaxLines + r.line] = make_int2(n_surf, n_corn);
}

// Per scan: where each line's output starts (line order), and the totals.
__global__ __launch_bounds__(kFeatMaxLines) void k_feat_prefix(int nscans, FeatureParams fp, int2* __restrict__ line_cnt, int* __restrict__ out_count,
                                                               int* __restrict__ corn_count) {
    __shared__ int2 s_c[kFeatMaxLines];
    const int s = blockIdx.x, tid = threadIdx.x;
    int2* c = line_cnt + (size_t)s * kFeatMaxLines;
    s_c[tid] = tid < fp.n_lines ? c[tid] : make_int2(0, 0);
    __syncthreads();
    if (tid == 0) {
        int a = 0, b = 0;
        for (int l = 0; l < fp.n_lines; ++l) { const int2 v = s_c[l]; s_c[l] = make_int2(a, b); a += v.x; b += v.y; }
        out_count[s] = a;
        corn_count[s] = b;
    }
    __syncthreads();
    if (tid < fp.n_lines) c[tid] = s_c[tid];
}

__device__ __forceinline__ PointXYZINormal feat_point(float x, float y, float z, float intensity, float curvature) {
    PointXYZINormal o;
    o.x = x; o.y = y; o.z = z; o.pad0 = 1.0f;  // PCL_ADD_POINT4D's data[3]
    o.normal_x = 0; o.normal_y = 0; o.normal_z = 0; o.pad1 = 0;
    o.intensity = intensity; o.curvature = curvature; o.pad2 = 0; o.pad3 = 0;
    return o;
}

__global__ __launch_bounds__(256) void k_feat_emit(const ScanSlot* __restrict__ slots, int nscans, FeatureParams fp, const int* __restrict__ line_off,
                                                   const uint8_t* __restrict__ lab, const int2* __restrict__ line_start, const float4* __restrict__ pts,
                                                   const float2* __restrict__ ic, PointXYZINormal* __restrict__ surf, PointXYZINormal* __restrict__ corn) {
    LineRef r;
    if (!line_of(blockIdx.x * 4 + wave_in_block(), nscans, fp, slots, line_off, r)) return;
    const int lane = threadIdx.x & 63, n = r.n;
    const uint8_t* L = lab + r.base + r.lb;
    const float4* P = pts + r.base + r.lb;
    const float2* I = ic + r.base + r.lb;
    const int2 st = line_start[(size_t)r.scan * kFeatMaxLines + r.line];
    PointXYZINormal* out_s = surf + r.base + st.x;
    PointXYZINormal* out_c = corn + r.base + st.y;
    int run_start = 0;
    const unsigned long long lt = (1ull << lane) - 1;
    for (int c0 = 0; c0 < n; c0 += 64) {
        const int i = c0 + lane;
        const bool valid = i < n;
        const uint8_t ft = valid ? L[i] : 0;
        const EmitChunk e = emit_chunk(ft, valid, i, lane, fp.point_filter_num, run_start);
        if ((e.emit >> lane) & 1) {
            PointXYZINormal o;
            if (e.rem) {  // PointXYZINormal ap: zeros, summed in line order in float, divided by the count
                float x = 0.f, y = 0.f, z = 0.f, in = 0.f, cv = 0.f;
                for (int k = i - e.rem; k < i; ++k) {
                    const float4 q = P[k];
                    const float2 w = I[k];
                    x += q.x; y += q.y; z += q.z; in += w.x; cv += w.y;
                }
                const float cnt = (float)e.rem;
                o = feat_point(x / cnt, y / cnt, z / cnt, in / cnt, cv / cnt);
            } else {
                const float4 q = P[i];
                const float2 w = I[i];
                o = feat_point(q.x, q.y, q.z, w.x, w.y);
            }
            out_s[__popcll(e.emit & lt)] = o;
        }
        if ((e.corner >> lane) & 1) {
            const float4 q = P[i];
            const float2 w = I[i];
            out_c[__popcll(e.corner & lt)] = feat_point(q.x, q.y, q.z, w.x, w.y);
        }
        out_s += __popcll(e.emit);
        out_c += __popcll(e.corner);
    }
}

void launch_feature_preprocess(const VelodynePoint* raw, const int* raw_count, const ScanSlot* slots, int nscans, const FeatureParams& fp,
                               const FeatureWork& w, PointXYZINormal* out, int* out_count, PointXYZINormal* corn, int* corn_count, hipStream_t st) {
    if (!nscans) return;
    const int lines = nscans * fp.n_lines, wave_blocks = (lines + 3) / 4;
    TC2LI_LAUNCH(k_feat_bucket, dim3(nscans), dim3(kBucketThreads), 0, st, raw, raw_count, slots, fp, w.line_off, w.pts, w.ic);
    TC2LI_LAUNCH(k_feat_dista, dim3(wave_blocks), dim3(256), 0, st, slots, nscans, fp, w.line_off, w.pts, w.dista, w.lab);
    TC2LI_LAUNCH(k_feat_planes, dim3((lines + 255) / 256), dim3(256), 0, st, slots, nscans, fp, w.line_off, w.pts, w.dista, w.lab, w.line_head);
    TC2LI_LAUNCH(k_feat_edges, dim3(wave_blocks), dim3(256), 0, st, slots, nscans, fp, w.line_off, w.line_head, w.pts, w.dista, w.lab);
    TC2LI_LAUNCH(k_feat_small_planes, dim3(wave_blocks), dim3(256), 0, st, slots, nscans, fp, w.line_off, w.lab, w.line_cnt);
    TC2LI_LAUNCH(k_feat_prefix, dim3(nscans), dim3(kFeatMaxLines), 0, st, nscans, fp, w.line_cnt, out_count, corn_count);
    TC2LI_LAUNCH(k_feat_emit, dim3(wave_blocks), dim3(256), 0, st, slots, nscans, fp, w.line_off, w.lab, w.line_cnt, w.pts, w.ic, out, corn);
}

}  // namespace tc2li

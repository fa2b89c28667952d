// Kernels of the CreateNewMapPoints core:
//   k_tri_search   ORBmatcher::SearchForTriangulation (SF/src/ORBmatcher.cc:916-1150): one thread per (neighbour, feature-vector
//                  entry of the current keyframe); the features of the same vocabulary node in the neighbour are scanned in order
//   k_tri_points   the per-pair body of LocalMapping::CreateNewMapPoints (SF/src/LocalMapping.cc:497-723): parallax gates,
//                  GeometricTools::Triangulate or KeyFrame::UnprojectStereo, depth / reprojection / scale gates
// The reference lets a keypoint that received a point from an earlier neighbour drop out of the later neighbours; a pair's result
// does not depend on any other pair, so every (neighbour, keypoint) is evaluated here and the first success is kept afterwards: by
// the host in the single-keyframe entry, by k_new_points_compact in the batch entry.  The *_batch kernels run the same device
// functions over a device table of (problem, neighbour) pairs or fuse items (keyframe_store.cpp).
#include <hip/hip_runtime.h>

#include "launch.hpp"
#pragma clang fp contract(off)
#include <stdint.h>

#include "fuse_search.hpp"
#include "mapping_device.hpp"

namespace tc2li {

// feature-vector entry e of the current keyframe against neighbour j: the body shared by k_tri_search and k_tri_search_batch
__device__ __forceinline__ void tri_search_entry(const MappingDev& m, int j, int e) {
    const KfDev& k2 = m.neigh[j];
    const KfDev& k1 = m.cur;
    if (e >= k1.fv_off[k1.n_nodes] || k2.skip) return;
    // node of entry e: the last node whose offset is <= e
    int lo = 0, hi = k1.n_nodes - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (k1.fv_off[mid] <= e) lo = mid; else hi = mid - 1; }
    const int node = k1.fv_node[lo];
    const int idx1 = k1.fv_idx[e];
    if (k1.has_point[idx1]) return;
    const bool stereo1 = k1.u_right[idx1] >= 0;
    if (m.only_stereo && !stereo1) return;
    // the same node in the neighbour
    int a = 0, b = k2.n_nodes;
    while (a < b) { const int mid = (a + b) >> 1; if (k2.fv_node[mid] < node) a = mid + 1; else b = mid; }
    if (a >= k2.n_nodes || k2.fv_node[a] != node) return;
    const Kp kp1 = load_kp(k1.keys, idx1);
    const uint32_t* d1 = reinterpret_cast<const uint32_t*>(k1.desc) + 8 * (size_t)idx1;
    uint32_t q[8];
#pragma unroll
    for (int w = 0; w < 8; ++w) q[w] = d1[w];
    const float* F = k2.F12;
    const float la = kp1.x * F[0] + kp1.y * F[3] + F[6];
    const float lb = kp1.x * F[1] + kp1.y * F[4] + F[7];
    const float lc = kp1.x * F[2] + kp1.y * F[5] + F[8];
    const float den = la * la + lb * lb;
    int bestDist = 50, bestIdx2 = -1;  // TH_LOW
    for (int i2 = k2.fv_off[a]; i2 < k2.fv_off[a + 1]; ++i2) {
        const int idx2 = k2.fv_idx[i2];
        if (k2.has_point[idx2]) continue;
        const bool stereo2 = k2.u_right[idx2] >= 0;
        if (m.only_stereo && !stereo2) continue;
        const uint32_t* d2 = reinterpret_cast<const uint32_t*>(k2.desc) + 8 * (size_t)idx2;
        int dist = 0;
#pragma unroll
        for (int w = 0; w < 8; ++w) dist += __popc(q[w] ^ d2[w]);
        if (dist > 50 || dist > bestDist) continue;
        const Kp kp2 = load_kp(k2.keys, idx2);
        if (!stereo1 && !stereo2) {
            const float dx = k2.ep[0] - kp2.x, dy = k2.ep[1] - kp2.y;
            if (dx * dx + dy * dy < 100 * m.scale_factors[kp2.octave]) continue;
        }
        bool ok = m.coarse != 0;
        if (!ok && den != 0) {  // Pinhole::epipolarConstrain
            const float num = la * kp2.x + lb * kp2.y + lc;
            const float dsqr = num * num / den;
            ok = (double)dsqr < 3.84 * (double)m.level_sigma2[kp2.octave];
        }
        if (ok) { bestIdx2 = idx2; bestDist = dist; }
    }
    if (bestIdx2 >= 0) m.match[(size_t)j * k1.n + idx1] = bestIdx2;
}

__global__ __launch_bounds__(256) void k_tri_search(MappingDev m) { tri_search_entry(m, blockIdx.y, blockIdx.x * 256 + threadIdx.x); }
// every (problem, neighbour) pair of a batch: `chunks` workgroups per pair, the problems' MappingDev records in a device table
__global__ __launch_bounds__(256) void k_tri_search_batch(const MappingDev* __restrict__ problems, const PairRef* __restrict__ pairs, int chunks) {
    const PairRef pr = pairs[blockIdx.x / chunks];
    const MappingDev m = problems[pr.problem];
    tri_search_entry(m, pr.neighbour, (blockIdx.x % chunks) * 256 + threadIdx.x);
}

// eigenvector of the smallest eigenvalue of the symmetric 4 x 4 M (cyclic Jacobi, double) -- stands in for JacobiSVD<Matrix4f>
__device__ void smallest_eigenvector4(double (&M)[16], double (&v)[4]) {
    double V[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) off += M[4 * p + q] * M[4 * p + q];
        if (off < 1e-40) break;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = M[4 * p + q];
                if (fabs(apq) < 1e-300) continue;
                const double theta = (M[4 * q + q] - M[4 * p + p]) / (2 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1));
                const double c = 1 / sqrt(t * t + 1), s = t * c;
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double a = M[4 * k + p], b = M[4 * k + q]; M[4 * k + p] = c * a - s * b; M[4 * k + q] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double a = M[4 * p + k], b = M[4 * q + k]; M[4 * p + k] = c * a - s * b; M[4 * q + k] = s * a + c * b; }
#pragma unroll
                for (int k = 0; k < 4; ++k) { const double a = V[4 * k + p], b = V[4 * k + q]; V[4 * k + p] = c * a - s * b; V[4 * k + q] = s * a + c * b; }
            }
    }
    // the diagonal entries through a select chain (no indexed register array)
    double best = M[0];
    int bi = 0;
    if (M[5] < best) { best = M[5]; bi = 1; }
    if (M[10] < best) { best = M[10]; bi = 2; }
    if (M[15] < best) { best = M[15]; bi = 3; }
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = bi == 0 ? V[4 * k] : (bi == 1 ? V[4 * k + 1] : (bi == 2 ? V[4 * k + 2] : V[4 * k + 3]));
}

__device__ __forceinline__ bool reproj_gate(const MappingDev& m, const float* Rcw, const float* tcw, const float x3D[3], const Kp& kp, bool stereo,
                                            float ur, float sig) {
    const float z = ((Rcw[6] * x3D[0] + Rcw[7] * x3D[1]) + Rcw[8] * x3D[2]) + tcw[2];
    if (z <= 0) return false;
    const float x = ((Rcw[0] * x3D[0] + Rcw[1] * x3D[1]) + Rcw[2] * x3D[2]) + tcw[0];
    const float y = ((Rcw[3] * x3D[0] + Rcw[4] * x3D[1]) + Rcw[5] * x3D[2]) + tcw[1];
    const float invz = (float)(1.0 / (double)z);
    if (!stereo) {
        const float u = m.fx * x / z + m.cx, v = m.fy * y / z + m.cy;
        const float ex = u - kp.x, ey = v - kp.y;
        return !((double)(ex * ex + ey * ey) > 5.991 * (double)sig);
    }
    const float u = m.fx * x * invz + m.cx, u_r = u - m.mbf * invz, v = m.fy * y * invz + m.cy;
    const float ex = u - kp.x, ey = v - kp.y, er = u_r - ur;
    return !((double)(ex * ex + ey * ey + er * er) > 7.8 * (double)sig);
}

// keypoint idx1 of the current keyframe and its match in neighbour j: the body shared by k_tri_points and k_tri_points_batch
__device__ __forceinline__ void tri_point_pair(const MappingDev& m, int j, int idx1) {
    const KfDev& k1 = m.cur;
    const KfDev& k2 = m.neigh[j];
    if (idx1 >= k1.n || k2.skip) return;
    const size_t slot = (size_t)j * k1.n + idx1;
    const int idx2 = m.match[slot];
    if (idx2 < 0) return;
    const Kp kp1 = load_kp(k1.keys, idx1), kp2 = load_kp(k2.keys, idx2);
    const float ur1 = k1.u_right[idx1], ur2 = k2.u_right[idx2];
    const bool stereo1 = ur1 >= 0, stereo2 = ur2 >= 0;
    const float* R1 = k1.Rcw; const float* R2 = k2.Rcw;
    const float xn1[3] = {(kp1.x - m.cx) / m.fx, (kp1.y - m.cy) / m.fy, 1.f};
    const float xn2[3] = {(kp2.x - m.cx) / m.fx, (kp2.y - m.cy) / m.fy, 1.f};
    float ray1[3], ray2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        ray1[r] = (R1[r] * xn1[0] + R1[3 + r] * xn1[1]) + R1[6 + r] * xn1[2];
        ray2[r] = (R2[r] * xn2[0] + R2[3 + r] * xn2[1]) + R2[6 + r] * xn2[2];
    }
    const float dot = (ray1[0] * ray2[0] + ray1[1] * ray2[1]) + ray1[2] * ray2[2];
    const float n1 = sqrtf((ray1[0] * ray1[0] + ray1[1] * ray1[1]) + ray1[2] * ray1[2]);
    const float n2 = sqrtf((ray2[0] * ray2[0] + ray2[1] * ray2[1]) + ray2[2] * ray2[2]);
    const float cosRays = dot / (n1 * n2);
    float cosS1 = cosRays + 1, cosS2 = cosRays + 1;
    if (stereo1) cosS1 = (float)cos(2 * atan2((double)(m.mb / 2), (double)k1.depth[idx1]));
    else if (stereo2) cosS2 = (float)cos(2 * atan2((double)(m.mb / 2), (double)k2.depth[idx2]));
    const float cosS = fminf(cosS1, cosS2);
    float x3D[3];
    bool point_stereo = false;
    const float invfx = 1.0f / m.fx, invfy = 1.0f / m.fy;
    if (cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || (cosRays < 0.9996 && m.inertial) || (cosRays < 0.9998 && !m.inertial))) {
        float A[16];
        const float T1[12] = {R1[0], R1[1], R1[2], k1.t[0], R1[3], R1[4], R1[5], k1.t[1], R1[6], R1[7], R1[8], k1.t[2]};
        const float T2[12] = {R2[0], R2[1], R2[2], k2.t[0], R2[3], R2[4], R2[5], k2.t[1], R2[6], R2[7], R2[8], k2.t[2]};
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            A[c] = xn1[0] * T1[8 + c] - T1[c];
            A[4 + c] = xn1[1] * T1[8 + c] - T1[4 + c];
            A[8 + c] = xn2[0] * T2[8 + c] - T2[c];
            A[12 + c] = xn2[1] * T2[8 + c] - T2[4 + c];
        }
        double M[16], v[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                double s = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) s += (double)A[4 * k + r] * (double)A[4 * k + c];
                M[4 * r + c] = s;
            }
        smallest_eigenvector4(M, v);
        const float h3 = (float)v[3];
        if (h3 == 0) return;
        x3D[0] = (float)v[0] / h3; x3D[1] = (float)v[1] / h3; x3D[2] = (float)v[2] / h3;
    } else if (stereo1 && cosS1 < cosS2) {
        point_stereo = true;
        const float z = k1.depth[idx1];
        if (!(z > 0)) return;
        const float xc[3] = {(kp1.x - m.cx) * z * invfx, (kp1.y - m.cy) * z * invfy, z};
#pragma unroll
        for (int r = 0; r < 3; ++r) x3D[r] = ((R1[r] * xc[0] + R1[3 + r] * xc[1]) + R1[6 + r] * xc[2]) + k1.Ow[r];
    } else if (stereo2 && cosS2 < cosS1) {
        point_stereo = true;
        const float z = k2.depth[idx2];
        if (!(z > 0)) return;
        const float xc[3] = {(kp2.x - m.cx) * z * invfx, (kp2.y - m.cy) * z * invfy, z};
#pragma unroll
        for (int r = 0; r < 3; ++r) x3D[r] = ((R2[r] * xc[0] + R2[3 + r] * xc[1]) + R2[6 + r] * xc[2]) + k2.Ow[r];
    } else {
        return;
    }
    if (!reproj_gate(m, R1, k1.t, x3D, kp1, stereo1, ur1, m.level_sigma2[kp1.octave])) return;
    if (!reproj_gate(m, R2, k2.t, x3D, kp2, stereo2, ur2, m.level_sigma2[kp2.octave])) return;
    const float d1[3] = {x3D[0] - k1.Ow[0], x3D[1] - k1.Ow[1], x3D[2] - k1.Ow[2]}, d2[3] = {x3D[0] - k2.Ow[0], x3D[1] - k2.Ow[1], x3D[2] - k2.Ow[2]};
    const float dist1 = sqrtf((d1[0] * d1[0] + d1[1] * d1[1]) + d1[2] * d1[2]), dist2 = sqrtf((d2[0] * d2[0] + d2[1] * d2[1]) + d2[2] * d2[2]);
    if (dist1 == 0 || dist2 == 0) return;
    if (m.far_points && (dist1 >= m.th_far || dist2 >= m.th_far)) return;
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = m.scale_factors[kp1.octave] / m.scale_factors[kp2.octave];
    if (ratioDist * m.ratio_factor < ratioOctave || ratioDist > ratioOctave * m.ratio_factor) return;
    m.ok[slot] = point_stereo ? 3 : 1;
    m.x3D[3 * slot] = x3D[0]; m.x3D[3 * slot + 1] = x3D[1]; m.x3D[3 * slot + 2] = x3D[2];
}

__global__ __launch_bounds__(128) void k_tri_points(MappingDev m) { tri_point_pair(m, blockIdx.y, blockIdx.x * 128 + threadIdx.x); }
__global__ __launch_bounds__(128) void k_tri_points_batch(const MappingDev* __restrict__ problems, const PairRef* __restrict__ pairs, int chunks) {
    const PairRef pr = pairs[blockIdx.x / chunks];
    const MappingDev m = problems[pr.problem];
    tri_point_pair(m, pr.neighbour, (blockIdx.x % chunks) * 128 + threadIdx.x);
}

// The "first neighbour that yields a point keeps the keypoint" rule of LocalMapping::CreateNewMapPoints and the ordered output
// (neighbour-major, keypoint-ascending), one workgroup per problem.  first[i] = the smallest j with ok[j][i]; a wavefront counts the
// keypoints of its neighbours (j = wave, wave + 4, ...) with ballots, wavefront 0 scans the counts over the neighbours, and the second
// walk over the same 64-wide strides gives every point the rank base + mbcnt(ballot).  No atomic takes part: the order is a function
// of ok alone.  The count is written whatever the room; records beyond the problem's room are dropped (the host reports it).
__global__ __launch_bounds__(256) void k_new_points_compact(const MappingDev* __restrict__ problems, const NewPointsOut* __restrict__ outs,
                                                            int32_t* neigh_count, int32_t* n_points, uint8_t* records) {
    __shared__ int32_t s_first[kNewPointsMaxKeys];
    const MappingDev m = problems[blockIdx.x];
    const NewPointsOut o = outs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = m.cur.n, nn = m.n_neigh;
    int32_t* cnt = neigh_count + o.pair_first;
    for (int i = tid; i < n; i += 256) {
        int first = -1;
        for (int j = 0; j < nn; ++j)
            if (m.ok[(size_t)j * n + i]) { first = j; break; }
        s_first[i] = first;
    }
    __syncthreads();
    for (int j = wave; j < nn; j += 4) {
        int c = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            c += __popcll(__ballot(i < n && s_first[i] == j));
        }
        if (lane == 0) cnt[j] = c;
    }
    __syncthreads();
    if (wave == 0) {  // exclusive scan over the neighbours, 64 at a time with a running base
        int run = 0;
        for (int base = 0; base < nn; base += 64) {
            const int j = base + lane;
            const int c = j < nn ? cnt[j] : 0;
            int incl = c;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d, 64); if (lane >= d) incl += t; }
            if (j < nn) cnt[j] = run + incl - c;
            run += __shfl(incl, 63, 64);
        }
        if (lane == 0) n_points[blockIdx.x] = run;
    }
    __syncthreads();
    for (int j = wave; j < nn; j += 4) {
        int run = cnt[j];
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool mine = i < n && s_first[i] == j;
            const unsigned long long mask = __ballot(mine);
            const int rank = run + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
            if (mine && rank < o.room) {
                const size_t slot = (size_t)j * n + i;
                int32_t* r = reinterpret_cast<int32_t*>(records + 32 * ((size_t)o.first_record + rank));  // tc2li_new_map_point
                r[0] = i; r[1] = j; r[2] = m.match[slot]; r[3] = (m.ok[slot] & 2) ? 1 : 0;
                r[4] = __float_as_int(m.x3D[3 * slot]); r[5] = __float_as_int(m.x3D[3 * slot + 1]); r[6] = __float_as_int(m.x3D[3 * slot + 2]);
                r[7] = 0;
            }
            run += __popcll(mask);
        }
    }
}

// ORBmatcher::Fuse, the search of one map point (SF/src/ORBmatcher.cc:1185-1300): projection and gates, predicted level, the
// keypoints of the window on the keyframe's feature grid, level / reprojection gates, best descriptor distance
// the search itself is fuse_search_one of fuse_search.hpp, shared with the host twin of SearchInNeighbors
// map point i of the list against the keyframe: the body shared by k_fuse_search and k_fuse_search_batch
__device__ __forceinline__ void fuse_point(const FuseDev& f, int i) {
    if (i >= f.n_points) return;
    int best_idx = -1, best_dist = 256;
    const float* P = reinterpret_cast<const float*>(f.points + 68 * (size_t)i);  // pos 3, normal 3, min, max, max_raw, descriptor
    if (f.valid[i]) fuse_search_one(f, P, &best_idx, &best_dist);
    f.best_dist[i] = best_dist;
    f.best_idx[i] = best_idx;
}

__global__ __launch_bounds__(128) void k_fuse_search(FuseDev f) { fuse_point(f, blockIdx.x * 128 + threadIdx.x); }
// every (item, point) of a batch: `chunks` workgroups per item, the items' FuseDev records (grids of the keyframe store) in a device table
__global__ __launch_bounds__(128) void k_fuse_search_batch(const FuseDev* __restrict__ items, int chunks) {
    const FuseDev f = items[blockIdx.x / chunks];
    fuse_point(f, (blockIdx.x % chunks) * 128 + threadIdx.x);
}

void launch_fuse_search(const FuseDev& f, hipStream_t st) {
    if (f.n_points > 0) TC2LI_LAUNCH(k_fuse_search, dim3((f.n_points + 127) / 128), dim3(128), 0, st, f);
}

void launch_fuse_search_batch(const FuseDev* items, int n_items, int max_points, hipStream_t st) {
    const int chunks = (max_points + 127) / 128;
    if (n_items > 0 && chunks > 0) TC2LI_LAUNCH(k_fuse_search_batch, dim3((unsigned)n_items * chunks), dim3(128), 0, st, items, chunks);
}
void launch_new_points_batch(const MappingDev* problems, int n_problems, const PairRef* pairs, int n_pairs, int max_entries, int max_keys,
                             const NewPointsOut* outs, int32_t* neigh_count, int32_t* n_points, uint8_t* records, hipStream_t st) {
    const int cs = (max_entries + 255) / 256, cp = (max_keys + 127) / 128;
    if (n_pairs > 0 && cs > 0) TC2LI_LAUNCH(k_tri_search_batch, dim3((unsigned)n_pairs * cs), dim3(256), 0, st, problems, pairs, cs);
    if (n_pairs > 0 && cp > 0) TC2LI_LAUNCH(k_tri_points_batch, dim3((unsigned)n_pairs * cp), dim3(128), 0, st, problems, pairs, cp);
    if (n_problems > 0) TC2LI_LAUNCH(k_new_points_compact, dim3(n_problems), dim3(256), 0, st, problems, outs, neigh_count, n_points, records);
}

void launch_tri_search(const MappingDev& m, int max_entries, hipStream_t st) {
    if (m.n_neigh > 0 && max_entries > 0) TC2LI_LAUNCH(k_tri_search, dim3((max_entries + 255) / 256, m.n_neigh), dim3(256), 0, st, m);
}
void launch_tri_points(const MappingDev& m, hipStream_t st) {
    if (m.n_neigh > 0 && m.cur.n > 0) TC2LI_LAUNCH(k_tri_points, dim3((m.cur.n + 127) / 128, m.n_neigh), dim3(128), 0, st, m);
}

}  // namespace tc2li

// Host arithmetic shared by the single-keyframe entries (mapping_host.cpp) and the batch entries over the keyframe store
// (keyframe_store.cpp): the view checks, a keyframe's pose constants, the per-pair constants of ORBmatcher::SearchForTriangulation
// (epipole, fundamental matrix) and the baseline of LocalMapping::CreateNewMapPoints -- float arithmetic in the order of Sophus /
// Eigen (SF/src/ORBmatcher.cc:919-944, SF/src/CameraModels/Pinhole.cpp:118-121).  One definition, so both paths hand the kernels
// the same bits.
#pragma once
#include <cmath>
#include <cstring>

#include "common.hpp"
#include "mapping_device.hpp"

namespace tc2li {
namespace mapping_host {

struct Q7 { float q[4], t[3]; };
inline void q_mul(const float a[4], const float b[4], float o[4]) {
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
}
inline void q_rot(const float q[4], const float v[3], float out[3]) {
    float uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    out[0] = v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]);
    out[1] = v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]);
    out[2] = v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0]);
}
inline void q_mat(const float q[4], float R[9]) {
    const float tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const float txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const float tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
inline Q7 inv7(const Q7& T) {
    Q7 o;
    o.q[0] = -T.q[0]; o.q[1] = -T.q[1]; o.q[2] = -T.q[2]; o.q[3] = T.q[3];
    const float nt[3] = {T.t[0] * -1.f, T.t[1] * -1.f, T.t[2] * -1.f};
    q_rot(o.q, nt, o.t);
    return o;
}
inline Q7 mul7(const Q7& a, const Q7& b) {
    Q7 o;
    q_mul(a.q, b.q, o.q);
    float r[3];
    q_rot(a.q, b.t, r);
    for (int c = 0; c < 3; ++c) o.t[c] = r[c] + a.t[c];
    return o;
}
inline void m3_mul(const float* a, const float* b, float* o) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) o[3 * r + c] = (a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c]) + a[3 * r + 2] * b[6 + c];
}
inline void m3_inv(const float* m, float* o) {
    const float c00 = m[4] * m[8] - m[5] * m[7], c10 = m[5] * m[6] - m[3] * m[8], c20 = m[3] * m[7] - m[4] * m[6];
    const float det = (m[0] * c00 + m[1] * c10) + m[2] * c20;
    const float id = 1.0f / det;
    o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c10 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c20 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// Tcw of a keyframe: rotation matrix and camera centre as the kernels read them
inline void set_pose(KfDev& d, const float pose7[7]) {
    memcpy(d.q, pose7, 16); memcpy(d.t, pose7 + 4, 12);
    q_mat(d.q, d.Rcw);
    Q7 T; memcpy(T.q, d.q, 16); memcpy(T.t, d.t, 12);
    const Q7 Tw = inv7(T);
    memcpy(d.Ow, Tw.t, 12);
}

inline float baseline(const KfDev& k1, const KfDev& k2) {
    const float vb[3] = {k2.Ow[0] - k1.Ow[0], k2.Ow[1] - k1.Ow[1], k2.Ow[2] - k1.Ow[2]};
    return std::sqrt(vb[0] * vb[0] + vb[1] * vb[1] + vb[2] * vb[2]);
}

inline int check_view(const tc2li_keyframe_view* v, const char* what) {
    if (!v || v->n < 0 || v->n_nodes < 0 || (v->n > 0 && (!v->keys || !v->descriptors || !v->u_right || !v->depth || !v->has_point)) ||
        (v->n_nodes > 0 && (!v->fv_node || !v->fv_offset || !v->fv_index))) {
        set_error("%s: invalid keyframe view", what);
        return TC2LI_ERR_INVALID;
    }
    if (v->n_nodes > 0) {
        if (v->fv_offset[0] != 0) { set_error("%s: fv_offset[0] must be 0", what); return TC2LI_ERR_INVALID; }
        for (int a = 0; a < v->n_nodes; ++a) {
            if (v->fv_offset[a + 1] < v->fv_offset[a] || (a > 0 && v->fv_node[a] <= v->fv_node[a - 1])) { set_error("%s: feature vector not ascending", what); return TC2LI_ERR_INVALID; }
        }
        for (int k = 0; k < v->fv_offset[v->n_nodes]; ++k)
            if (v->fv_index[k] < 0 || v->fv_index[k] >= v->n) { set_error("%s: feature index out of range", what); return TC2LI_ERR_INVALID; }
    }
    return 0;
}

// epipole of the current keyframe in the neighbour and F12 (the same pinhole camera on both sides)
inline void pair_constants(const KfDev& k1, KfDev& k2, const tc2li_camera* cam) {
    Q7 T1, T2;
    memcpy(T1.q, k1.q, 16); memcpy(T1.t, k1.t, 12); memcpy(T2.q, k2.q, 16); memcpy(T2.t, k2.t, 12);
    float C2[3];
    q_rot(T2.q, k1.Ow, C2);
    for (int c = 0; c < 3; ++c) C2[c] += T2.t[c];
    const float fx = (float)cam->fx, fy = (float)cam->fy, cx = (float)cam->cx, cy = (float)cam->cy;
    k2.ep[0] = fx * C2[0] / C2[2] + cx; k2.ep[1] = fy * C2[1] / C2[2] + cy;
    const Q7 T12 = mul7(T1, inv7(T2));
    float R12[9];
    q_mat(T12.q, R12);
    const float K[9] = {fx, 0.f, cx, 0.f, fy, cy, 0.f, 0.f, 1.f};
    const float Kt[9] = {K[0], K[3], K[6], K[1], K[4], K[7], K[2], K[5], K[8]};
    const float tx[9] = {0.f, -T12.t[2], T12.t[1], T12.t[2], 0.f, -T12.t[0], -T12.t[1], T12.t[0], 0.f};
    float KtInv[9], KInv[9], a[9], b[9];
    m3_inv(Kt, KtInv);
    m3_inv(K, KInv);
    m3_mul(KtInv, tx, a);
    m3_mul(a, R12, b);
    m3_mul(b, KInv, k2.F12);
}

inline bool octaves_ok(const tc2li_keyframe_view* v, int n_levels) {
    for (int i = 0; i < v->n; ++i) if (v->keys[i].octave < 0 || v->keys[i].octave >= n_levels) return false;
    return true;
}

}  // namespace mapping_host
}  // namespace tc2li

// Sophus::SE3f in float, for host and device: the operations of the reference's pose algebra in the order Sophus writes them, every
// product and sum rounded (no contraction).  The same functions as lidar_pose_host.cpp:34-73, which fixed these evaluations first.
//   unit         SO3::normalize (so3.hpp): len = sqrt(x*x + y*y + z*z + w*w), summed left to right, then four divisions
//   spin         SO3 * point (so3.hpp:358-367): uv = q.vec x p; uv += uv; p + w * uv + q.vec x uv, summed left to right
//   rotation_of  Eigen's QuaternionBase::toRotationMatrix
//   inverse      SE3::inverse (se3.hpp:208-211): the conjugate goes through the SO3(Quaternion) constructor, which normalises it again;
//                the translation is invR * (t * -1)
//   compose      SO3 * SO3 (so3.hpp:325-339): the quaternion product, then normalize(); SE3 * SE3 (se3.hpp:304-308): t_a + R_a * t_b
// Where Eigen leaves a summation order to its build, THESE CHOICES DEFINE PARITY (as include/tc2li_hip.h does for the culling norm):
//   a 3-term row sum of a matrix-vector product is ((a*x + b*y) + c*z), a translation is added after it;
//   a vector norm is sqrtf((x*x + y*y) + z*z), the order of k_map_points_refresh.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#pragma clang fp contract(off)

namespace tc2li {
namespace se3f {

struct Quat { float x, y, z, w; };
struct Vec3 { float v[3]; };
struct Mat3 { float m[9]; };   // row-major
struct Pose {                  // Sophus::SE3f; across the ABI seven floats: x, y, z, w, then the translation
    Quat q;
    Vec3 t;
};

__host__ __device__ inline Pose from7(const float* p) { return Pose{Quat{p[0], p[1], p[2], p[3]}, Vec3{{p[4], p[5], p[6]}}}; }
__host__ __device__ inline void to7(const Pose& T, float* p) {
    p[0] = T.q.x; p[1] = T.q.y; p[2] = T.q.z; p[3] = T.q.w; p[4] = T.t.v[0]; p[5] = T.t.v[1]; p[6] = T.t.v[2];
}

__host__ __device__ inline Quat unit(const Quat& q) {
    const float len = sqrtf(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    return Quat{q.x / len, q.y / len, q.z / len, q.w / len};
}
__host__ __device__ inline Vec3 spin(const Quat& q, const Vec3& p) {
    float a[3] = {q.y * p.v[2] - q.z * p.v[1], q.z * p.v[0] - q.x * p.v[2], q.x * p.v[1] - q.y * p.v[0]};
    for (int k = 0; k < 3; ++k) a[k] = a[k] + a[k];
    const float b[3] = {q.y * a[2] - q.z * a[1], q.z * a[0] - q.x * a[2], q.x * a[1] - q.y * a[0]};
    return Vec3{{p.v[0] + q.w * a[0] + b[0], p.v[1] + q.w * a[1] + b[1], p.v[2] + q.w * a[2] + b[2]}};
}
__host__ __device__ inline Mat3 rotation_of(const Quat& q) {
    const float tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const float twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y,
                tzz = tz * q.z;
    return Mat3{{1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)}};
}
// SO3::inverse: SO3(unit_quaternion().conjugate())
__host__ __device__ inline Quat inverse_q(const Quat& q) { return unit(Quat{-q.x, -q.y, -q.z, q.w}); }
__host__ __device__ inline Quat compose_q(const Quat& a, const Quat& b) {
    return unit(Quat{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                     a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z});
}
__host__ __device__ inline Pose inverse(const Pose& T) {
    Pose o;
    o.q = inverse_q(T.q);
    o.t = spin(o.q, Vec3{{T.t.v[0] * -1.0f, T.t.v[1] * -1.0f, T.t.v[2] * -1.0f}});
    return o;
}
__host__ __device__ inline Pose compose(const Pose& A, const Pose& B) {
    Pose o;
    o.q = compose_q(A.q, B.q);
    const Vec3 r = spin(A.q, B.t);
    for (int k = 0; k < 3; ++k) o.t.v[k] = A.t.v[k] + r.v[k];
    return o;
}
// SE3 * point: so3() * p + translation()
__host__ __device__ inline Vec3 act(const Pose& T, const Vec3& p) {
    const Vec3 r = spin(T.q, p);
    return Vec3{{r.v[0] + T.t.v[0], r.v[1] + T.t.v[1], r.v[2] + T.t.v[2]}};
}
// row r of M * x: ((a*x + b*y) + c*z)
__host__ __device__ inline float row_dot(const Mat3& M, int r, const float* x) { return (M.m[3 * r] * x[0] + M.m[3 * r + 1] * x[1]) + M.m[3 * r + 2] * x[2]; }
__host__ __device__ inline float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

}  // namespace se3f
}  // namespace tc2li

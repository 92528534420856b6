// tpamd_quat.h -- the quaternion arithmetic of the pose-spline samplers (k_sample_pose_splines in
// tpamd_kernels.h, k_sample_ik_targets in tpamd_pose_fit.hip): BSplineQ's QuatPower = exp(p log q)
// (splines/bsplineq.cc:98-146) with Eigen's stableNorm / stableNormalized of the vector part.
// Quaternions are [w, x, y, z]. The operations follow the reference in order; log / atan2 / sin /
// cos / exp come from the device math library.
#pragma once

#include <hip/hip_runtime.h>

namespace tpamd {

struct Quat { double w, x, y, z; };

__device__ __forceinline__ Quat quat_mul(const Quat &a, const Quat &b) {
  Quat r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  return r;
}
__device__ __forceinline__ double quat_sqnorm(const Quat &q) { return q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w; }
__device__ __forceinline__ Quat quat_inverse(const Quat &q) {
  const double n2 = quat_sqnorm(q);
  Quat r = {0.0, 0.0, 0.0, 0.0};
  if (n2 > 0.0) { r.w = q.w / n2; r.x = -q.x / n2; r.y = -q.y / n2; r.z = -q.z / n2; }
  return r;
}
// bsplineq.cc:98-108
__device__ __forceinline__ void quat_normalize_positive_real(Quat &q) {
  if (q.w < 0) { q.w *= -1.0; q.x *= -1.0; q.y *= -1.0; q.z *= -1.0; }
  if (fabs(quat_sqnorm(q) - 1.0) > 1e-12) {
    const double n = sqrt(quat_sqnorm(q));
    q.w /= n; q.x /= n; q.y /= n; q.z /= n;
  }
}
// Eigen stableNorm / stableNormalized of the vector part (restated as in the oracle)
__device__ __forceinline__ double vec3_stable_norm(double x, double y, double z) {
  double mx = fabs(x);
  if (fabs(y) > mx) mx = fabs(y);
  if (fabs(z) > mx) mx = fabs(z);
  if (!(mx > 0.0)) return mx;
  const double inv = 1.0 / mx;
  const double a = x * inv, b = y * inv, c = z * inv;
  return mx * sqrt(a * a + b * b + c * c);
}
__device__ __forceinline__ void vec3_stable_normalized(double &x, double &y, double &z) {
  double w = fabs(x);
  if (fabs(y) > w) w = fabs(y);
  if (fabs(z) > w) w = fabs(z);
  const double a = x / w, b = y / w, c = z / w;
  const double zz = a * a + b * b + c * c;
  if (zz > 0.0) {
    const double s = sqrt(zz);
    x = a / s; y = b / s; z = c / s;
  }
}
// bsplineq.cc:136-146 with QuatLog :112-125 and QuatExp :127-134
__device__ __forceinline__ Quat quat_power(Quat q, double power) {
  quat_normalize_positive_real(q);
  Quat l;
  {
    const double nv = vec3_stable_norm(q.x, q.y, q.z);
    l.w = 0.5 * log(quat_sqnorm(q));
    if (nv > 1e-12) {
      double nx = q.x, ny = q.y, nz = q.z;
      vec3_stable_normalized(nx, ny, nz);
      const double ang = atan2(nv, q.w);
      l.x = nx * ang; l.y = ny * ang; l.z = nz * ang;
    } else {
      l.x = q.x; l.y = q.y; l.z = q.z;
    }
  }
  l.w *= power; l.x *= power; l.y *= power; l.z *= power;
  Quat r;
  {
    const double nv = vec3_stable_norm(l.x, l.y, l.z);
    double nx = l.x, ny = l.y, nz = l.z;
    r.w = cos(nv);
    vec3_stable_normalized(nx, ny, nz);
    const double sn = sin(nv);
    r.x = nx * sn; r.y = ny * sn; r.z = nz * sn;
    const double e = exp(l.w);
    r.w *= e; r.x *= e; r.y *= e; r.z *= e;
  }
  return r;
}

}  // namespace tpamd

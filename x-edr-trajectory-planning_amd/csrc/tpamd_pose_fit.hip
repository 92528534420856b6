// tpamd_pose_fit.hip -- the two kernels of tpamd_pose_fit.h in a translation unit of their own.
#include <hip/hip_runtime.h>

#include "tpamd_device.h"          // knot_span_deg2, basis_ders_deg2
#include "tpamd_quat.h"            // Quat, quat_mul, quat_inverse, quat_power

#define TPAMD_HD_ROUTINES_ONLY     // sw_polyline, not the switch and readout kernels
#include "tpamd_pose_fit.h"

namespace tpamd {

// One thread per listed path (W is tens at most): the fit straight into the path's packed slots.
static __global__ void __launch_bounds__(64) k_fit_pose_waypoints(PoseFitParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.Q) return;
  const int D = p.D;
  const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0;
  if (W < 1) {             // "no waypoints": no slots, nothing else written
    p.num_points[k] = 0;
    p.path_end[k] = 0.0;
    p.status[k] = kSwInvalidArgument;
    return;
  }
  const size_t po = (size_t)p.point_offsets[k];
  double *knots = p.knots + (size_t)p.knot_offsets[k];
  const int P = fit_pose_waypoints(p.pose_wps + (size_t)w0 * 7, p.joint_wps + (size_t)w0 * D, W, D,
                                   p.translation_rounding[k], p.rotation_rounding[k], knots, p.trans + po * 3,
                                   p.rot + po * 4, p.joint_cp + po * D);
  p.num_points[k] = P;
  p.path_end[k] = knots[P + 2];
  p.status[k] = kSwOk;
}

void launch_fit_pose_waypoints(const PoseFitParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_fit_pose_waypoints, dim3((unsigned)((p.Q + 63) / 64)), dim3(64), 0, st, p);
}

// One thread per (path, row); grid (ceil(max rows / 256), paths). A block's 256 consecutive rows
// touch a short run of consecutive knots and control points: they are read from global memory (L2),
// so a path of any size is sampled.
static __global__ void __launch_bounds__(256) k_sample_ik_targets(IkTargetParams p) {
  const int k = blockIdx.y;
  const int r0 = p.row_offsets[k], rows = p.row_offsets[k + 1] - r0;
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const double delta = p.delta[k];
  if (!(delta > 0.0)) return;                 // the path's rows stay untouched
  const int P = p.num_points[k], K = P + 3, D = p.D;
  const double *knots = p.knots + (size_t)p.knot_offsets[k];
  const size_t po = (size_t)p.point_offsets[k];
  const double *tr = p.trans + po * 3, *ro = p.rot + po * 4, *jc = p.joint_cp + po * D;
  double *pose = p.pose_targets + ((size_t)r0 + r) * 7;
  double *joint = p.joint_targets + ((size_t)r0 + r) * D;
  const double kend = knots[K - 1];
  // table row first_row[k] + r belongs to (first_row[k] + r) * delta, never to an accumulated
  // parameter: a row's targets do not depend on which call samples it
  const double parameter = ((p.first_row ? p.first_row[k] : 0) + r) * delta;
  if (!(parameter < kend - delta) || parameter < knots[0]) {
    // from knots.back() - delta on: the last control pose and joint control point (a first knot
    // above 0 is the caller's error; its rows get the last pose as well rather than garbage)
    for (int d = 0; d < 3; d++) pose[d] = tr[3 * (size_t)(P - 1) + d];
    for (int d = 0; d < 4; d++) pose[3 + d] = ro[4 * (size_t)(P - 1) + d];
    for (int d = 0; d < D; d++) joint[d] = jc[(size_t)(P - 1) * D + d];
    return;
  }
  const int span = knot_span_deg2(knots, K, parameter);
  double ders[3][3];
  basis_ders_deg2(knots, span, parameter, ders);     // ders[0][*]: the basis of NURBS A2.2
  const double b0 = ders[0][0], b1 = ders[0][1], b2 = ders[0][2];
  const double *t0 = tr + 3 * (size_t)(span - 2);
  for (int d = 0; d < 3; d++) {
    double v = 0.0;
    v += b0 * t0[d]; v += b1 * t0[3 + d]; v += b2 * t0[6 + d];
    pose[d] = v;
  }
  const double cum1 = b2, cum0 = cum1 + b1;            // bsplineq.cc:313-316
  const double *q0 = ro + 4 * (size_t)(span - 2);
  const Quat p0 = {q0[0], q0[1], q0[2], q0[3]}, p1 = {q0[4], q0[5], q0[6], q0[7]},
             p2 = {q0[8], q0[9], q0[10], q0[11]};
  Quat q = p0;
  q = quat_mul(q, quat_power(quat_mul(quat_inverse(p0), p1), cum0));
  q = quat_mul(q, quat_power(quat_mul(quat_inverse(p1), p2), cum1));
  quat_normalize_positive_real(q);
  pose[3] = q.w; pose[4] = q.x; pose[5] = q.y; pose[6] = q.z;
  const double *j0 = jc + (size_t)(span - 2) * D, *j1 = j0 + D, *j2 = j1 + D;
  for (int d = 0; d < D; d++) {                        // BSplineT::EvalCurve
    double v = 0.0;
    v += b0 * j0[d]; v += b1 * j1[d]; v += b2 * j2[d];
    joint[d] = v;
  }
}

void launch_sample_ik_targets(const IkTargetParams &p, int max_rows, hipStream_t st) {
  if (max_rows < 1 || p.Q < 1) return;
  hipLaunchKernelGGL(k_sample_ik_targets, dim3((unsigned)((max_rows + 255) / 256), (unsigned)p.Q), dim3(256), 0, st,
                     p);
}

}  // namespace tpamd

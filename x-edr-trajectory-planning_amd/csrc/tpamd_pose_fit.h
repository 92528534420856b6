// tpamd_pose_fit.h -- Cartesian goals on the device (include/tpamd.h tpamd_fit_pose_waypoints_*,
// tpamd_sample_ik_targets_*): the two stages that surround the user's IK.
//
// Fit: TimeableCartesianSplinePath::SetWaypoints / FitSplineToWaypoints
// (timeable_path_cartesian_spline.cc:415-482 as the host mirror restates them:
// host/timeable_path_cartesian_spline.cc) for every listed path:
//   1. an empty waypoint list is an error (InvalidArgument);
//   2. joint control points: PolyLineToControlPoints with the ROTATION rounding as the radius
//      (sw_polyline, tpamd_switch.h; the mirror passes options_.rounding());
//   3. pose control points: PolyLineToBspline3Waypoints on poses (splines/spline_utils.cc:150-204):
//      W = 1 gives four copies, otherwise P = 3 W - 2 poses with out[3 i] corner i and each
//      neighbour out[k] * CornerOffset(out[k].inverse() * out[k +- 3], translation radius, rotation
//      radius), the interior corners first, then out[1] and out[P - 2];
//   4. the uniform degree-2 knots [P + 3] on [0, 1] by running accumulation;
//   5. every knot multiplied by max(L + L, 0.1) * 10, L the length of the translation control
//      polygon ("translation + translation" is the reference's, :436-438).
// Pose3d product and inverse, quaternion product, quaternion times vector and
// AngleAxisd(Quaterniond) are those of host/compat.h:133-214, operation by operation. Quaternions
// are [w, x, y, z] and are not normalised; any rounding value passes (only CornerOffset's 1e-6 rule).
//
// fit_pose_waypoints compiles for the host as well (TPAMD_HD): tests/cpp/test_pose_fit.cc holds it
// bit-equal to the mirror there (both sides glibc, -ffp-contract=off). On the device atan2, sin and
// cos come from the device math library: the pose control points and the knots agree with the host to
// rounding; the joint control points (no libm call) stay bit-equal.
//
// Targets: what ExtendIkSolution (timeable_path_cartesian_spline.cc:484-526) evaluates for the IK
// callback, for a ragged batch: row r of path k belongs to parameter r * delta[k]; below
// knots.back() - delta the pose target is the translation spline and the BSplineQ::EvalCurve
// quaternion (as k_sample_pose_splines, tpamd_kernels.h) and the joint target the joint spline's
// EvalCurve with the same basis; from there on the last control pose and the last joint control
// point, bit for bit.
#pragma once

#include "tpamd_fit.h"          // fit_points, sw_polyline, TPAMD_HD, kSw*

namespace tpamd {

// A pose as the packed arrays hold it: translation, then quaternion (w, x, y, z).
struct PfPose {
  double t[3];
  double q[4];
};

// compat::Quaterniond::operator*(Quaterniond): Hamilton product
TPAMD_HD inline void pf_quat_mul(const double *a, const double *b, double *r) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  const double x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  const double z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
  r[0] = w; r[1] = x; r[2] = y; r[3] = z;
}

// compat::Quaterniond::operator*(Vector3d): Eigen's _transformVector
TPAMD_HD inline void pf_quat_rotate(const double *q, const double *p, double *r) {
  const double u0 = q[1], u1 = q[2], u2 = q[3], w = q[0];
  const double c0 = (u1 * p[2] - u2 * p[1]) * 2.0;
  const double c1 = (u2 * p[0] - u0 * p[2]) * 2.0;
  const double c2 = (u0 * p[1] - u1 * p[0]) * 2.0;
  const double r0 = (p[0] + c0 * w) + (u1 * c2 - u2 * c1);
  const double r1 = (p[1] + c1 * w) + (u2 * c0 - u0 * c2);
  const double r2 = (p[2] + c2 * w) + (u0 * c1 - u1 * c0);
  r[0] = r0; r[1] = r1; r[2] = r2;
}

// compat::Pose3d::inverse
TPAMD_HD inline PfPose pf_inverse(const PfPose &a) {
  PfPose r;
  const double n2 = a.q[0] * a.q[0] + a.q[1] * a.q[1] + a.q[2] * a.q[2] + a.q[3] * a.q[3];
  if (!(n2 > 0.0)) {
    r.q[0] = r.q[1] = r.q[2] = r.q[3] = 0.0;
  } else {
    r.q[0] = a.q[0] / n2; r.q[1] = -a.q[1] / n2; r.q[2] = -a.q[2] / n2; r.q[3] = -a.q[3] / n2;
  }
  double v[3];
  pf_quat_rotate(r.q, a.t, v);
  for (int d = 0; d < 3; d++) r.t[d] = v[d] * -1.0;
  return r;
}

// compat::Pose3d::operator*
TPAMD_HD inline PfPose pf_mul(const PfPose &a, const PfPose &b) {
  PfPose r;
  pf_quat_mul(a.q, b.q, r.q);
  double v[3];
  pf_quat_rotate(a.q, b.t, v);
  for (int d = 0; d < 3; d++) r.t[d] = a.t[d] + v[d];
  return r;
}

TPAMD_HD inline double pf_norm3(const double *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// CornerOffset (splines/spline_utils.cc:104-148)
TPAMD_HD inline PfPose pf_corner_offset(const PfPose &delta, double translation_radius, double rotation_radius) {
  PfPose offset;
  offset.t[0] = offset.t[1] = offset.t[2] = 0.0;
  offset.q[0] = 1.0; offset.q[1] = offset.q[2] = offset.q[3] = 0.0;
  if (translation_radius < 1e-6 || rotation_radius < 1e-6) return offset;
  const double translation_norm = pf_norm3(delta.t);
  // AngleAxisd(Quaterniond)
  double angle = 0.0, axis[3] = {1.0, 0.0, 0.0};
  double n = pf_norm3(delta.q + 1);
  if (n != 0.0) {
    angle = 2.0 * atan2(n, fabs(delta.q[0]));
    if (delta.q[0] < 0) n = -n;
    axis[0] = delta.q[1] / n; axis[1] = delta.q[2] / n; axis[2] = delta.q[3] / n;
  }
  const double pct_trans = translation_norm == 0.0 ? INFINITY : translation_radius / translation_norm;
  const double pct_rot = angle == 0.0 ? INFINITY : rotation_radius / angle;
  double pct = pct_rot < pct_trans ? pct_rot : pct_trans;            // std::min(pct_trans, pct_rot)
  if (pct > (1.0 / 4.0)) pct = (1.0 / 4.0);                          // kMinWaypointSpacingFactor
  for (int d = 0; d < 3; d++) offset.t[d] = delta.t[d] * pct;
  angle *= pct;
  const double ha = 0.5 * angle;                                     // AngleAxisd::toQuaternion
  const double s = sin(ha);
  offset.q[0] = cos(ha);
  offset.q[1] = s * axis[0]; offset.q[2] = s * axis[1]; offset.q[3] = s * axis[2];
  return offset;
}

TPAMD_HD inline PfPose pf_load(const double *trans, const double *rot, int k) {
  PfPose p;
  for (int d = 0; d < 3; d++) p.t[d] = trans[(size_t)3 * k + d];
  for (int d = 0; d < 4; d++) p.q[d] = rot[(size_t)4 * k + d];
  return p;
}
TPAMD_HD inline void pf_store(double *trans, double *rot, int k, const PfPose &p) {
  for (int d = 0; d < 3; d++) trans[(size_t)3 * k + d] = p.t[d];
  for (int d = 0; d < 4; d++) rot[(size_t)4 * k + d] = p.q[d];
}

// out[k + step] = out[k] * CornerOffset(out[k].inverse() * out[k + 3 step], ...), step = +-1
TPAMD_HD inline void pf_corner(double *trans, double *rot, int k, int step, double tr, double rr) {
  const PfPose a = pf_load(trans, rot, k), b = pf_load(trans, rot, k + 3 * step);
  pf_store(trans, rot, k + step, pf_mul(a, pf_corner_offset(pf_mul(pf_inverse(a), b), tr, rr)));
}

// FitSplineToWaypoints on pose waypoints [W][7] (translation, then quaternion w x y z) and joint
// waypoints [W][D]: knots [P + 3], translation points [P][3], rotation points [P][4], joint control
// points [P][D] with P = fit_points(W). Returns P, or 0 (nothing written) for W < 1.
TPAMD_HD inline int fit_pose_waypoints(const double *pose_wps, const double *joint_wps, int W, int D,
                                       double translation_rounding, double rotation_rounding, double *knots,
                                       double *trans, double *rot, double *joint_cp) {
  if (W < 1) return 0;                                  // "no waypoints"
  const int P = sw_polyline(joint_wps, W, D, rotation_rounding, joint_cp);
  // PolyLineToBspline3Waypoints on the poses
  if (W == 1) {
    for (int k = 0; k < 4; k++) {
      for (int d = 0; d < 3; d++) trans[3 * k + d] = pose_wps[d];
      for (int d = 0; d < 4; d++) rot[4 * k + d] = pose_wps[3 + d];
    }
  } else {
    for (int i = 0; i < W; i++) {
      for (int d = 0; d < 3; d++) trans[(size_t)9 * i + d] = pose_wps[(size_t)7 * i + d];
      for (int d = 0; d < 4; d++) rot[(size_t)12 * i + d] = pose_wps[(size_t)7 * i + 3 + d];
    }
    for (int i = 1; i + 1 < W; i++) {
      pf_corner(trans, rot, 3 * i, +1, translation_rounding, rotation_rounding);
      pf_corner(trans, rot, 3 * i, -1, translation_rounding, rotation_rounding);
    }
    pf_corner(trans, rot, 0, +1, translation_rounding, rotation_rounding);
    pf_corner(trans, rot, P - 1, -1, translation_rounding, rotation_rounding);
  }
  const int nk = P + 2 + 1;                             // kSplineOrder + 1
  const double spacing = (1.0 / (nk - 2.0 * (2 + 1.0) + 1.0)) * (1.0 - 0.0);
  double u = 0.0;
  for (int i = 0; i <= 2; i++) knots[i] = 0.0;
  for (int i = 3; i < nk - 3; i++) {
    u = u + spacing;
    knots[i] = u;
  }
  for (int i = nk - 3; i < nk; i++) knots[i] = 1.0;
  double translation_length = 0.0;
  for (int i = 0; i + 1 < P; i++) {
    double diff[3];
    for (int d = 0; d < 3; d++) diff[d] = trans[(size_t)3 * (i + 1) + d] - trans[(size_t)3 * i + d];
    translation_length += pf_norm3(diff);
  }
  const double twice = translation_length + translation_length;      // sic
  const double weighted = twice < 0.1 ? 0.1 : twice;                 // std::max(.., kMinimumFinalKnotValue)
  const double scale = weighted * 10.0;                              // kPathParameterPerPolygonLength
  for (int i = 0; i < nk; i++) knots[i] *= scale;
  return P;
}

#if defined(__HIPCC__) || defined(__HIP__)
// ------------------------------------------------------------------ the fit kernel
struct PoseFitParams {
  int Q, D;                            // listed paths; joints
  const int *offsets;                  // [Q + 1] waypoint rows of path k: offsets[k] .. offsets[k + 1)
  const int *point_offsets;            // [Q + 1] first control point of path k (an empty path takes none)
  const double *pose_wps;              // [rows][7]
  const double *joint_wps;             // [rows][D]
  const double *translation_rounding;  // [Q]
  const double *rotation_rounding;     // [Q]
  // packed raggedly: path k's knots at point_offsets[k] + 3 k' where k' counts the non-empty paths
  // before k (knot_offsets), its points at point_offsets[k]
  const int *knot_offsets;             // [Q + 1]
  double *knots, *trans, *rot, *joint_cp;
  int *num_points;                     // [Q]
  double *path_end;                    // [Q]
  int *status;                         // [Q] TPAMD_PLAN_*
};

// ------------------------------------------------------------------ the target kernel
struct IkTargetParams {
  int Q, D;
  const int *num_points;               // [Q] P_k >= 3
  const int *point_offsets;            // [Q + 1]
  const int *knot_offsets;             // [Q + 1]
  const int *row_offsets;              // [Q + 1]
  const int *first_row;                // [Q] table row of the path's first output row; null: 0
  const double *knots, *trans, *rot, *joint_cp;
  const double *delta;                 // [Q]; a path whose delta is not > 0 is left untouched
  double *pose_targets;                // [rows][7]
  double *joint_targets;               // [rows][D]
};

// Both kernels live in a translation unit of their own (tpamd_pose_fit.hip).
void launch_fit_pose_waypoints(const PoseFitParams &p, hipStream_t st);
void launch_sample_ik_targets(const IkTargetParams &p, int max_rows, hipStream_t st);
#endif

}  // namespace tpamd

// tpamd_switch.h -- the online path switch of a planner set on the device
// (include/tpamd.h tpamd_planner_set_switch_paths): for every listed planner, on its resident state,
//   1. the fastest-stop path parameter (tpamd_stop.h), unless the caller gives the parameter;
//   2. the velocity at the switch time, TrajectoryBuffer::GetVelocityAtTime
//      (trajectory_buffer.cc:233-275) on the resident trajectory;
//   3. TimeableJointSplinePath::SwitchToWaypointPath (timeable_path_joint_spline.cc:209-250 as the
//      host mirror restates it: host/timeable_path_joint_spline.cc, host/spline_edit.cc):
//      TruncateSplineAt (knot insertion, NURBS A5.1), EvalCurve at the stop point,
//      ProjectPointOnPath, the 1e-3 rule for the projected first waypoint,
//      PolyLineToControlPoints (rounding radius SwitchParams::radius: the PathOptions default 0.2,
//      or the argument of tpamd_planner_set_switch_paths_rounded) and ExtendWithControlPoints;
//   4. the commit: new knots / control points / count, the velocity as the initial velocity
//      (SetInitialVelocity) and path_state = 2 (kModifiedPath). A planner whose switch failed
//      keeps its state bit for bit.
//
// The edit routines below compile for the host as well (TPAMD_HD): tests/cpp/test_switch_edit.cc
// runs them on the CPU against the mirror. They repeat the mirror's arithmetic operation by
// operation (same operands, same order, no contraction: the library is built with
// -ffp-contract=off; '/' and sqrt are correctly rounded on both sides), so the results are
// bit-identical. One thread per planner: the work is O(P D + W D) control flow whose sums are
// ordered, which leaves nothing to split across lanes.
//
// What holds them besides the mirror: tests/switch_reference.py restates the edit from the
// reference's sources and checks what a switch means in exact arithmetic (kept curve, join,
// knots, end point, least-distance projection). tests/cpp/test_switch_reference.cc with
// tests/test_switch_reference_cpu.py holds the routines, the mirror and that restatement
// bit-equal for every D = 1..16; tests/test_gpu_switch_all_dofs.py holds k_pset_switch to it at
// every D (every edge branch, shuffled ids, a partly filled last wave, P_cap growth, the
// committed velocity through the next Plan); tests/cpp/test_set_switch.cc follows 260-planner
// sets at D = 3 and 7 against the mirror. DESIGN.md "What holds the spline edits".
#pragma once

#include <math.h>
#include <float.h>

// TPAMD_HD_ROUTINES_ONLY: the routines without the kernels (tpamd_fit.hip)
#if (defined(__HIPCC__) || defined(__HIP__)) && !defined(TPAMD_HD_ROUTINES_ONLY)
#include "tpamd_planner_set.h"   // pset_time_to_sec
#endif

#include "tpamd_readout.h"     // TPAMD_HD, the trajectory bracket

namespace tpamd {

// TPAMD_PLAN_* (include/tpamd.h) for the Status codes of the mirror's spline edit
enum { kSwOk = 0, kSwFailedPrecondition = 1, kSwOutOfRange = 2, kSwInvalidArgument = 3, kSwInternal = 4 };

constexpr double kSwitchRounding = 0.2;   // PathOptions::rounding() default (host/timeable_path.h)

// A degree-2 B-spline being edited in place: knots [nk] and points [np][D] in arrays with room
// for cap_points points (cap_points + 3 knots). umin / umax as EditableBSpline keeps them.
struct SwSpline {
  double *knots, *pts;
  int nk, np, D;
  int knot_capacity;        // EditableBSpline's knot_capacity_ (the reference's allocation)
  double umin, umax;
  bool empty;
};

// EditableBSpline::KnotSpan, degree 2
TPAMD_HD inline int sw_knot_span(const double *k, int nk, double u) {
  if (nk == 0) return 0;
  if (u == k[nk - 1]) return nk - 2 - 2;
  int lo = 2, hi = nk - 2;
  while (lo < hi) {
    const int mid = lo + (hi - lo) / 2;
    if (k[mid] <= u) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// EditableBSpline::Basis, degree 2
TPAMD_HD inline void sw_basis(const double *k, int span, double u, double *N) {
  double left[3], right[3];
  N[0] = 1.0;
  for (int j = 1; j <= 2; j++) {
    left[j] = u - k[span + 1 - j];
    right[j] = k[span + j] - u;
  }
  for (int j = 1; j <= 2; j++) {
    double saved = 0.0;
    for (int r = 0; r < j; r++) {
      const double tmp = N[r] / (right[r + 1] + left[j - r]);
      N[r] = saved + right[r + 1] * tmp;
      saved = left[j - r] * tmp;
    }
    N[j] = saved;
  }
}

// EditableBSpline::InsertKnotAndUpdateControlPoints (CanInsertKnot first)
TPAMD_HD inline int sw_insert_knot(SwSpline &s, double knot, int multiplicity) {
  if (multiplicity > 3) return kSwInvalidArgument;
  if (s.nk + multiplicity > s.knot_capacity) return kSwFailedPrecondition;
  if (s.nk < 2) return kSwFailedPrecondition;
  if (knot <= s.knots[0] || knot >= s.knots[s.nk - 1]) return kSwInvalidArgument;
  const int D = s.D;
  for (int m = 0; m < multiplicity; m++) {
    const int span = sw_knot_span(s.knots, s.nk, knot);
    const int k0 = span - 1, k1 = span;
    const double a0 = (knot - s.knots[k0]) / (s.knots[k0 + 2] - s.knots[k0]);
    const double a1 = (knot - s.knots[k1]) / (s.knots[k1 + 2] - s.knots[k1]);
    // points span .. np-1 move up by one (points_.insert(begin + span, points_[span]))
    for (int i = s.np; i > span; i--)
      for (int d = 0; d < D; d++) s.pts[(size_t)i * D + d] = s.pts[(size_t)(i - 1) * D + d];
    // fresh points from the values before the shift (indices span-2 .. span are unmoved)
    for (int d = 0; d < D; d++) {
      const double f0 = a0 * s.pts[(size_t)k0 * D + d] + (1.0 - a0) * s.pts[(size_t)(k0 - 1) * D + d];
      const double f1 = a1 * s.pts[(size_t)k1 * D + d] + (1.0 - a1) * s.pts[(size_t)(k1 - 1) * D + d];
      s.pts[(size_t)(span - 1) * D + d] = f0;
      s.pts[(size_t)span * D + d] = f1;
    }
    s.np += 1;
    for (int i = s.nk; i > span + 1; i--) s.knots[i] = s.knots[i - 1];
    s.knots[span + 1] = knot;
    s.nk += 1;
  }
  return kSwOk;
}

// EditableBSpline::TruncateSplineAt
TPAMD_HD inline int sw_truncate(SwSpline &s, double u_end) {
  if (u_end >= s.umax) return kSwOk;
  if (u_end <= s.umin) {
    s.umin = INFINITY;
    s.umax = -INFINITY;
    s.nk = 0;
    s.np = 0;
    s.empty = true;
    return kSwOk;
  }
  const int st = sw_insert_knot(s, u_end, 3);
  if (st != kSwOk) return st;
  const int span = sw_knot_span(s.knots, s.nk, u_end);
  s.nk = span + 1;
  s.np = s.nk - 3;
  s.umax = u_end;
  return kSwOk;
}

// EditableBSpline::EvalCurve
TPAMD_HD inline int sw_eval(const SwSpline &s, double u, double *value) {
  if (s.empty || s.nk == 0 || u < s.umin || u > s.umax) return kSwOutOfRange;
  const int span = sw_knot_span(s.knots, s.nk, u);
  double N[3];
  sw_basis(s.knots, span, u, N);
  for (int d = 0; d < s.D; d++) value[d] = 0.0;
  for (int i = 0; i <= 2; i++) {
    const double *p = s.pts + (size_t)(span - 2 + i) * s.D;
    for (int d = 0; d < s.D; d++) value[d] += N[i] * p[d];
  }
  return kSwOk;
}

// ProjectPointOnPath (host/spline_edit.cc): waypoint index and line parameter of the closest
// segment point; projected point into `proj`
TPAMD_HD inline int sw_project(const double *wps, int W, int D, const double *point, int *index, double *line_parameter,
                               double *proj) {
  if (W <= 0) return kSwInvalidArgument;
  if (W == 1) {
    *index = 0;
    *line_parameter = 0.0;
    for (int d = 0; d < D; d++) proj[d] = wps[d];
    return kSwOk;
  }
  double best = DBL_MAX, best_t = 0.0;
  int best_i = 0;
  for (int i = 0; i + 1 < W; i++) {
    const double *a = wps + (size_t)i * D, *b = a + D;
    double ab2 = 0.0, ap_ab = 0.0;
    for (int d = 0; d < D; d++) {
      ab2 += (b[d] - a[d]) * (b[d] - a[d]);
      ap_ab += (point[d] - a[d]) * (b[d] - a[d]);
    }
    double t = ab2 > 0.0 ? ap_ab / ab2 : 0.0;
    if (t > 1.0) t = 1.0;
    const double tc = t < 0.0 ? 0.0 : t;
    double dd = 0.0;
    for (int d = 0; d < D; d++) {
      const double c = a[d] + tc * (b[d] - a[d]);
      dd += (c - point[d]) * (c - point[d]);
    }
    dd = sqrt(dd);
    if (dd < best) { best = dd; best_t = t; best_i = i; }
  }
  *index = best_i;
  *line_parameter = best_t;
  const double *a = wps + (size_t)best_i * D, *b = a + D;
  for (int d = 0; d < D; d++) proj[d] = a[d] + best_t * (b[d] - a[d]);
  return kSwOk;
}

// CornerOffset (splines/spline_utils.cc:25-45) added to `from`: out = from + offset
TPAMD_HD inline void sw_corner(const double *from, const double *to, double radius, int D, double *out) {
  double sq = 0.0;
  for (int i = 0; i < D; i++) {
    const double delta = to[i] - from[i];
    sq += delta * delta;
  }
  const double norm = sqrt(sq);
  for (int i = 0; i < D; i++) {
    const double delta = to[i] - from[i];
    double offset = norm > 1e-6 ? delta / norm : 0.0;
    if (norm > 4.0 * radius) offset = offset * radius;
    else offset = offset * (1.0 / 4.0) * norm;
    out[i] = from[i] + offset;
  }
}

// PolyLineToControlPoints: W waypoints -> max(3W - 2, 4) control points into cp; returns the count
TPAMD_HD inline int sw_polyline(const double *wps, int W, int D, double radius, double *cp) {
  if (W == 1) {
    for (int k = 0; k < 4; k++)
      for (int d = 0; d < D; d++) cp[(size_t)k * D + d] = wps[d];
    return 4;
  }
  const int n = 3 * W - 2;
  for (int i = 0; i < W; i++)
    for (int d = 0; d < D; d++) cp[(size_t)3 * i * D + d] = wps[(size_t)i * D + d];
  for (int i = 1; i + 1 < W; i++) {
    const int k = 3 * i;
    sw_corner(cp + (size_t)k * D, cp + (size_t)(k + 3) * D, radius, D, cp + (size_t)(k + 1) * D);
    sw_corner(cp + (size_t)k * D, cp + (size_t)(k - 3) * D, radius, D, cp + (size_t)(k - 1) * D);
  }
  sw_corner(cp, cp + (size_t)3 * D, radius, D, cp + (size_t)D);
  sw_corner(cp + (size_t)(n - 1) * D, cp + (size_t)(n - 4) * D, radius, D, cp + (size_t)(n - 2) * D);
  return n;
}

// EditableBSpline::ExtendWithControlPoints for the m points already stored behind the spline's
// points (pts[np .. np + m)): knots and the moved end point
TPAMD_HD inline int sw_extend(SwSpline &s, int m) {
  const int num_knots = s.nk, num_points = s.np;
  const int new_num_points = num_points + m;
  const int added_knots = (m + 1 + 2 + 1) - 4;
  const int new_num_knots = num_knots + added_knots;
  if (num_knots < 6) return kSwFailedPrecondition;
  if (new_num_knots > s.knot_capacity || new_num_points > s.knot_capacity - 3) return kSwFailedPrecondition;
  if (m < 2) return kSwInternal;      // UnimplementedError
  double *k = s.knots;
  const double u_join = k[num_knots - 1];
  const double old_knot_range = k[num_knots - 1] - k[0];
  const int old_inner = num_knots - 4 - 1;
  const int new_inner = new_num_knots - 4 - 1;
  const double new_knot_range = (old_knot_range * new_inner) / old_inner;
  const int lin_start = num_knots - 2 - 1;
  const int lin_size = (new_num_knots - 2) - lin_start;
  for (int i = 0; i < lin_size; i++) {
    const double step = (lin_size > 1) ? (new_knot_range - old_knot_range) / (lin_size - 1) : 0.0;
    k[lin_start + i] = (i == lin_size - 1) ? new_knot_range : old_knot_range + i * step;
  }
  for (int i = 0; i <= 2; i++) k[new_num_knots - 2 - 1 + i] = k[0] + new_knot_range;
  s.nk = new_num_knots;
  s.umax = k[new_num_knots - 1];
  const int modified = num_points - 1;
  const int span = sw_knot_span(k, new_num_knots, u_join);
  double N[3];
  sw_basis(k, span, u_join, N);
  if (!(N[1] > 0)) return kSwFailedPrecondition;
  const int D = s.D;
  for (int d = 0; d < D; d++) {
    const double v = 1.0 / N[1] * (s.pts[(size_t)modified * D + d] - N[0] * s.pts[(size_t)(modified - 1) * D + d]);
    s.pts[(size_t)modified * D + d] = v;
  }
  s.np = new_num_points;
  return kSwOk;
}

// Points a switch can give a spline of P points and W new waypoints: P + 3 (the truncation's
// inserted knots) + 3 (W + 1) - 2 (the new control polygon, the projected point included).
TPAMD_HD inline int sw_points_bound(int P, int W) { return P + 3 + 3 * (W + 1) - 2; }

// TimeableJointSplinePath::SwitchToWaypointPath on knots [nk] / pts [np][D], edited in place.
// The arrays hold sw_points_bound(np, W) points (+3 knots); `work` holds (W + 1) * D + D doubles.
// On success *nk_out / *np_out are the new sizes; on failure the arrays' contents are undefined
// (the caller works on a copy).
TPAMD_HD inline int sw_switch_to_waypoint_path(double *knots, double *pts, int nk, int np, int D, double keep_path_until,
                                               const double *wps, int W, double radius, double *work, int *nk_out,
                                               int *np_out) {
  if (nk == 0) return kSwFailedPrecondition;             // "No path to switch from."
  SwSpline s;
  s.knots = knots; s.pts = pts; s.nk = nk; s.np = np; s.D = D; s.empty = false;
  // capacity of the reference's allocation (host mirror: max(2 K + 3 W + 8, 100))
  s.knot_capacity = 2 * nk + 3 * W + 8 > 100 ? 2 * nk + 3 * W + 8 : 100;
  // EditableBSpline::Init
  if (nk < 6) return kSwOutOfRange;
  if (nk > s.knot_capacity) return kSwOutOfRange;
  if (np != nk - 3) return kSwInvalidArgument;
  for (int i = 1; i < nk; i++)
    if (knots[i] < knots[i - 1]) return kSwInvalidArgument;
  s.umin = knots[0];
  s.umax = knots[nk - 1];
  int st = sw_truncate(s, keep_path_until);
  if (st != kSwOk) return st;
  double *switch_position = work;                // [D]
  double *new_wps = work + D;                    // [W + 1][D]
  st = sw_eval(s, keep_path_until, switch_position);
  if (st != kSwOk) return st;
  int index = 0;
  double line_parameter = 0.0;
  double *proj = new_wps;                        // the projected point is the first candidate row
  st = sw_project(wps, W, D, switch_position, &index, &line_parameter, proj);
  if (st != kSwOk) return st;
  double inf_norm = 0.0;
  for (int d = 0; d < D; d++) {
    const double e = fabs(switch_position[d] - proj[d]);
    inf_norm = inf_norm < e ? e : inf_norm;      // std::max(inf_norm, e)
  }
  int n = (inf_norm > 1e-3) ? 1 : 0;
  const int first_waypoint = line_parameter >= 0 ? index + 1 : index;
  for (int i = first_waypoint; i < W; i++, n++)
    for (int d = 0; d < D; d++) new_wps[(size_t)n * D + d] = wps[(size_t)i * D + d];
  if (n == 0) return kSwInvalidArgument;         // "No waypoints left after the switch position."
  const int m = sw_polyline(new_wps, n, D, radius, s.pts + (size_t)s.np * D);
  st = sw_extend(s, m);
  if (st != kSwOk) return st;
  *nk_out = s.nk;
  *np_out = s.np;
  return kSwOk;
}

// TrajectoryBuffer::GetVelocityAtTime (trajectory_buffer.cc:233-275): the bracket of tb_bracket
// (upper_bound over time [n]), then InterpolateLinear (lerp a + t (b - a), as lerp_ref in
// tpamd_kernels.h) between the bracket's velocities [n][D]; at the last sample: its velocity.
TPAMD_HD inline int sw_velocity_at_time(const double *time, const double *vel, int n, int D, double time_sec,
                                        double *out) {
  int l = 0, u = 0;
  const int st = tb_bracket(time, n, time_sec, &l, &u);   // "No samples." / out of range
  if (st != kRdOk) return st;
  tb_interpolate(vel, l, u, D, tb_fraction(time, l, u, time_sec), out);
  return kSwOk;
}

#if (defined(__HIPCC__) || defined(__HIP__)) && !defined(TPAMD_HD_ROUTINES_ONLY)
// ------------------------------------------------------------------ the switch kernel
struct SwitchParams {
  int Q, D, K, pcap, tcap;             // queries; joints; knot / point strides of the set (K = pcap + 3)
  int scr_points, scr_work;            // scratch per query: points (knots: + 3) and work doubles
  double radius;                       // PathOptions::rounding of the new control polygon
  const int *ids;                      // [Q] planner of query k
  const long long *time_ns;            // [Q] switch time
  const double *keep;                  // [Q] caller's stop parameters, or null: stop_in / stop_status
  const double *stop_in;               // [Q] fastest-stop parameters (tpamd_stop.h)
  const int *stop_status;              // [Q]
  const int *offsets;                  // [Q + 1] waypoint rows of query k: offsets[k] .. offsets[k + 1)
  const double *wps;                   // [rows][D]
  // planner state
  double *knots, *cps, *iv;            // [B][K], [B][pcap][D], [B][D]
  int *np, *path_state;                // [B]
  const int *has_path, *initial_plan, *t_first, *t_count;
  const double *t_time, *t_qd;         // [B][tcap], [B][tcap][D]
  // scratch and results
  double *scr;                         // [Q][scr_points + 3 + scr_points * D + scr_work]
  double *stop_out;                    // [Q]
  int *np_out, *status_out;            // [Q]
};

// One thread per listed planner: stop parameter (given or from the stop kernel), velocity at the
// switch time, the spline edit in scratch, and the commit into the planner's slot on success.
static __global__ void __launch_bounds__(64) k_pset_switch(SwitchParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.Q) return;
  const int b = p.ids[k], D = p.D;
  const int P = p.np[b];
  double *sk = p.scr + (size_t)k * (p.scr_points + 3 + (size_t)p.scr_points * D + p.scr_work);
  double *sp = sk + p.scr_points + 3;
  double *vel = sp + (size_t)p.scr_points * D;          // [D], then the edit's work area
  double *work = vel + D;
  int st = kSwOk;
  double stop = 0.0;
  if (p.keep) {
    stop = p.keep[k];
  } else {
    stop = p.stop_in[k];
    st = p.stop_status[k];
  }
  // TrajectoryBuffer::GetVelocityAtTime on the resident trajectory
  if (st == kSwOk) {
    if (!p.initial_plan[b]) {
      st = kSwFailedPrecondition;
    } else {
      const size_t o = (size_t)b * p.tcap + p.t_first[b];
      st = sw_velocity_at_time(p.t_time + o, p.t_qd + o * D, p.t_count[b], D, pset_time_to_sec(p.time_ns[k]), vel);
    }
  }
  int nk = 0, npts = P;
  if (st == kSwOk) {
    if (!p.has_path[b]) {
      st = kSwFailedPrecondition;
    } else {
      const double *kb = p.knots + (size_t)b * p.K, *cb = p.cps + (size_t)b * p.pcap * D;
      for (int i = 0; i < P + 3; i++) sk[i] = kb[i];
      for (int i = 0; i < P * D; i++) sp[i] = cb[i];
      const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0;
      st = sw_switch_to_waypoint_path(sk, sp, P + 3, P, D, stop, p.wps + (size_t)w0 * D, W, p.radius, work,
                                      &nk, &npts);
    }
  }
  if (st == kSwOk) {        // the commit
    double *kb = p.knots + (size_t)b * p.K, *cb = p.cps + (size_t)b * p.pcap * D;
    for (int i = 0; i < nk; i++) kb[i] = sk[i];
    for (int i = 0; i < npts * D; i++) cb[i] = sp[i];
    for (int d = 0; d < D; d++) p.iv[(size_t)b * D + d] = vel[d];
    p.np[b] = npts;
    p.path_state[b] = 2;    // kModifiedPath
  } else {
    npts = P;
  }
  p.stop_out[k] = stop;
  p.np_out[k] = npts;
  p.status_out[k] = st;
}
#endif

}  // namespace tpamd

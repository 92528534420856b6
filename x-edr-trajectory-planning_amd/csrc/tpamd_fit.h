// tpamd_fit.h -- giving planner-set planners new waypoint paths on the device
// (include/tpamd.h tpamd_planner_set_set_waypoints*): TimeableJointSplinePath::SetWaypoints /
// FitSplineToWaypoints (timeable_path_joint_spline.cc:199-206, :252-292 as the host mirror restates
// them: host/timeable_path_joint_spline.cc) for every listed planner:
//   1. an empty waypoint list is an error (InvalidArgument "Control point vector empty.");
//   2. PolyLineToControlPoints with the rounding radius (sw_polyline, tpamd_switch.h): W = 1 gives
//      four copies of the waypoint, otherwise P = 3 W - 2 points with rounded corners;
//   3. the uniform degree-2 knots [P + 3] by running accumulation (BSplineBase::MakeUniformKnotVector,
//      splines/bspline_base.cc:356-381, on [0, 1]);
//   4. every knot scaled by max(control-polygon length, 0.1), the length summed segment by segment
//      in the mirror's order, each segment's norm a sequential sum of squares.
// The mirror's dimension check has no counterpart here: the waypoints of the C-ABI are [rows][D]
// (PathTimingTrajectorySet::SetWaypointPaths checks each waypoint before it packs them).
//
// fit_waypoints compiles for the host as well (TPAMD_HD): tests/cpp/test_fit_waypoints.cc holds it
// bit-equal to the mirror and to the oracle's fit. The operations are the mirror's, in its order (the library
// is built with -ffp-contract=off; '/' and sqrt are correctly rounded on both sides).
// tests/switch_reference.py restates the fit from the reference's sources and checks what a fit
// means (waypoints on control points 0, 3, 6, ..., uniform knots, the last knot against the polygon
// length in high precision): tests/test_switch_reference_cpu.py holds fit_waypoints, the mirror,
// the oracle and that restatement bit-equal for every D = 1..16, tests/test_gpu_switch_all_dofs.py
// holds k_pset_set_waypoints to it at every D through both entries, and
// tests/cpp/test_set_waypoints.cc runs 260-planner sets at D = 3 and 7.
//
// k_pset_set_waypoints: one thread per listed planner fits into the planner's own slot and writes
// what tpamd_planner_set_upload_paths_ragged writes with path_state 1 (kNewPath): knots, control
// points, count, limits, delta, initial velocity, path_state and has_path. A planner with no
// waypoints keeps its state.
#pragma once

#include "tpamd_switch.h"       // TPAMD_HD, sw_polyline, kSw*

namespace tpamd {

// Control points of the fit of W >= 1 waypoints: PolyLineToControlPoints' count
TPAMD_HD inline int fit_points(int W) { return W == 1 ? 4 : 3 * W - 2; }

// FitSplineToWaypoints on waypoints [W][D]: control points into cp [fit_points(W)][D], knots into
// knots [fit_points(W) + 3]. Returns the number of control points, or 0 (nothing written) for W < 1.
TPAMD_HD inline int fit_waypoints(const double *wps, int W, int D, double rounding, double *knots, double *cp) {
  if (W < 1) return 0;                                  // "Control point vector empty."
  const int P = sw_polyline(wps, W, D, rounding, cp);
  const int nk = P + 2 + 1;                             // kSplineOrder + 1
  // MakeUniformKnotVector(P, 0.0, 1.0): knots[0..2] = 0, running sums, the last three = 1
  const double spacing = (1.0 / (nk - 2.0 * (2 + 1.0) + 1.0)) * (1.0 - 0.0);
  double u = 0.0;
  for (int i = 0; i <= 2; i++) knots[i] = 0.0;
  for (int i = 3; i < nk - 3; i++) {
    u = u + spacing;
    knots[i] = u;
  }
  for (int i = nk - 3; i < nk; i++) knots[i] = 1.0;
  // the control polygon's length
  double length = 0.0;
  for (int i = 0; i + 1 < P; i++) {
    const double *a = cp + (size_t)i * D, *b = a + D;
    double sq = 0.0;
    for (int d = 0; d < D; d++) {
      const double diff = b[d] - a[d];
      sq += diff * diff;
    }
    length += sqrt(sq);
  }
  const double weighted = length * 1.0 < 0.1 ? 0.1 : length * 1.0;    // std::max(length * 1.0, 0.1)
  for (int i = 0; i < nk; i++) knots[i] *= weighted;
  return P;
}

#if defined(__HIPCC__) || defined(__HIP__)
// ------------------------------------------------------------------ the set-waypoints kernel
struct FitParams {
  int Q, D, K, pcap;                   // listed planners; joints; knot / point strides of the set
  double rounding;                     // PathOptions::rounding of every listed planner
  const int *ids;                      // [Q] planner of listed entry k (distinct)
  const int *offsets;                  // [Q + 1] waypoint rows of entry k: offsets[k] .. offsets[k + 1)
  const double *wps;                   // [rows][D]
  const double *vmax, *amax;           // [Q][D]
  const double *delta;                 // [Q]
  const double *iv;                    // [Q][D], or null: zero
  // planner state
  double *knots, *cps;                 // [B][K], [B][pcap][D]
  double *s_vmax, *s_amax, *s_delta, *s_iv;
  int *np, *path_state, *has_path;     // [B]
  // results
  int *np_out;                         // [Q] or null: control points after the call (0: no path)
  int *status_out;                     // [Q] TPAMD_PLAN_*
};

// Enqueues k_pset_set_waypoints on `st`, one thread per listed planner. The kernel lives in a
// translation unit of its own (tpamd_fit.hip), so that the switch kernel, which shares
// sw_polyline, keeps its code.
void launch_set_waypoints(const FitParams &p, hipStream_t st);
#endif

}  // namespace tpamd

// tpamd_joint_fit.h -- waypoint batches (include/tpamd.h tpamd_fit_joint_waypoints_*,
// tpamd_time_waypoint_paths_*): TimeableJointSplinePath::SetWaypoints / FitSplineToWaypoints
// (timeable_path_joint_spline.cc:200-207, :252-292) for every path of a batch, so that a batch of
// waypoint lists is timed without a host fit, without knowing the paths' lengths beforehand and
// without a group per control-point count.
//
// The fit itself is fit_waypoints (tpamd_fit.h), unchanged: its operations in its order. What this
// header adds is where path k's spline goes and what else is known once the fit has run:
//   - packed: path k's control points start at point_offsets[k], its knots at knot_offsets[k]
//     (path k behind path k - 1, a path without waypoints takes no slots), as
//     tpamd_fit_pose_waypoints_* and tpamd_planner_set_upload_paths_ragged pack splines;
//   - strided: path k's knots start at k * (p_stride + 3), its points at k * p_stride * D, which is
//     what the sampling/LP kernel reads when Workspace::np is set (sample_lp_joint_body);
//   - num_points[k] = max(3 W - 2, 4) and path_end[k] = the last knot (both 0 without waypoints);
//   - delta[k]: the caller's, or path_end[k] / (n_k - 1) -- ONE division, "n_k samples cover the
//     whole path" (path_timing_trajectory.cc:340-341 read backwards: s_end = 0 + delta (n_k - 1));
//   - samples[k]: n_k, or 0 for a path without waypoints. With that count every later launch of the
//     solve leaves the path alone (no block of the sampling/LP kernel has a sample of it, the
//     boundary kernels and the epilogue see no sample), and k_skip_empty_paths, which runs behind
//     the set-up kernel, marks it as taking no part (kErrSkip), so the sweep writes nothing either.
//
// joint_fit_path compiles for the host as well (TPAMD_HD): tests/cpp/test_joint_fit_layout.cc runs
// it for ragged batches in both layouts (also under the address and undefined-behaviour sanitizers)
// and tests/test_waypoint_batch_cpu.py holds it bit-equal to the oracle's fit.
#pragma once

#include <stdint.h>

#include "tpamd_fit.h"          // fit_waypoints, fit_points, kSw*

namespace tpamd {

struct JointFitParams {
  int Q, D;                            // paths; joints
  const int32_t *offsets;              // [Q + 1] waypoint rows of path k: offsets[k] .. offsets[k + 1)
  const double *wps;                   // [rows][D]
  const double *rounding;              // [Q], or null: 0.2 (PathOptions::rounding's default)
  // layout of the splines: packed (both offset arrays set) or strided (both null)
  const int32_t *point_offsets;        // [Q] first control point of path k
  const int32_t *knot_offsets;         // [Q] first knot of path k
  int p_stride;                        // strided: control points per slot (>= the largest P)
  double *knots, *cps;
  // per path, each may be null
  int32_t *num_points;                 // [Q]
  double *path_end;                    // [Q]
  int32_t *status;                     // [Q]: status_empty for a path without waypoints; 0 for the
  int status_empty;                    //      others if status_all (the timing entry leaves those to
  int status_all;                      //      the sweep)
  // the timing entry
  int N;                               // samples of a path when `samples_in` is null
  const int32_t *samples_in;           // [Q] or null
  const double *delta_in;              // [Q] or null: the whole path
  double *delta;                       // [Q] or null
  int32_t *samples;                    // [Q] or null
  double *zero;                        // [Q] or null: set to 0 (path_start, and the start values a caller leaves out)
};

// Path k of the batch. Returns its number of control points (0: no waypoints, no spline written).
TPAMD_HD inline int joint_fit_path(const JointFitParams &p, int k) {
  const int D = p.D;
  const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0;
  const int n = p.samples_in ? p.samples_in[k] : p.N;
  int P = 0;
  double end = 0.0;
  if (W >= 1) {
    double *knots = p.point_offsets ? p.knots + (size_t)p.knot_offsets[k] : p.knots + (size_t)k * (p.p_stride + 3);
    double *cp = p.point_offsets ? p.cps + (size_t)p.point_offsets[k] * D : p.cps + (size_t)k * p.p_stride * D;
    P = fit_waypoints(p.wps + (size_t)w0 * D, W, D, p.rounding ? p.rounding[k] : 0.2, knots, cp);
    end = knots[P + 2];
  }
  if (p.num_points) p.num_points[k] = P;
  if (p.path_end) p.path_end[k] = end;
  if (p.status) {
    if (W < 1) p.status[k] = p.status_empty;      // "Control point vector empty."
    else if (p.status_all) p.status[k] = kSwOk;
  }
  if (p.delta) p.delta[k] = p.delta_in ? p.delta_in[k] : end / (double)(n - 1);
  if (p.samples) p.samples[k] = W < 1 ? 0 : n;
  if (p.zero) p.zero[k] = 0.0;
  return P;
}

#if defined(__HIPCC__) || defined(__HIP__)
// Enqueues k_fit_joint_waypoints on `st`, one thread per path. The kernel lives in a translation
// unit of its own (tpamd_joint_fit.hip), so that every other kernel keeps its code.
void launch_fit_joint_waypoints(const JointFitParams &p, hipStream_t st);
// Enqueues k_skip_empty_paths on `st`: err_bits[k] |= kErrSkip where num_points[k] == 0. Runs
// behind the set-up kernel, which writes err_bits.
void launch_skip_empty_paths(int Q, const int32_t *num_points, uint32_t *err_bits, hipStream_t st);
#endif

}  // namespace tpamd

// tpamd_retarget.h -- path_tools.{h,cc} on the device, and the retarget of moving planner-set
// planners (include/tpamd.h tpamd_compute_stopping_points_*, tpamd_project_points_on_paths_*,
// tpamd_planner_set_retarget*):
//   rt_stopping_point      ComputeStoppingPoint (path_tools.cc:25-74): where a robot at `pos` with
//                          `vel` comes to rest on the straight line along `vel` within `acc`,
//                          shifted by the corner rounding (CornerOffset, spline_utils.cc:25-45);
//   rt_project             ProjectPointOnPath (path_tools.h:56-100): sw_project plus the distance;
//   k_stopping_points,
//   k_project_points       one thread per row / per waypoint list;
//   k_pset_retarget        for every listed planner, on its resident state: position and velocity
//                          at the retarget time (TrajectoryBuffer::GetPositionAtTime /
//                          GetVelocityAtTime), the stopping point, the waypoint list
//                          [position, stopping point, new waypoints...] (a planner at rest: without
//                          the stopping point), FitSplineToWaypoints into the planner's slot and the
//                          commit of k_pset_set_waypoints with the velocity as initial velocity.
//                          Readout and stopping point run before anything is written: a planner
//                          that fails one of them keeps its state bit for bit.
//
// The routines compile for the host as well (TPAMD_HD): tests/cpp/test_path_tools.cc runs them on
// the CPU against the mirror (host/path_tools.cc). They repeat the mirror's arithmetic operation by
// operation (sums in index order, no contraction: the library is built with -ffp-contract=off; '/'
// and sqrt are correctly rounded on both sides), so the results are bit-identical. One thread per
// item: the work is ordered O(W D) control flow, as in the switch and fit kernels.
#pragma once

#include "tpamd_fit.h"          // fit_waypoints, sw_project, tb_bracket, kSw*

namespace tpamd {

// ComputeStoppingPoint on pos / vel / acc [D] with the corner rounding radius `rounding`; the point
// into out [D] (out may be pos). kSwInvalidArgument ("Acceleration limits must be strictly
// positive.", nothing written) if the smallest limit is <= 0. *at_rest (may be null) is set when
// every |vel[i]| is below 100 epsilon: out is then pos.
//   dec   = ScaleDownToLimits(-vel / |vel| * max acc, acc): eigenmath::ScaleDownToLimits restated as
//           the uniform scaling by min(1, min over {i : |dec_i| > acc_i} of acc_i / |dec_i|)
//   t     = -(vel . vel) / (vel . dec)
//   delta = t (vel + 0.5 t dec)
//   out   = pos + delta + CornerOffset(delta, rounding)
// dec and delta are recomputed where they are used instead of stored: the same operations on the
// same operands give the same doubles, and a thread needs no [D] arrays.
TPAMD_HD inline int rt_stopping_point(const double *pos, const double *vel, const double *acc, double rounding, int D,
                                      double *out, int *at_rest = nullptr) {
  double amin = acc[0], amax = acc[0], vabs = 0.0;
  for (int i = 0; i < D; i++) {
    amin = acc[i] < amin ? acc[i] : amin;
    amax = acc[i] > amax ? acc[i] : amax;
    const double a = fabs(vel[i]);
    vabs = a > vabs ? a : vabs;
  }
  if (at_rest) *at_rest = 0;
  if (amin <= 0.0) return kSwInvalidArgument;
  if (vabs < DBL_EPSILON * 100) {
    if (at_rest) *at_rest = 1;
    for (int i = 0; i < D; i++) out[i] = pos[i];
    return kSwOk;
  }
  double sq = 0.0;
  for (int i = 0; i < D; i++) sq += vel[i] * vel[i];
  const double norm = sqrt(sq);
  double factor = 1.0;
  for (int i = 0; i < D; i++) {
    const double d = fabs(-(vel[i] / norm) * amax);
    if (d > acc[i]) {
      const double f = acc[i] / d;
      factor = f < factor ? f : factor;
    }
  }
  double vd = 0.0;
  for (int i = 0; i < D; i++) vd += vel[i] * (-(vel[i] / norm) * amax * factor);
  const double stop_time = -sq / vd;
  double dsq = 0.0;
  for (int i = 0; i < D; i++) {
    const double delta = stop_time * (vel[i] + 0.5 * stop_time * (-(vel[i] / norm) * amax * factor));
    dsq += delta * delta;
  }
  const double dnorm = sqrt(dsq);
  for (int i = 0; i < D; i++) {
    const double delta = stop_time * (vel[i] + 0.5 * stop_time * (-(vel[i] / norm) * amax * factor));
    // CornerOffset(delta, rounding): sw_corner with a zero `from`
    double offset = dnorm > 1e-6 ? delta / dnorm : 0.0;
    if (dnorm > 4.0 * rounding) offset = offset * rounding;
    else offset = offset * (1.0 / 4.0) * dnorm;
    out[i] = pos[i] + delta + offset;
  }
  return kSwOk;
}

// ProjectPointOnPath with every field of ProjectedPointResult: sw_project (which the switch uses
// unchanged), then the distance of the winning segment's clamped point, summed as sw_project sums it.
TPAMD_HD inline int rt_project(const double *wps, int W, int D, const double *point, int *index, double *line_parameter,
                               double *distance, double *proj) {
  const int st = sw_project(wps, W, D, point, index, line_parameter, proj);
  if (st != kSwOk) return st;
  const double *a = wps + (size_t)*index * D;
  const double t = *line_parameter, tc = t < 0.0 ? 0.0 : t;
  double dd = 0.0;
  for (int d = 0; d < D; d++) {
    const double c = W == 1 ? a[d] : a[d] + tc * (a[D + d] - a[d]);
    dd += (c - point[d]) * (c - point[d]);
  }
  *distance = sqrt(dd);
  return kSwOk;
}

#if defined(__HIPCC__) || defined(__HIP__)
// ------------------------------------------------------------------ the batch kernels
struct StoppingPointParams {
  int count, D;
  const double *position, *velocity, *acceleration_limit;   // [count][D]
  const double *corner_rounding;                            // [count]
  double *point;                                            // [count][D]
  int *status;                                              // [count]
};

struct ProjectParams {
  int count, D;
  const int *offsets;                  // [count + 1] waypoint rows of list k: offsets[k] .. offsets[k + 1)
  const double *wps;                   // [rows][D]
  const double *point;                 // [count][D]
  int *waypoint_index;                 // [count]
  double *distance, *line_parameter;   // [count]
  double *projected;                   // [count][D]
  int *status;                         // [count]
};

// ------------------------------------------------------------------ the retarget kernel
struct RetargetParams {
  int Q, D, K, pcap, tcap;             // listed planners; joints; knot / point / trajectory strides
  double rounding;                     // PathOptions::rounding of the new paths and of the stopping points
  const int *ids;                      // [Q] planner of listed entry k (distinct)
  const long long *time_ns;            // [Q] retarget time
  const int *offsets;                  // [Q + 1] waypoint rows of entry k: offsets[k] .. offsets[k + 1)
  const double *wps;                   // [rows][D]
  const double *vmax, *amax;           // [Q][D]
  const double *delta;                 // [Q]
  const double *stop_acc;              // [Q][D], or null: amax
  // planner state
  double *knots, *cps;                 // [B][K], [B][pcap][D]
  double *s_vmax, *s_amax, *s_delta, *s_iv;
  int *np, *path_state, *has_path;     // [B]
  const int *initial_plan, *t_first, *t_count;
  const double *t_time, *t_q, *t_qd;   // [B][tcap], [B][tcap][D]
  // scratch: entry k's waypoint list and velocity, (W_k + 3) D doubles from (offsets[k] + 3 k) D
  double *scr;
  // results
  int *np_out, *status_out;            // [Q]
  double *pos_out, *vel_out, *stop_out;   // [Q][D], any may be null
};

// Enqueue the kernels on `st`, one thread per item (tpamd_retarget.hip).
void launch_stopping_points(const StoppingPointParams &p, hipStream_t st);
void launch_project_points(const ProjectParams &p, hipStream_t st);
void launch_pset_retarget(const RetargetParams &p, hipStream_t st);
#endif

}  // namespace tpamd

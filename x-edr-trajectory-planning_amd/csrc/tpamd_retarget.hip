// tpamd_retarget.hip -- the kernels of tpamd_retarget.h in a translation unit of their own.
#include <hip/hip_runtime.h>

#define TPAMD_HD_ROUTINES_ONLY     // the edit, fit and readout routines, not the switch and readout kernels
#include "tpamd_retarget.h"

namespace tpamd {

// One thread per row: ComputeStoppingPoint. A row with a non-positive limit keeps its point.
static __global__ void __launch_bounds__(64) k_stopping_points(StoppingPointParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const size_t o = (size_t)k * p.D;
  p.status[k] = rt_stopping_point(p.position + o, p.velocity + o, p.acceleration_limit + o, p.corner_rounding[k], p.D,
                                  p.point + o);
}

// One thread per waypoint list: ProjectPointOnPath. An empty list ("No waypoints.") keeps its outputs.
static __global__ void __launch_bounds__(64) k_project_points(ProjectParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0, D = p.D;
  int index = 0;
  double t = 0.0, dist = 0.0;
  const int st = rt_project(p.wps + (size_t)w0 * D, W, D, p.point + (size_t)k * D, &index, &t, &dist,
                            p.projected + (size_t)k * D);
  p.status[k] = st;
  if (st != kSwOk) return;
  p.waypoint_index[k] = index;
  p.distance[k] = dist;
  p.line_parameter[k] = t;
}

// One thread per listed planner: the readout and the stopping point into scratch, then the fit
// straight into the planner's slot (it cannot fail: the list holds the position at least) and what
// k_pset_set_waypoints commits, with the velocity read out as the initial velocity.
static __global__ void __launch_bounds__(64) k_pset_retarget(RetargetParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.Q) return;
  const int b = p.ids[k], D = p.D;
  const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0;
  double *list = p.scr + ((size_t)w0 + 3 * (size_t)k) * D;       // [W + 2][D]: q, stop, the new waypoints
  double *vel = list + (size_t)(W + 2) * D;                      // [D]
  double *q = list, *stop = list + D;
  // TrajectoryBuffer::GetPositionAtTime / GetVelocityAtTime on the resident trajectory
  int st = kSwOk, at_rest = 0;
  if (!p.initial_plan[b]) {
    st = kSwFailedPrecondition;
  } else {
    const size_t o = (size_t)b * p.tcap + p.t_first[b];
    const double *tm = p.t_time + o;
    const double time_sec = (double)p.time_ns[k] / 1e9;          // TimeToSec
    int l = 0, u = 0;
    st = tb_bracket(tm, p.t_count[b], time_sec, &l, &u);
    if (st == kRdOk) {
      const double at = tb_fraction(tm, l, u, time_sec);
      tb_interpolate(p.t_q + o * D, l, u, D, at, q);
      tb_interpolate(p.t_qd + o * D, l, u, D, at, vel);
    }
  }
  if (st == kSwOk)
    st = rt_stopping_point(q, vel, (p.stop_acc ? p.stop_acc : p.amax) + (size_t)k * D, p.rounding, D, stop, &at_rest);
  p.status_out[k] = st;
  if (st != kSwOk) {       // the planner keeps its state
    p.np_out[k] = p.has_path[b] ? p.np[b] : 0;
    return;
  }
  for (int d = 0; d < D; d++) {
    const size_t i = (size_t)k * D + d;
    if (p.pos_out) p.pos_out[i] = q[d];
    if (p.vel_out) p.vel_out[i] = vel[d];
    if (p.stop_out) p.stop_out[i] = stop[d];
  }
  // a planner at rest gets no stopping waypoint: the user's waypoints follow the position
  double *user = at_rest ? stop : stop + D;
  for (int i = 0; i < W * D; i++) user[i] = p.wps[(size_t)w0 * D + i];
  const int n = W + (at_rest ? 1 : 2);
  const int P = fit_waypoints(list, n, D, p.rounding, p.knots + (size_t)b * p.K, p.cps + (size_t)b * p.pcap * D);
  for (int d = 0; d < D; d++) {
    const size_t i = (size_t)k * D + d, o = (size_t)b * D + d;
    p.s_vmax[o] = p.vmax[i];
    p.s_amax[o] = p.amax[i];
    p.s_iv[o] = vel[d];
  }
  p.s_delta[b] = p.delta[k];
  p.np[b] = P;
  p.path_state[b] = 1;     // kNewPath
  p.has_path[b] = 1;
  p.np_out[k] = P;
}

void launch_stopping_points(const StoppingPointParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_stopping_points, dim3((unsigned)((p.count + 63) / 64)), dim3(64), 0, st, p);
}

void launch_project_points(const ProjectParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_project_points, dim3((unsigned)((p.count + 63) / 64)), dim3(64), 0, st, p);
}

void launch_pset_retarget(const RetargetParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_pset_retarget, dim3((unsigned)((p.Q + 63) / 64)), dim3(64), 0, st, p);
}

}  // namespace tpamd

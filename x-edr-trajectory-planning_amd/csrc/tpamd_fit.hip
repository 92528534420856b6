// tpamd_fit.hip -- the set-waypoints kernel of tpamd_fit.h in a translation unit of its own.
#include <hip/hip_runtime.h>

#define TPAMD_HD_ROUTINES_ONLY     // sw_polyline, not the switch and readout kernels
#include "tpamd_fit.h"

namespace tpamd {

// One thread per listed planner: the fit straight into the planner's slot (it cannot fail once
// W >= 1), then the limits, delta, initial velocity, count and state.
static __global__ void __launch_bounds__(64) k_pset_set_waypoints(FitParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.Q) return;
  const int b = p.ids[k], D = p.D;
  const int w0 = p.offsets[k], W = p.offsets[k + 1] - w0;
  if (W < 1) {             // "Control point vector empty.": the planner keeps its state
    if (p.np_out) p.np_out[k] = p.has_path[b] ? p.np[b] : 0;
    p.status_out[k] = kSwInvalidArgument;
    return;
  }
  const int P = fit_waypoints(p.wps + (size_t)w0 * D, W, D, p.rounding, p.knots + (size_t)b * p.K,
                              p.cps + (size_t)b * p.pcap * D);
  for (int d = 0; d < D; d++) {
    const size_t i = (size_t)k * D + d, o = (size_t)b * D + d;
    p.s_vmax[o] = p.vmax[i];
    p.s_amax[o] = p.amax[i];
    p.s_iv[o] = p.iv ? p.iv[i] : 0.0;
  }
  p.s_delta[b] = p.delta[k];
  p.np[b] = P;
  p.path_state[b] = 1;     // kNewPath
  p.has_path[b] = 1;
  if (p.np_out) p.np_out[k] = P;
  p.status_out[k] = kSwOk;
}

void launch_set_waypoints(const FitParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_pset_set_waypoints, dim3((unsigned)((p.Q + 63) / 64)), dim3(64), 0, st, p);
}

}  // namespace tpamd

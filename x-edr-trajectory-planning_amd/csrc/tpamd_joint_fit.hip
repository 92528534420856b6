// tpamd_joint_fit.hip -- the two kernels of tpamd_joint_fit.h in a translation unit of their own.
#include <hip/hip_runtime.h>

#include "tpamd_device.h"          // kErrSkip

#define TPAMD_HD_ROUTINES_ONLY     // sw_polyline, not the switch and readout kernels
#include "tpamd_joint_fit.h"

namespace tpamd {

// One thread per path (W is tens at most, the work O(W D)): the fit straight into the path's slot.
static __global__ void __launch_bounds__(64) k_fit_joint_waypoints(JointFitParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.Q) return;
  joint_fit_path(p, k);
}

static __global__ void __launch_bounds__(128) k_skip_empty_paths(int Q, const int32_t *num_points,
                                                                 uint32_t *err_bits) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= Q) return;
  if (num_points[k] == 0) err_bits[k] |= kErrSkip;
}

void launch_fit_joint_waypoints(const JointFitParams &p, hipStream_t st) {
  if (p.Q < 1) return;
  hipLaunchKernelGGL(k_fit_joint_waypoints, dim3((unsigned)((p.Q + 63) / 64)), dim3(64), 0, st, p);
}

void launch_skip_empty_paths(int Q, const int32_t *num_points, uint32_t *err_bits, hipStream_t st) {
  if (Q < 1) return;
  hipLaunchKernelGGL(k_skip_empty_paths, dim3((unsigned)((Q + 127) / 128)), dim3(128), 0, st, Q, num_points,
                     err_bits);
}

}  // namespace tpamd

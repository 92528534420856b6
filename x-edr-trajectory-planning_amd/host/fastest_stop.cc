#include "fastest_stop.h"

#include <algorithm>
#include <cmath>

#include "../../include/tpamd.h"

namespace trajectory_planning {

int ComputeFastestStop(int sample_count, int num_dofs, const double *time, const double *const *velocities,
                       const double *const *accelerations, const double *max_acceleration,
                       double *total_duration, FastestStopProfile *profile) {
  // Time scaling s(t) of the path: stop_acc = traj_vel(s) * 1/2 d(rate2)/ds + traj_acc(s) * rate2
  // with rate2 = (ds/dt)^2. rate2 starts at 1 and decreases as fast as the limits allow.
  double duration = 0.0;
  double rate_squared = 1.0;
  double diff_rate_squared = 0.0;
  const double first_time_point = time[0];
  int index = 0;
  for (; (index < sample_count - 1) && (rate_squared > 0.0); index++) {
    const double *vel = velocities[index];
    const double *acc = accelerations[index];
    double diff_rate_squared_min = 0.0;
    for (int dof = 0; dof < num_dofs; dof++) {
      if (std::fabs(vel[dof]) < 1e-6) continue;
      const double bias = acc[dof] * rate_squared;
      for (int sign = 0; sign < 2; sign++) {
        // the largest deceleration of this joint alone, against -a and +a
        const double candidate = sign == 0 ? 2.0 * (-bias - max_acceleration[dof]) / vel[dof]
                                           : 2.0 * (-bias + max_acceleration[dof]) / vel[dof];
        bool valid = true;
        for (int j = 0; j < num_dofs; j++) {
          const double a = acc[j] * rate_squared + (0.5 * vel[j]) * candidate;
          valid = valid && (max_acceleration[j] - a >= -1e-10) && (-max_acceleration[j] - a <= 1e-10);
        }
        if (valid && candidate < diff_rate_squared_min) diff_rate_squared_min = candidate;
      }
    }
    diff_rate_squared = std::min(diff_rate_squared_min, 0.0);
    if (profile) {
      profile->time.push_back(first_time_point + duration);
      profile->rate_squared.push_back(rate_squared);
      profile->diff_rate_squared.push_back(diff_rate_squared);
    }
    // forward Euler step of rate2 over the sample interval
    const double unscaled_dt = time[index + 1] - time[index];
    const double next_rate_squared = std::max(0.0, rate_squared + unscaled_dt * diff_rate_squared);
    duration += 2.0 * unscaled_dt / (std::sqrt(rate_squared) + std::sqrt(next_rate_squared));
    rate_squared = next_rate_squared;
  }
  if (profile) {
    profile->time.push_back(first_time_point + duration);
    profile->rate_squared.push_back(rate_squared);
    profile->diff_rate_squared.push_back(diff_rate_squared);
  }
  *total_duration = duration;
  return index;
}

int FastestStopAtTime(int count, int num_dofs, const double *time, const double *s, const double *qd,
                      const double *qdd, const double *max_acceleration, double query_time,
                      double *stop_parameter, int *stop_index, double *duration, FastestStopProfile *profile) {
  const int offset = (int)(std::lower_bound(time, time + std::max(count, 0), query_time) - time);
  if (offset >= count) {
    *stop_parameter = 0.0;
    *stop_index = -1;
    *duration = 0.0;
    return TPAMD_PLAN_INVALID_ARGUMENT;
  }
  const int n = count - offset;
  std::vector<const double *> vel(n), acc(n);
  for (int i = 0; i < n; i++) {
    vel[i] = qd + (size_t)(offset + i) * num_dofs;
    acc[i] = qdd + (size_t)(offset + i) * num_dofs;
  }
  const int k = ComputeFastestStop(n, num_dofs, time + offset, vel.data(), acc.data(), max_acceleration, duration,
                                   profile);
  *stop_index = offset + k;
  *stop_parameter = s[offset + k];
  return TPAMD_PLAN_OK;
}

}  // namespace trajectory_planning

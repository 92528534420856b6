// RescaleTrajectoryBackwardToStop (rescale_to_stop.cc), restated on the compat types.
#include "rescale_to_stop.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

namespace trajectory_planning {

::tpamd::compat::StatusOr<SampledTrajectory> RescaleTrajectoryBackwardToStop(
    const VectorXd &max_acceleration, Span<const double> times, Span<const VectorXd> positions,
    Span<const VectorXd> velocities, Span<const VectorXd> accelerations) {
  const Status valid = AreInputsValidForSampledTrajectory(times, positions, velocities, accelerations);
  if (!valid.ok()) return valid;

  // Already at rest: nothing to rescale.
  constexpr double kTiny = 1e-8;
  if (velocities[velocities.size() - 1].maxAbs() < kTiny) return SampledTrajectory{};

  const int joint_count = (int)max_acceleration.size();
  const int sample_count = (int)times.size();
  std::vector<double> rescaled_times{0.0};
  std::vector<VectorXd> rescaled_velocities{VectorXd(joint_count, 0.0)};
  std::vector<VectorXd> rescaled_accelerations{VectorXd(joint_count, 0.0)};

  // rate_squared = (d unscaled time / d time)^2, 0 at the stop; diff_rate_squared its derivative
  // over unscaled time. The scaled acceleration is 0.5 velocity diff_rate_squared +
  // acceleration rate_squared; every joint's bound, hit with either sign, gives one candidate
  // diff_rate_squared, and the smallest admissible one (<= 0) is taken.
  double rate_squared = 0.0;
  double diff_rate_squared = 0.0;
  VectorXd acceleration_bias(joint_count), scaled_acceleration(joint_count);
  for (int i = sample_count - 1; i > 1; --i) {
    const VectorXd &velocity = velocities[i];
    for (int j = 0; j < joint_count; ++j) acceleration_bias[j] = accelerations[i][j] * rate_squared;
    diff_rate_squared = 0.0;
    for (int joint = 0; joint < joint_count; ++joint) {
      if (std::abs(velocity[joint]) < kTiny) continue;
      for (const double sign : {-1.0, 1.0}) {
        const double diff_rate_squared_joint =
            -2.0 * (acceleration_bias[joint] + sign * max_acceleration[joint]) / velocity[joint];
        bool acceleration_valid = true;
        for (int j = 0; j < joint_count; ++j) {
          scaled_acceleration[j] = acceleration_bias[j] + 0.5 * velocity[j] * diff_rate_squared_joint;
          acceleration_valid = acceleration_valid && max_acceleration[j] - scaled_acceleration[j] >= -kTiny &&
                               -max_acceleration[j] - scaled_acceleration[j] <= kTiny;
        }
        if (acceleration_valid && diff_rate_squared_joint < diff_rate_squared)
          diff_rate_squared = diff_rate_squared_joint;
      }
    }
    const double unscaled_dt = times[i] - times[i - 1];
    const double next_rate_squared = rate_squared - diff_rate_squared * unscaled_dt;
    // clamped so that the integration does not overshoot the original speed
    const double clamped_rate_squared = std::min(next_rate_squared, 1.0);
    // trapezoidal rule
    const double new_time_delta = 2.0 * unscaled_dt / (std::sqrt(rate_squared) + std::sqrt(clamped_rate_squared));
    rescaled_times.push_back(rescaled_times.back() - new_time_delta);
    const double rate = std::sqrt(clamped_rate_squared);
    VectorXd v(joint_count), a(joint_count);
    for (int j = 0; j < joint_count; ++j) {
      v[j] = rate * velocity[j];
      a[j] = acceleration_bias[j] + 0.5 * velocity[j] * diff_rate_squared;
    }
    rescaled_velocities.push_back(v);
    rescaled_accelerations.push_back(a);
    if (next_rate_squared >= 1.0) break;
    rate_squared = next_rate_squared;
  }

  // Time runs forward with increasing index.
  std::reverse(rescaled_times.begin(), rescaled_times.end());
  std::reverse(rescaled_velocities.begin(), rescaled_velocities.end());
  std::reverse(rescaled_accelerations.begin(), rescaled_accelerations.end());

  // Line the segment up with the input: it starts at sample switch_index.
  const int switch_index = sample_count - (int)rescaled_times.size();
  if (switch_index < 0) std::abort();   // cannot happen: one row per sample at most
  const double time_offset = times[switch_index] - rescaled_times.front();
  for (double &time : rescaled_times) time += time_offset;

  SampledTrajectory out;
  out.times = std::move(rescaled_times);
  out.positions.assign(positions.begin() + switch_index, positions.begin() + switch_index + out.times.size());
  out.velocities = std::move(rescaled_velocities);
  out.accelerations = std::move(rescaled_accelerations);
  return out;
}

}  // namespace trajectory_planning

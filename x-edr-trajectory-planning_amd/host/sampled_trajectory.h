// Host mirror of trajectory_planning/sampled_trajectory.h: a trajectory given by samples, and the
// validity test the stop rescaling applies to its inputs (sampled_trajectory.cc).
#ifndef TPAMD_HOST_SAMPLED_TRAJECTORY_H_
#define TPAMD_HOST_SAMPLED_TRAJECTORY_H_

#include <vector>

#include "compat.h"

namespace trajectory_planning {

using ::tpamd::compat::Span;
using ::tpamd::compat::Status;
using ::tpamd::compat::VectorXd;

struct SampledTrajectory {
  std::vector<double> times;
  std::vector<VectorXd> positions;
  std::vector<VectorXd> velocities;
  std::vector<VectorXd> accelerations;
};

// At least two samples, one of each kind per time, and strictly increasing times.
inline Status AreInputsValidForSampledTrajectory(Span<const double> times, Span<const VectorXd> positions,
                                                 Span<const VectorXd> velocities,
                                                 Span<const VectorXd> accelerations) {
  const size_t sample_count = times.size();
  if (sample_count < 2) return ::tpamd::compat::InvalidArgumentError("Need at least two samples.");
  if (positions.size() != sample_count || velocities.size() != sample_count ||
      accelerations.size() != sample_count)
    return ::tpamd::compat::InvalidArgumentError("inconsistent sizes for samples.");
  for (size_t i = 0; i + 1 < sample_count; ++i)
    if (times[i + 1] <= times[i])
      return ::tpamd::compat::InvalidArgumentError("Time samples not strictly increasing.");
  return ::tpamd::compat::OkStatus();
}

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_SAMPLED_TRAJECTORY_H_

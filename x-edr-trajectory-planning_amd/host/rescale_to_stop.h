// Host mirror of trajectory_planning/rescale_to_stop.h: the time scaling that brings a sampled
// trajectory to rest at its last sample along the same positions.
#ifndef TPAMD_HOST_RESCALE_TO_STOP_H_
#define TPAMD_HOST_RESCALE_TO_STOP_H_

#include "compat.h"
#include "sampled_trajectory.h"

namespace trajectory_planning {

// Integrates the squared time-scaling rate backward from the last sample (rate 0: at rest) along
// the steepest change that keeps every scaled joint acceleration within +-max_acceleration, until
// the rate reaches 1 (the original speed) or sample 2. Returns the stopping segment: it ends at the
// last sample's position at rest, its positions are the input's, and its times are shifted so that
// it starts at the time of the input sample it starts on. An empty trajectory if the input already
// ends at rest (|velocities.back()| < 1e-8); the input's validity status if it is not valid.
// Operations are in the reference's order (the device kernel, csrc/tpamd_rescale.h, matches this
// bit for bit; the library is built with -ffp-contract=off).
::tpamd::compat::StatusOr<SampledTrajectory> RescaleTrajectoryBackwardToStop(
    const VectorXd &max_acceleration, Span<const double> times, Span<const VectorXd> positions,
    Span<const VectorXd> velocities, Span<const VectorXd> accelerations);

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_RESCALE_TO_STOP_H_

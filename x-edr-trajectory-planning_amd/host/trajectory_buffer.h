// Host mirror of trajectory_planning/trajectory_buffer.h: the samples and the sequence number,
// InsertSegment / AppendSample, DiscardSegmentBefore, the interpolating getters,
// GetPositionsUpToTime, AddOffsetToTimestamps, and StopAtIndex / StopBeforeTime
// (trajectory_buffer.cc:296-385), which cut the trajectory and time-scale its tail to rest with
// RescaleTrajectoryBackwardToStop. The planner set's tpamd_planner_set_stop_trajectories and the
// batch tpamd_stop_trajectories_* compute the same stop on the device, bit for bit; a buffer set
// (tpamd_buffer_set_*, host/trajectory_buffer_set.h) keeps B such buffers on the device.
//
// One deliberate deviation: a StopAtIndex whose sample is already at rest (|v| < 1e-8) before the
// last sample makes the rescaling return nothing, and the reference then aborts
// (CHECK(!rescaled_stop.times.empty())). Here it returns InternalError and leaves the buffer
// unchanged. So does a StopAtIndex whose sample has no admissible deceleration (its joints at or
// above the 1e-8 cut all ask too much of another joint): the first rescaled time step is 2 dt / 0,
// and the reference inserts a segment with NaN times.
#ifndef TPAMD_HOST_TRAJECTORY_BUFFER_H_
#define TPAMD_HOST_TRAJECTORY_BUFFER_H_

#include <memory>
#include <vector>

#include "compat.h"
#include "sampled_trajectory.h"

namespace trajectory_planning {

using ::tpamd::compat::Time;

struct TrajectoryBufferOptions {
  // Time stamps closer than this are treated as equal.
  double timestep_tolerance = 1e-6;
};

class TrajectoryBuffer {
 public:
  static ::tpamd::compat::StatusOr<std::shared_ptr<TrajectoryBuffer>> Create(
      TrajectoryBufferOptions options = TrajectoryBufferOptions{});
  // Empties the buffer; the sequence number goes back to 0.
  void Clear();
  void Reserve(size_t size);
  // Time of the first sample (TimeFromSec); TimeFromSec(0) without samples.
  Time GetStartTime() const;
  // Time of the last sample; Time() without samples.
  Time GetEndTime() const;
  // InsertSegment calls since the buffer was last replaced as a whole (or cleared).
  int GetSequenceNumber() const { return sequence_number_; }
  size_t GetNumSamples() const { return positions_.size(); }
  Span<const double> GetTimes() const { return Span<const double>(times_.data(), times_.size()); }
  Span<const VectorXd> GetPositions() const { return Span<const VectorXd>(positions_.data(), positions_.size()); }
  Span<const VectorXd> GetVelocities() const { return Span<const VectorXd>(velocities_.data(), velocities_.size()); }
  Span<const VectorXd> GetAccelerations() const {
    return Span<const VectorXd>(accelerations_.data(), accelerations_.size());
  }

  // Replaces the samples from times.front() on (the sample within timestep_tolerance before it
  // included) with the segment; a segment that starts before the buffer replaces all of it.
  // The sequence number goes up by one (an empty segment included), and back to 0 when the
  // segment replaces the whole buffer.
  Status InsertSegment(Span<const double> times, Span<const VectorXd> positions, Span<const VectorXd> velocities,
                       Span<const VectorXd> accelerations);

  // One sample behind the last; InvalidArgument unless time is after the last sample's.
  Status AppendSample(double time, const VectorXd &positions, const VectorXd &velocities,
                      const VectorXd &accelerations);

  // Drops the samples before the time: nothing at or before the first sample, everything (Clear)
  // after the last. A time that is more than timestep_tolerance before the next sample makes the
  // sample before it the new first one, overwritten with the state interpolated at the time; a
  // sample within timestep_tolerance before the time is kept as it is.
  void DiscardSegmentBefore(Time time);
  void DiscardSegmentBefore(double time_sec);

  // The positions before the bracket of `time` (upper_bound - 1 of them); none for a time outside
  // the samples.
  Span<const VectorXd> GetPositionsUpToTime(Time time) const;

  // Cuts the trajectory after sample `index` and time-scales samples up to it so that it ends at
  // rest at sample index's position without exceeding max_acceleration. OutOfRange for index
  // outside [1, GetNumSamples() - 1]; InvalidArgument for max_acceleration.minCoeff() <= 0,
  // time_step <= 0 or times not strictly increasing up to index; NotFound if the stop needs every
  // sample and still does not match the original velocity (1e-2). On the last sample with
  // |v| < 1e-4 only its velocity and acceleration are zeroed. time_step is checked, not used
  // (as in the reference). On failure the buffer is unchanged.
  Status StopAtIndex(int index, const VectorXd &max_acceleration, double time_step);
  // StopAtIndex(min(lower_bound(time) + 1, GetNumSamples() - 1)); OK without samples, OutOfRange
  // before the first sample.
  Status StopBeforeTime(Time time, const VectorXd &max_acceleration, double time_step);
  Status StopBeforeTime(double time_sec, const VectorXd &max_acceleration, double time_step);

  // Linear interpolation between the samples bracketing the time (upper_bound); on the last
  // sample that sample. FailedPrecondition without samples, OutOfRange outside them.
  ::tpamd::compat::StatusOr<VectorXd> GetPositionAtTime(Time time) const;
  ::tpamd::compat::StatusOr<VectorXd> GetPositionAtTime(double time_sec) const;
  ::tpamd::compat::StatusOr<VectorXd> GetVelocityAtTime(Time time) const;
  ::tpamd::compat::StatusOr<VectorXd> GetVelocityAtTime(double time_sec) const;
  ::tpamd::compat::StatusOr<VectorXd> GetAccelerationAtTime(Time time) const;
  ::tpamd::compat::StatusOr<VectorXd> GetAccelerationAtTime(double time_sec) const;

  // Adds the offset (a duration as offset / Seconds(1)) to every time stamp.
  void AddOffsetToTimestamps(::tpamd::compat::Duration offset);
  void AddOffsetToTimestamps(double offset);

 private:
  explicit TrajectoryBuffer(TrajectoryBufferOptions options) : options_(options) {}
  ::tpamd::compat::StatusOr<VectorXd> ValueAtTime(const std::vector<VectorXd> &values, double time_sec) const;

  TrajectoryBufferOptions options_;
  int sequence_number_ = 0;
  std::vector<double> times_;
  std::vector<VectorXd> positions_, velocities_, accelerations_;
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_TRAJECTORY_BUFFER_H_

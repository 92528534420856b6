// TrajectoryBuffer (trajectory_buffer.cc) restated on the compat types. Quirks of the reference are kept on purpose: InsertSegment's upper_bound with a <= b and
// its step back by one within the tolerance, and StopAtIndex validating time_step without using it.
#include "trajectory_buffer.h"

#include <algorithm>
#include <cmath>
#include <string>

#include "rescale_to_stop.h"

namespace trajectory_planning {

using ::tpamd::compat::StatusOr;

StatusOr<std::shared_ptr<TrajectoryBuffer>> TrajectoryBuffer::Create(TrajectoryBufferOptions options) {
  if (!(options.timestep_tolerance > 0))
    return ::tpamd::compat::FailedPreconditionError("timestep_tolerance (" +
                                                    std::to_string(options.timestep_tolerance) + ") not positive");
  return std::shared_ptr<TrajectoryBuffer>(new TrajectoryBuffer(options));
}

static double TimeToSec(Time time) { return (double)::tpamd::compat::ToUnixNanos(time) / 1e9; }
static Time TimeFromSec(double seconds) { return ::tpamd::compat::FromUnixSeconds(seconds); }

Time TrajectoryBuffer::GetStartTime() const { return TimeFromSec(times_.empty() ? 0.0 : times_.front()); }

Time TrajectoryBuffer::GetEndTime() const { return times_.empty() ? Time() : TimeFromSec(times_.back()); }

void TrajectoryBuffer::Reserve(size_t size) {
  times_.reserve(size);
  positions_.reserve(size);
  velocities_.reserve(size);
  accelerations_.reserve(size);
}

void TrajectoryBuffer::Clear() {
  sequence_number_ = 0;
  times_.clear();
  positions_.clear();
  velocities_.clear();
  accelerations_.clear();
}

Status TrajectoryBuffer::InsertSegment(Span<const double> times, Span<const VectorXd> positions,
                                       Span<const VectorXd> velocities, Span<const VectorXd> accelerations) {
  if (positions.size() != velocities.size())
    return ::tpamd::compat::InvalidArgumentError("positions and velocity arguments have different size.");
  if (positions.size() != accelerations.size())
    return ::tpamd::compat::InvalidArgumentError("positions and accelerations arguments have different size.");
  if (positions.size() != times.size())
    return ::tpamd::compat::InvalidArgumentError("positions and times arguments have different size.");
  sequence_number_++;
  if (positions.empty()) return ::tpamd::compat::OkStatus();

  // the first sample later than times.front()
  auto it_upper = std::upper_bound(times_.begin(), times_.end(), times[0],
                                   [](const double a, const double b) { return a <= b; });
  if (positions_.empty() || it_upper == times_.begin()) {
    times_.assign(times.begin(), times.end());
    positions_.assign(positions.begin(), positions.end());
    velocities_.assign(velocities.begin(), velocities.end());
    accelerations_.assign(accelerations.begin(), accelerations.end());
    sequence_number_ = 0;
    return ::tpamd::compat::OkStatus();
  }
  // the new first sample is just after an existing one: replace that one
  if (times[0] - *std::prev(it_upper) < options_.timestep_tolerance) --it_upper;
  const size_t samples_to_keep = (size_t)(it_upper - times_.begin());
  times_.resize(samples_to_keep);
  positions_.resize(samples_to_keep);
  velocities_.resize(samples_to_keep);
  accelerations_.resize(samples_to_keep);
  times_.insert(times_.end(), times.begin(), times.end());
  positions_.insert(positions_.end(), positions.begin(), positions.end());
  velocities_.insert(velocities_.end(), velocities.begin(), velocities.end());
  accelerations_.insert(accelerations_.end(), accelerations.begin(), accelerations.end());
  return ::tpamd::compat::OkStatus();
}

StatusOr<VectorXd> TrajectoryBuffer::ValueAtTime(const std::vector<VectorXd> &values, double time_sec) const {
  if (times_.empty()) return ::tpamd::compat::FailedPreconditionError("No samples.");
  if (time_sec < times_.front() || time_sec > times_.back())
    return ::tpamd::compat::OutOfRangeError("Time outside the trajectory");
  const auto upper = std::upper_bound(times_.begin(), times_.end(), time_sec);
  if (upper == times_.end()) return values.back();
  const size_t u = upper - times_.begin(), l = u - 1;
  const double t = (time_sec - times_[l]) / (times_[u] - times_[l]);
  VectorXd v(values[l].size());
  for (size_t d = 0; d < v.size(); d++) v[d] = values[l][d] + t * (values[u][d] - values[l][d]);
  return v;
}

Status TrajectoryBuffer::AppendSample(double time, const VectorXd &positions, const VectorXd &velocities,
                                      const VectorXd &accelerations) {
  if (!times_.empty() && times_.back() >= time)
    return ::tpamd::compat::InvalidArgumentError("time must be > times_.back().");
  times_.push_back(time);
  positions_.push_back(positions);
  velocities_.push_back(velocities);
  accelerations_.push_back(accelerations);
  return ::tpamd::compat::OkStatus();
}

void TrajectoryBuffer::DiscardSegmentBefore(Time time) { DiscardSegmentBefore(TimeToSec(time)); }

void TrajectoryBuffer::DiscardSegmentBefore(const double time_sec) {
  if (times_.empty()) return;
  if (time_sec <= times_.front()) return;
  if (time_sec > times_.back()) {
    Clear();
    return;
  }
  // the first sample at or after time_sec
  int offset = (int)(std::upper_bound(times_.begin(), times_.end(), time_sec,
                                      [](const double a, const double b) { return a <= b; }) -
                     times_.begin());
  if (offset <= 0) return;
  if (offset >= (int)times_.size()) offset = (int)times_.size() - 1;   // unsorted times only
  // The sample before it stays if it is within the tolerance of time_sec, or if it is to become
  // the interpolated first sample.
  const bool close_to_existing_sample = time_sec - times_[offset - 1] <= options_.timestep_tolerance;
  const bool create_initial_sample_by_interpolation =
      std::fabs(times_[offset] - time_sec) > options_.timestep_tolerance;
  if (close_to_existing_sample || create_initial_sample_by_interpolation) --offset;
  if (create_initial_sample_by_interpolation) {
    const auto start_position = GetPositionAtTime(time_sec);
    const auto start_velocity = GetVelocityAtTime(time_sec);
    const auto start_acceleration = GetAccelerationAtTime(time_sec);
    if (start_position.ok() && start_velocity.ok() && start_acceleration.ok()) {   // by construction
      times_[offset] = time_sec;
      positions_[offset] = *start_position;
      velocities_[offset] = *start_velocity;
      accelerations_[offset] = *start_acceleration;
    }
  }
  times_.erase(times_.begin(), times_.begin() + offset);
  positions_.erase(positions_.begin(), positions_.begin() + offset);
  velocities_.erase(velocities_.begin(), velocities_.begin() + offset);
  accelerations_.erase(accelerations_.begin(), accelerations_.begin() + offset);
}

Span<const VectorXd> TrajectoryBuffer::GetPositionsUpToTime(Time time) const {
  if (times_.empty()) return Span<const VectorXd>();
  const double time_sec = TimeToSec(time);
  if (time_sec < times_.front() || time_sec > times_.back()) return Span<const VectorXd>();
  const auto it = std::upper_bound(times_.begin(), times_.end(), time_sec);   // the first sample after time
  return Span<const VectorXd>(positions_.data(), (size_t)((it - 1) - times_.begin()));
}

void TrajectoryBuffer::AddOffsetToTimestamps(::tpamd::compat::Duration offset) {
  AddOffsetToTimestamps(offset / ::tpamd::compat::Seconds(1));
}
void TrajectoryBuffer::AddOffsetToTimestamps(const double offset) {
  for (double &time : times_) time = time + offset;
}

StatusOr<VectorXd> TrajectoryBuffer::GetPositionAtTime(double time_sec) const {
  return ValueAtTime(positions_, time_sec);
}
StatusOr<VectorXd> TrajectoryBuffer::GetVelocityAtTime(double time_sec) const {
  return ValueAtTime(velocities_, time_sec);
}
StatusOr<VectorXd> TrajectoryBuffer::GetAccelerationAtTime(double time_sec) const {
  return ValueAtTime(accelerations_, time_sec);
}
StatusOr<VectorXd> TrajectoryBuffer::GetPositionAtTime(Time time) const { return GetPositionAtTime(TimeToSec(time)); }
StatusOr<VectorXd> TrajectoryBuffer::GetVelocityAtTime(Time time) const { return GetVelocityAtTime(TimeToSec(time)); }
StatusOr<VectorXd> TrajectoryBuffer::GetAccelerationAtTime(Time time) const {
  return GetAccelerationAtTime(TimeToSec(time));
}

Status TrajectoryBuffer::StopAtIndex(int index, const VectorXd &max_acceleration, double time_step) {
  const int n = (int)GetNumSamples();
  if (index <= 0 || index > n - 1)
    return ::tpamd::compat::OutOfRangeError("index (" + std::to_string(index) + ")  out of range (0, " +
                                            std::to_string(n - 1) + "].");
  double min_acceleration = max_acceleration.size() ? max_acceleration[0] : 0.0;
  for (size_t j = 1; j < max_acceleration.size(); j++)
    min_acceleration = max_acceleration[j] < min_acceleration ? max_acceleration[j] : min_acceleration;
  if (min_acceleration <= 0.0)
    return ::tpamd::compat::InvalidArgumentError("max_acceleration has non-positive minimum coefficient " +
                                                 std::to_string(min_acceleration));
  if (time_step <= 0.0)
    return ::tpamd::compat::InvalidArgumentError("`time_step` should be positive but is " +
                                                 std::to_string(time_step) + ".");

  constexpr double kVerySmall = 1e-4;
  if (index == n - 1 && velocities_.back().maxAbs() < kVerySmall) {
    velocities_.back().setZero();
    accelerations_.back().setZero();
    return ::tpamd::compat::OkStatus();
  }

  const size_t samples_for_stop = (size_t)index + 1;
  const auto rescaled = RescaleTrajectoryBackwardToStop(
      max_acceleration, Span<const double>(times_.data(), samples_for_stop),
      Span<const VectorXd>(positions_.data(), samples_for_stop),
      Span<const VectorXd>(velocities_.data(), samples_for_stop),
      Span<const VectorXd>(accelerations_.data(), samples_for_stop));
  if (!rescaled.ok()) return rescaled.status();
  const SampledTrajectory &stop = *rescaled;
  // The reference aborts here (CHECK); this happens when sample `index` is already at rest.
  if (stop.times.empty())
    return ::tpamd::compat::InternalError("sample " + std::to_string(index) +
                                          " is at rest before the end: no stopping trajectory");

  // A rest sample without an admissible deceleration (every candidate invalid at rate 0) makes the
  // first rescaled step 2 dt / 0 and the segment's times NaN; the reference inserts them.
  if (!std::isfinite(stop.times.front()))
    return ::tpamd::compat::InternalError("sample " + std::to_string(index) +
                                          " has no admissible deceleration: no stopping trajectory");

  // A stop that needs every sample must match the original velocity where it starts.
  if (stop.times.size() == (size_t)index) {
    const auto velocity_at_start = GetVelocityAtTime(stop.times.front());
    if (!velocity_at_start.ok()) return velocity_at_start.status();
    double err = 0.0;
    for (size_t j = 0; j < stop.velocities.front().size(); j++) {
      const double e = std::fabs((*velocity_at_start)[j] - stop.velocities.front()[j]);
      err = e > err ? e : err;
    }
    constexpr double kAcceptableMatchError = 1e-2;
    if (err > kAcceptableMatchError)
      return ::tpamd::compat::NotFoundError("No safe stopping trajectory found (likely not enough time).");
  }
  return InsertSegment(stop.times, stop.positions, stop.velocities, stop.accelerations);
}

Status TrajectoryBuffer::StopBeforeTime(Time time, const VectorXd &max_acceleration, double time_step) {
  return StopBeforeTime(TimeToSec(time), max_acceleration, time_step);
}

Status TrajectoryBuffer::StopBeforeTime(double time_sec, const VectorXd &max_acceleration, double time_step) {
  if (times_.empty()) return ::tpamd::compat::OkStatus();
  if (time_sec < times_.front()) return ::tpamd::compat::OutOfRangeError("time < times_.front().");
  // the sample after the first one at or after time_sec, or the last
  const int lower = (int)(std::lower_bound(times_.begin(), times_.end(), time_sec) - times_.begin());
  const int index = std::min<int>(lower + 1, (int)times_.size() - 1);
  return StopAtIndex(index, max_acceleration, time_step);
}

}  // namespace trajectory_planning

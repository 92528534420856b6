// Host mirror of trajectory_planning/trajectory_planner.h: TrajectoryPlannerOptions
// (:29-55) and the abstract TrajectoryPlanner (:59-160).
#ifndef TPAMD_HOST_TRAJECTORY_PLANNER_H_
#define TPAMD_HOST_TRAJECTORY_PLANNER_H_

#include <algorithm>
#include <memory>
#include <vector>

#include "compat.h"
#include "timeable_path.h"

namespace trajectory_planning {

using ::tpamd::compat::Duration;
using ::tpamd::compat::Time;

template <typename DerivedOptions>
class TrajectoryPlannerOptions {
 public:
  size_t GetNumDofs() const { return num_dofs_; }
  Duration GetTimeStep() const { return time_step_; }
  DerivedOptions &SetNumDofs(size_t n) { num_dofs_ = n; return static_cast<DerivedOptions &>(*this); }
  DerivedOptions &SetTimeStep(Duration d) { time_step_ = d; return static_cast<DerivedOptions &>(*this); }

 protected:
  Duration time_step_;
  size_t num_dofs_ = 0;
};

class TrajectoryPlanner {
 public:
  TrajectoryPlanner() = default;
  virtual ~TrajectoryPlanner() = default;

  void Reset() {
    ResetBase();
    ResetDerived();
  }
  virtual Status Plan(Time start, Duration time_horizon) = 0;
  size_t GetNumTimeSamples() const { return time_.size(); }
  Time GetStartTime() const { return start_time_; }
  Time GetEndTime() const { return end_time_; }
  const std::vector<double> &GetTime() const { return time_; }
  const std::vector<VectorXd> &GetPositions() const { return positions_; }
  const std::vector<VectorXd> &GetVelocities() const { return velocities_; }
  const std::vector<VectorXd> &GetAccelerations() const { return accelerations_; }
  const std::vector<double> &GetPathParameters() const { return path_parameter_; }
  const std::vector<double> &GetPathParameterDerivatives() const { return path_parameter_derivative_; }
  const std::vector<double> &GetSecondPathParameterDerivatives() const {
    return second_path_parameter_derivative_;
  }
  // TrajectoryBuffer::Get{Position,Velocity,Acceleration}AtTime (trajectory_buffer.cc:228-294):
  // the bracket of `time` by upper_bound over GetTime(), then InterpolateLinear (a + t (b - a)
  // with t the time fraction) between its rows; a time on the last sample gives that sample.
  // FailedPrecondition without samples, OutOfRange outside [first, last] time stamp.
  ::tpamd::compat::StatusOr<VectorXd> GetPositionAtTime(Time time) const { return ValueAtTime(positions_, time); }
  ::tpamd::compat::StatusOr<VectorXd> GetVelocityAtTime(Time time) const { return ValueAtTime(velocities_, time); }
  ::tpamd::compat::StatusOr<VectorXd> GetAccelerationAtTime(Time time) const {
    return ValueAtTime(accelerations_, time);
  }
  virtual bool IsTrajectoryAtEnd() const {
    const bool path_unchanged = path_ == nullptr ||
                                (path_->GetState() != TimeablePath::State::kModifiedPath &&
                                 path_->GetState() != TimeablePath::State::kNewPath);
    return path_unchanged && target_reached_;
  }
  virtual Status SetPath(std::shared_ptr<TimeablePath> path) = 0;

 protected:
  virtual void ResetDerived() = 0;
  void ResetBase() {
    if (path_ != nullptr) path_->Reset();
    start_time_ = ::tpamd::compat::FromUnixSeconds(0.0);
    end_time_ = ::tpamd::compat::FromUnixSeconds(0.0);
    time_.clear();
    path_parameter_.clear();
    path_parameter_derivative_.clear();
    second_path_parameter_derivative_.clear();
    positions_.clear();
    velocities_.clear();
    accelerations_.clear();
    target_reached_ = false;
  }

  std::shared_ptr<TimeablePath> path_;
  Time start_time_, end_time_;
  std::vector<double> time_, path_parameter_, path_parameter_derivative_,
      second_path_parameter_derivative_;
  std::vector<VectorXd> positions_, velocities_, accelerations_;
  bool target_reached_ = false;

 private:
  // GetOffsetBracket (:233-251) and InterpolateLinear on one of the sample arrays
  ::tpamd::compat::StatusOr<VectorXd> ValueAtTime(const std::vector<VectorXd> &values, Time time) const {
    if (time_.empty()) return ::tpamd::compat::FailedPreconditionError("No samples.");
    const double time_sec = (double)::tpamd::compat::ToUnixNanos(time) / 1e9;
    if (time_sec < time_.front() || time_sec > time_.back())
      return ::tpamd::compat::OutOfRangeError("Time outside the trajectory");
    const auto upper = std::upper_bound(time_.begin(), time_.end(), time_sec);
    if (upper == time_.end()) return values.back();
    const size_t u = upper - time_.begin(), l = u - 1;
    const double t = (time_sec - time_[l]) / (time_[u] - time_[l]);
    VectorXd v(values[l].size());
    for (size_t d = 0; d < v.size(); d++) v[d] = values[l][d] + t * (values[u][d] - values[l][d]);
    return v;
  }
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_TRAJECTORY_PLANNER_H_

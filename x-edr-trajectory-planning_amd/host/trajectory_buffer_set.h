// TrajectoryBufferSet -- B TrajectoryBuffers (trajectory_buffer.h) of the same number of joints whose
// samples, sample counts and sequence numbers stay ON THE DEVICE (include/tpamd.h
// tpamd_buffer_set_*). The methods are TrajectoryBuffer's in batched form: each takes the list of
// buffers it works on (each listed once where the call changes buffers), runs one launch, and
// leaves every listed buffer as the same call on a TrajectoryBuffer would, bit for bit.
// InsertFromPlannerSet splices the trajectories a PathTimingTrajectorySet has just planned into the
// buffers device to device, so the control loop Plan -> InsertSegment -> DiscardSegmentBefore ->
// Get*AtTime moves only lists, statuses and setpoints over PCIe.
#ifndef TPAMD_HOST_TRAJECTORY_BUFFER_SET_H_
#define TPAMD_HOST_TRAJECTORY_BUFFER_SET_H_

#include <vector>

#include "engine_handle.h"
#include "path_timing_trajectory_set.h"
#include "sampled_trajectory.h"
#include "trajectory_buffer.h"

namespace trajectory_planning {

// GetNumSamples, GetSequenceNumber, GetStartTime, GetEndTime and the size of
// GetPositionsUpToTime(time) of one buffer
struct TrajectoryBufferInfo {
  size_t num_samples = 0;
  int sequence_number = 0;
  Time start_time, end_time;
  size_t positions_up_to_time = 0;
};

class TrajectoryBufferSet {
 public:
  // A set with an engine of its own. capacity: samples per buffer the set starts with (0: 256);
  // it grows as the inserts need.
  TrajectoryBufferSet(size_t num_buffers, size_t num_dofs, TrajectoryBufferOptions options = TrajectoryBufferOptions{},
                      size_t capacity = 0, int device = -1);
  // A set on the engine of `planners` with its number of joints, as InsertFromPlannerSet needs;
  // it must not outlive `planners`.
  TrajectoryBufferSet(const PathTimingTrajectorySet &planners, size_t num_buffers, size_t num_dofs,
                      TrajectoryBufferOptions options = TrajectoryBufferOptions{}, size_t capacity = 0);
  ~TrajectoryBufferSet();
  TrajectoryBufferSet(const TrajectoryBufferSet &) = delete;
  TrajectoryBufferSet &operator=(const TrajectoryBufferSet &) = delete;

  Status status() const { return init_status_; }     // construction outcome (no GPU, options: not ok)
  size_t size() const { return num_buffers_; }
  Status Reserve(size_t size);
  size_t DeviceBytes() const;

  // InsertSegment(segments[k]) on buffer buffers[k]. A segment whose vectors differ in size or
  // whose rows have the wrong dimension fails the call and changes nothing.
  std::vector<Status> InsertSegments(const std::vector<size_t> &buffers, const std::vector<SampledTrajectory> &segments);
  // InsertSegment of planner planners[k]'s trajectory (GetTime, GetPositions, ...) on buffer
  // buffers[k], device to device. `set` must be the planner set this buffer set was made on.
  std::vector<Status> InsertFromPlannerSet(const PathTimingTrajectorySet &set, const std::vector<size_t> &buffers,
                                           const std::vector<size_t> &planners);
  std::vector<Status> AppendSamples(const std::vector<size_t> &buffers, const std::vector<double> &times,
                                    const std::vector<VectorXd> &positions, const std::vector<VectorXd> &velocities,
                                    const std::vector<VectorXd> &accelerations);
  Status DiscardSegmentsBefore(const std::vector<size_t> &buffers, const std::vector<Time> &time);
  Status DiscardSegmentsBefore(const std::vector<size_t> &buffers, const std::vector<double> &time_sec);
  // StopBeforeTime in place; one status per listed buffer.
  std::vector<Status> StopBeforeTimes(const std::vector<size_t> &buffers, const std::vector<Time> &time,
                                      const std::vector<VectorXd> &max_acceleration, double time_step);
  // Get{Position,Velocity,Acceleration}AtTime(start[k] + j step), j < ticks (as
  // PathTimingTrajectorySet::GetSetpoints).
  Status GetSetpoints(const std::vector<size_t> &buffers, const std::vector<Time> &start, Duration step, int ticks,
                      TrajectorySetpoints *out) const;
  Status AddOffsetsToTimestamps(const std::vector<size_t> &buffers, const std::vector<Duration> &offset);
  Status AddOffsetsToTimestamps(const std::vector<size_t> &buffers, const std::vector<double> &offset);
  Status Clear(const std::vector<size_t> &buffers);
  // `time` empty: positions_up_to_time stays 0.
  Status GetInfo(const std::vector<size_t> &buffers, const std::vector<Time> &time,
                 std::vector<TrajectoryBufferInfo> *out) const;
  // GetTimes / GetPositions / GetVelocities / GetAccelerations of each listed buffer: one packed download.
  Status GetSamples(const std::vector<size_t> &buffers, std::vector<SampledTrajectory> *out) const;

 private:
  void Init(tpamd_engine *engine, TrajectoryBufferOptions options, size_t capacity);
  Status Ids(const std::vector<size_t> &buffers, std::vector<int32_t> *ids) const;

  const size_t num_buffers_, num_dofs_;
  Status init_status_;
  ::tpamd::EngineLease lease_;
  const PathTimingTrajectorySet *planners_ = nullptr;
  tpamd_buffer_set *set_ = nullptr;
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_TRAJECTORY_BUFFER_SET_H_

// BatchWaypointTiming -- BatchPathTiming for callers who have what the reference's users have,
// waypoints (TimeableJointSplinePath::SetWaypoints, timeable_path_joint_spline.cc:200-207): the fit
// runs on the device inside the engine call that times the paths (tpamd_time_waypoint_paths_host),
// so nothing is fitted on the host, a path's length need not be known to choose its delta, and
// paths are not bucketed by control-point count: one engine call per (joint count, constraint
// safety). Each path gets the result PathTimingTrajectory::ComputeTimingProfile would have produced
// for a new path without an initial velocity (path_timing_trajectory.cc:307-475: s from 0, zero start
// velocity), bit for bit what BatchPathTiming gives for TimeableJointSplinePath objects of the same
// waypoints and options.
#ifndef TPAMD_HOST_BATCH_WAYPOINT_TIMING_H_
#define TPAMD_HOST_BATCH_WAYPOINT_TIMING_H_

#include <vector>

#include "batch_path_timing.h"

namespace trajectory_planning {

class BatchWaypointTiming {
 public:
  // One more path. options: num_dofs, num_path_samples (3..8192), rounding, constraint_safety and
  // delta_parameter (unless CoverWholePath is on). Every waypoint and both limits must have
  // options.num_dofs() entries (InvalidArgument otherwise, the batch is unchanged), as
  // PathTimingTrajectorySet::SetWaypointPaths checks them; an empty waypoint list is accepted here and
  // comes back with status TPAMD_PATH_NO_WAYPOINTS.
  Status AddPath(const std::vector<VectorXd> &waypoints, const JointPathOptions &options,
                 Span<const double> max_velocity, Span<const double> max_acceleration);
  void Clear();
  size_t NumPaths() const { return paths_.size(); }
  // On: every path's samples cover exactly the whole path, delta = path_end / (num_path_samples - 1),
  // computed on the device where the length is known; the options' delta_parameter is not used.
  void CoverWholePath(bool on = true) { cover_whole_path_ = on; }
  // Times every path starting at path parameter 0 and time `time_start_sec`. The result has
  // BatchPathTiming's packed layout.
  Status ComputeTimingProfiles(double time_start_sec, BatchTimingResult *result);
  // What the fit found, per path, after ComputeTimingProfiles.
  const std::vector<int32_t> &num_control_points() const { return num_points_; }
  const std::vector<double> &path_end() const { return path_end_; }
  const std::vector<double> &delta_used() const { return delta_used_; }
  int EngineCallsOfLastCompute() const { return engine_calls_; }   // (check calls are not counted)
  // On: every group's solve is followed by one check of its solutions against the group's constraint rows
  // on the device (tpamd_check_joint_paths_host on the fitted splines the solve returns; the solve is asked
  // for them and for sd2), and the result carries violations / worst_sample / worst_row / worst_excess.
  // Off (default): the engine calls and the result are what they are without this option.
  void CheckSolutions(bool on = true) { check_solutions_ = on; }
  // BatchPathTiming::RefineSolutions for waypoint paths (tpamd_time_waypoint_paths_refined_host); off by
  // default, and with it off the engine calls and the result are what they are without this option.
  void RefineSolutions(const RefineOptions &options) { refine_ = options; }

 private:
  struct Path {
    std::vector<double> waypoints;      // [W][D]
    size_t W, D, N;
    double rounding, safety, delta;
    std::vector<double> vmax, amax;
  };
  std::vector<Path> paths_;
  bool cover_whole_path_ = false;
  bool check_solutions_ = false;
  RefineOptions refine_{/*enabled=*/false};
  std::vector<int32_t> num_points_;
  std::vector<double> path_end_, delta_used_;
  int engine_calls_ = 0;
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_BATCH_WAYPOINT_TIMING_H_

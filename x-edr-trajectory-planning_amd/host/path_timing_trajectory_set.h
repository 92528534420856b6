// PathTimingTrajectorySet -- B PathTimingTrajectory planners (path_timing_trajectory.h:91-186) with
// TimeableJointSplinePath paths (any number of control points) whose state stays ON THE DEVICE between Plan calls
// (include/tpamd.h tpamd_planner_set_*). Where PathTimingTrajectory::PlanBatch ships every
// planner's window history up and down on each call (about 200 MB each way for 1024 planners),
// a Plan call here moves 24 bytes per planner up and one 56-byte record down; the histories, the
// window loop, the resampling in time and the erase / append bookkeeping of
// path_timing_trajectory.cc:540-577, :660-684 run on the device. Every planner ends in exactly the
// state Plan(start, time_horizon) would have left a PathTimingTrajectory in.
//
// New goals: SetPath uploads a spline fitted on the host (TimeableJointSplinePath::SetWaypoints), or
// SetWaypointPaths fits the waypoints on the device, bit-identically. The online switch to new waypoints runs on the device
// (SwitchToWaypointPaths): stop parameter, velocity at the switch time and the spline edit, with
// no trajectory download. Splines of different sizes share a set. Trajectories come down only when
// asked for: one planner (GetTrajectory), several in one packed download (GetTrajectories), or only
// the setpoints at control ticks (GetSetpoints).
#ifndef TPAMD_HOST_PATH_TIMING_TRAJECTORY_SET_H_
#define TPAMD_HOST_PATH_TIMING_TRAJECTORY_SET_H_

#include <functional>
#include <memory>
#include <vector>

#include "engine_handle.h"
#include "path_timing_trajectory.h"
#include "timeable_path_cartesian_spline.h"
#include "timeable_path_joint_spline.h"

namespace trajectory_planning {

// What TrajectoryPlanner's getters return for one planner (trajectory_planner.h:81-110).
struct PlannedTrajectory {
  std::vector<double> time, path_parameter, path_parameter_derivative, second_path_parameter_derivative;
  std::vector<double> positions, velocities, accelerations;   // [samples][dofs], packed
};

// Setpoints of several planners at a grid of control ticks (GetSetpoints): positions, velocities
// and accelerations [planners][ticks][dofs], packed, and one status per (planner, tick). The
// values of a tick whose status is not ok are NaN.
struct TrajectorySetpoints {
  size_t num_planners = 0, num_ticks = 0, num_dofs = 0;
  std::vector<double> positions, velocities, accelerations;
  std::vector<Status> status;
};

// One planner's stop (StopTrajectoriesBeforeTime): the stopped trajectory is the planner's first
// `keep` samples followed by the segment's rows (time [rows], positions / velocities /
// accelerations [rows][dofs], packed). A failed stop keeps every sample and has no rows.
struct StoppingSegment {
  Status status;
  size_t keep = 0;
  std::vector<double> time, positions, velocities, accelerations;
};

// The paths of a Cartesian set as raw IK tables (SetIkTables), for callers whose IK is not a
// std::function: planner k's table is rows row_offsets[k] .. row_offsets[k + 1]) of ik_positions
// [rows][dofs] and jacobians [rows][6][dofs] (row-major); row r belongs to path parameter
// r * delta[k]. path_end[k] is the path's last knot (CloseToEnd). initial_velocity may be empty
// (zero); path_state[k] is 1 (kNewPath) or 2 (kModifiedPath), empty: all new.
struct IkTables {
  std::vector<int32_t> row_offsets;
  std::vector<double> ik_positions, jacobians;
  std::vector<double> path_end, max_translational_velocity, max_rotational_velocity, delta;
  std::vector<double> max_velocity, max_acceleration, initial_velocity;   // [planners][dofs]
  std::vector<int32_t> path_state;
};

// Limits and path options of the planners listed in SetCartesianWaypointPaths, one entry per listed
// planner (initial_velocity may be empty: zero). The roundings and delta_parameter are the
// CartesianPathOptions of every listed path (translation_rounding 0.05, rounding 0.2 and
// delta_parameter 0.005 are the options' defaults).
struct CartesianPathLimits {
  std::vector<VectorXd> max_velocity, max_acceleration, initial_velocity;
  std::vector<double> max_translational_velocity, max_rotational_velocity;
  double translation_rounding = 0.05, rotation_rounding = 0.2, delta_parameter = 0.005;
};

// The caller's IK on the device (SetCartesianWaypointPaths): pose_targets [rows][7] (translation, then
// quaternion w, x, y, z) and joint_targets [rows][dofs] are DEVICE pointers, row_offsets (host) says
// which rows belong to which loaded planner; the function fills the DEVICE arrays ik_positions
// [rows][dofs] and jacobians [rows][6][dofs] (row-major), enqueueing on hip_stream (a hipStream_t).
using DeviceIkFunc = std::function<Status(const double *pose_targets, const double *joint_targets,
                                          const std::vector<int32_t> &row_offsets, double *ik_positions,
                                          double *jacobians, void *hip_stream)>;

// The caller's IK on the device for streaming tables (SetCartesianWaypointPaths(..., streaming),
// PlanStreaming): as DeviceIkFunc, plus seed_rows [planners][dofs] (DEVICE), the initial value of
// each planner's run as the reference's callback receives it (initial_value,
// timeable_path_cartesian_spline.cc:504-506): the table's last resident row, whose targets the
// run's first row repeats. seed_rows is null for the first rows of a new path (the reference seeds
// those with the first joint target, which the function has in joint_targets).
using DeviceSeededIkFunc =
    std::function<Status(const double *pose_targets, const double *joint_targets, const std::vector<int32_t> &row_offsets,
                         const double *seed_rows, double *ik_positions, double *jacobians, void *hip_stream)>;

// Constructor tag of a Cartesian set: rows per planner the IK tables hold to start with (they grow).
struct CartesianTableCapacity {
  size_t rows;
};

class PathTimingTrajectorySet {
 public:
  // All planners share the planner options and the path options (dofs, samples; delta may differ
  // per path: it is taken from each path). num_control_points is the per-planner capacity the
  // set starts with; paths of any size are accepted and the capacity grows as needed.
  PathTimingTrajectorySet(const PathTimingTrajectoryOptions &options, size_t num_planners,
                          size_t num_control_points, double constraint_safety = 0.8, int device = -1);
  // A set of the second kind: every planner's path is the IK table of a
  // TimeableCartesianSplinePath (tpamd_planner_set_create_cartesian). Plan runs on the device on
  // the resident tables and leaves every planner in the state a PathTimingTrajectory that plans
  // the same path window by window is in -- provided the IK callback's result for a sample does not
  // depend on how the samples were split into calls (closed-form and per-sample solvers qualify; a
  // solver warm-started across the samples of one call does not). The contract of the set is the
  // table. A set holds one kind: the joint-spline methods (SetPath(s), SetWaypointPaths,
  // SwitchToWaypointPaths, GetPath) return FailedPrecondition on a Cartesian set, the Cartesian
  // ones on a joint set. Everything that reads the trajectories works on both.
  PathTimingTrajectorySet(const PathTimingTrajectoryOptions &options, size_t num_planners,
                          CartesianTableCapacity table_capacity, double constraint_safety = 0.8, int device = -1);
  ~PathTimingTrajectorySet();
  bool is_cartesian() const { return cartesian_; }
  // BuildIkTable on the path (one IK callback call over the whole path, one Jacobian callback per
  // row), then the table with the path's limits, delta, initial velocity and state go to the
  // device. The path must be kNewPath or kModifiedPath; its state does not change.
  // With `streaming` only rows 0 .. N-1 go up, built as the path's first SamplePath builds them
  // (ExtendIkTable), and the set keeps a pointer to the path: PlanStreaming extends the table when
  // a planner's window reaches past it. The path must outlive the set or its next path.
  Status SetCartesianPath(size_t planner, TimeableCartesianSplinePath &path, bool streaming = false);
  Status SetCartesianPaths(const std::vector<std::shared_ptr<TimeableCartesianSplinePath>> &paths,
                           bool streaming = false);
  // Raw tables for the listed planners (each listed once).
  Status SetIkTables(const std::vector<size_t> &planners, const IkTables &tables);
  // New Cartesian goals for the listed planners (each listed once) without per-row data on the host:
  // pose_waypoints[k] / joint_waypoints[k] are fitted on the device
  // (tpamd_fit_pose_waypoints_device: TimeableCartesianSplinePath::SetWaypoints), path_end comes
  // down and sizes each table (tpamd_ik_table_rows), the pose and joint targets of every table row
  // are sampled on the device (tpamd_sample_ik_targets_device), `ik` turns them into the tables in
  // device memory, and tpamd_planner_set_upload_ik_tables_device loads them as new paths. A planner
  // whose waypoint lists are empty, differ in length or hold a joint waypoint of the wrong
  // dimension is left as it is (path and plan); the others are loaded and the call returns
  // InvalidArgument naming the first such planner. FailedPrecondition on a joint set; a planner out
  // of range or listed twice, vectors of the wrong length or a non-positive delta_parameter fail the
  // call and change nothing. Synchronises.
  Status SetCartesianWaypointPaths(const std::vector<size_t> &planners,
                                   const std::vector<std::vector<Pose3d>> &pose_waypoints,
                                   const std::vector<std::vector<VectorXd>> &joint_waypoints,
                                   const CartesianPathLimits &limits, const DeviceIkFunc &ik);
  // The same chain for tables that grow: with `streaming` only rows 0 .. N-1 of every table are
  // sampled, solved and uploaded, and the fitted splines stay in device memory with the set.
  // PlanStreaming then extends a waiting planner's table on the device: the targets of rows
  // need_first - 1 .. need_first + need_count - 1 (tpamd_sample_ik_target_rows_device), `ik` with
  // the table's last row as the seed, and tpamd_planner_set_append_ik_rows_device for everything but
  // the re-evaluated first row. Nothing per row touches the host. Without `streaming` this is the
  // call above with a seeded IK (seed_rows null).
  Status SetCartesianWaypointPaths(const std::vector<size_t> &planners,
                                   const std::vector<std::vector<Pose3d>> &pose_waypoints,
                                   const std::vector<std::vector<VectorXd>> &joint_waypoints,
                                   const CartesianPathLimits &limits, const DeviceSeededIkFunc &ik, bool streaming);
  // Seconds the last SetCartesianPath(s) / PlanStreaming call spent in the paths' IK and Jacobian
  // callbacks on the host (measurement: tools/cartesian_stream_bench.cc).
  double HostCallbackSecondsOfLastCall() const { return callback_seconds_; }
  // The planner's resident table (no table: empty). An error once front rows were discarded
  // (DiscardIkRows): the table no longer starts at row 0; GetIkTableInfo says where it starts.
  Status GetIkTable(size_t planner, std::vector<double> *ik_positions, std::vector<double> *jacobians) const;
  // Path rows supplied to the planner's table so far (no download; discarded front rows count);
  // -1 on a joint set or a planner out of range.
  int GetIkTableRows(size_t planner) const;
  PathTimingTrajectorySet(const PathTimingTrajectorySet &) = delete;
  PathTimingTrajectorySet &operator=(const PathTimingTrajectorySet &) = delete;

  Status status() const { return init_status_; }      // construction outcome (no GPU: not ok)
  size_t size() const { return num_planners_; }
  // SetPath for one planner / for planners 0..paths.size()-1: the path must be kNewPath (after
  // SetWaypoints) or kModifiedPath (after SwitchToWaypointPath); its spline (any number of
  // control points >= 3), limits, sampling distance and initial velocity go to the device.
  Status SetPath(size_t planner, const TimeableJointSplinePath &path);
  Status SetPaths(const std::vector<std::shared_ptr<TimeableJointSplinePath>> &paths);
  void Reset(size_t planner);
  // Plan(start, time_horizon) for every planner; one status per planner.
  std::vector<Status> Plan(Time start, Duration time_horizon);
  std::vector<Status> Plan(const std::vector<Time> &start, const std::vector<Duration> &time_horizon);
  // Plan for a Cartesian set whose paths were loaded with `streaming`: the tables grow exactly as
  // TimeableCartesianSplinePath::SamplePath grows path_ik_positions_ (:464-549). While planners wait
  // for rows (tpamd_planner_set_plan_streaming), each waiting planner's path extends its IK solution
  // to the last row its window needs -- one IK callback call, seeded with the table's last row --,
  // the Jacobian callback runs on the new rows, one tpamd_planner_set_append_ik_rows takes all of
  // them and tpamd_planner_set_plan_resume goes on. The set then equals one PathTimingTrajectory
  // per planner planning window by window, also with an IK whose result depends on the split into
  // calls.
  // With `discard` every completed call ends with DiscardIkRows(): the tables keep the rows a later
  // Plan can read and stop growing with the distance travelled. Off by default; the plans are the
  // same either way, bit for bit.
  std::vector<Status> PlanStreaming(Time start, Duration time_horizon, bool discard = false);
  std::vector<Status> PlanStreaming(const std::vector<Time> &start, const std::vector<Duration> &time_horizon,
                                    bool discard = false);
  int SuspensionsOfLastPlan() const { return suspensions_; }
  // Capacity ahead of time (tpamd_planner_set_reserve / _capacity): the history and trajectory
  // buffers grow to at least these samples per planner, never shrink, and keep every planner's
  // state bit for bit; the engine's workspace is sized for this set. PlanDevice allocates nothing
  // after a Reserve. Synchronises when anything grows.
  Status Reserve(int history, int trajectory);
  Status GetCapacity(int *history, int *trajectory) const;
  // Plan, enqueued only (tpamd_planner_set_plan_device): start and horizon [planners] in
  // nanoseconds are DEVICE arrays that stay valid until hip_stream (a hipStream_t; null: the null
  // stream) has run the call; exactly max_windows window iterations are enqueued, and every planner
  // ends as Plan leaves it with GetMaxPlanningIterations() = min(the options' value,
  // max_windows - 1). Nothing is copied to the host and nothing blocks. A planner without room in
  // its history or for its trajectory gets ResourceExhausted (LastPlanDeviceInfo() says what
  // Reserve needs; then Reset and a new path). Work on the set may be enqueued behind the call on
  // the same stream (retargets, TrajectoryBufferSet::InsertFromPlannerSet on the device, ...).
  // Between PlanDevice and FinishPlanDevice the summary getters below (GetNumTimeSamples,
  // GetEndTime, IsTrajectoryAtEnd, WindowsOfLastPlan, ...) are STALE: they still describe the Plan
  // before; GetTrajectory / GetTrajectories, which size their download from them, and a second
  // PlanDevice or a Reserve return FailedPrecondition.
  Status PlanDevice(const int64_t *start_ns_dev, const int64_t *horizon_ns_dev, int max_windows, void *hip_stream);
  // Waits for the PlanDevice call, downloads the summaries and the info record and refreshes the
  // getters; one status per planner, as Plan returns them.
  std::vector<Status> FinishPlanDevice();
  bool PlanDevicePending() const { return plan_pending_; }
  const tpamd_plan_device_info &LastPlanDeviceInfo() const { return plan_info_; }
  // Discards, for every planner that has a table, the consumed rows below its safe floor
  // (tpamd_planner_set_discard_ik_rows with keep_from NULL: the lowest row a later Plan can read).
  // Returns the first resident row of every planner (0 for one without a table).
  ::tpamd::compat::StatusOr<std::vector<int32_t>> DiscardIkRows();
  // (first resident row, path rows supplied, table rows allocated per planner) of one planner
  Status GetIkTableInfo(size_t planner, int32_t *first_row, int32_t *rows, int32_t *capacity) const;

  // State after the last Plan, from the summary record (no trajectory download).
  size_t GetNumTimeSamples(size_t planner) const { return (size_t)summary_[planner].num_samples; }
  Time GetStartTime(size_t planner) const { return ::tpamd::compat::FromUnixNanos(summary_[planner].start_time_ns); }
  Time GetEndTime(size_t planner) const { return ::tpamd::compat::FromUnixNanos(summary_[planner].end_time_ns); }
  Time GetFinalDecelStart(size_t planner) const {
    return ::tpamd::compat::FromUnixNanos(summary_[planner].final_decel_start_ns);
  }
  Time GetNextPlanStartTime(size_t planner, Time target_time) const {
    return std::min(GetEndTime(planner), std::max(target_time, GetStartTime(planner)));
  }
  bool IsTrajectoryAtEnd(size_t planner) const {      // trajectory_planner.h:103-110
    const int st = summary_[planner].path_state;
    return st != 1 && st != 2 && summary_[planner].target_reached != 0;
  }
  int WindowsOfLastPlan(size_t planner) const { return summary_[planner].windows; }
  // PathTimingTrajectory::GetPathStopParameter(time) on the resident trajectories after the last
  // Plan (tpamd_planner_set_stop_parameters): one planner, or every planner with one time each
  // (one launch, no trajectory download). No planner state changes.
  ::tpamd::compat::StatusOr<double> GetPathStopParameter(size_t planner, Time time) const;
  std::vector<::tpamd::compat::StatusOr<double>> GetPathStopParameters(const std::vector<Time> &time) const;
  // The online path switch of path_timing_trajectory_test.cc:298-420 for the listed planners, on
  // the device (tpamd_planner_set_switch_paths): stop = GetPathStopParameter(time[k]);
  // path->SwitchToWaypointPath(stop, waypoints[k]); path->SetInitialVelocity(the trajectory's
  // GetVelocityAtTime(time[k])). The next Plan plans the modified path. One status per listed
  // planner; a planner whose switch failed keeps its state. The new control polygon is rounded
  // with the PathOptions default radius (0.2).
  std::vector<Status> SwitchToWaypointPaths(const std::vector<size_t> &planners, const std::vector<Time> &time,
                                            const std::vector<std::vector<VectorXd>> &waypoints);
  // The same with the new control polygon rounded with `rounding`, as a path whose
  // PathOptions::rounding has that value switches (tpamd_planner_set_switch_paths_rounded).
  std::vector<Status> SwitchToWaypointPaths(const std::vector<size_t> &planners, const std::vector<Time> &time,
                                            const std::vector<std::vector<VectorXd>> &waypoints, double rounding);
  // Redirects the listed moving planners (each listed once) onto new waypoints, abandoning the old
  // path at `time[k]`, on the device (tpamd_planner_set_retarget). Planner planners[k] ends in the
  // state that this sequence on a PathTimingTrajectory `planner` with a fresh path leaves, bit for
  // bit (path_tools.h:44-53):
  //   TrajectoryBuffer buffer(...); buffer.InsertTrajectory(planner's time / positions / velocities /
  //       accelerations);
  //   position = buffer.GetPositionAtTime(time[k]); velocity = buffer.GetVelocityAtTime(time[k]);
  //   stop = ComputeStoppingPoint(position, velocity, stopping_acceleration[k], rounding);
  //   path->SetWaypoints({position, stop, waypoints[k]...})   ({position, waypoints[k]...} if every
  //       |velocity| is below 100 epsilon: ComputeStoppingPoint then returns the position), with
  //       PathOptions rounding `rounding` and delta_parameter `delta_parameter`;
  //   path->SetMaxJointVelocity(max_velocity[k]); path->SetMaxJointAcceleration(max_acceleration[k]);
  //   path->SetInitialVelocity(velocity); planner.SetPath(path);
  // so that the next Plan(time[k], horizon) continues from the trajectory at time[k].
  // stopping_acceleration may be empty (max_acceleration for all); waypoints[k] may be empty (the
  // path is the straight stop). One status per listed planner: FailedPrecondition without a plan,
  // OutOfRange for a time outside the trajectory, InvalidArgument for a waypoint or limit of the
  // wrong dimension or a non-positive stopping acceleration ("Acceleration limits must be strictly
  // positive."); such a planner keeps its state. A planner out of range or listed twice, or
  // vectors of the wrong length, fail the call and change nothing.
  std::vector<Status> RetargetWaypointPaths(const std::vector<size_t> &planners, const std::vector<Time> &time,
                                            const std::vector<std::vector<VectorXd>> &waypoints,
                                            const std::vector<VectorXd> &max_velocity,
                                            const std::vector<VectorXd> &max_acceleration, double rounding = 0.2,
                                            double delta_parameter = 0.005,
                                            const std::vector<VectorXd> &stopping_acceleration = {});
  // Position, velocity and stopping point [listed planners][dofs] of the last RetargetWaypointPaths
  // call (rows of planners that failed are NaN).
  const std::vector<double> &LastRetargetPositions() const { return retarget_position_; }
  const std::vector<double> &LastRetargetVelocities() const { return retarget_velocity_; }
  const std::vector<double> &LastRetargetStoppingPoints() const { return retarget_stop_; }
  // New waypoint paths for the listed planners (each listed once), fitted on the device
  // (tpamd_planner_set_set_waypoints): planner planners[k] ends in the state that
  //   path->SetWaypoints(waypoints[k]) (with PathOptions rounding `rounding` and delta_parameter
  //   `delta_parameter`); path->SetMaxJointVelocity(max_velocity[k]);
  //   path->SetMaxJointAcceleration(max_acceleration[k]); path->SetInitialVelocity(initial_velocity[k]);
  //   SetPath(planners[k], *path)
  // leaves, bit for bit. initial_velocity may be empty (zero for all). One status per listed
  // planner: a waypoint or a limit of the wrong dimension or an empty waypoint list gives
  // InvalidArgument and leaves that planner unchanged. A planner out of range or listed twice, or
  // vectors of the wrong length, fail the call and change nothing.
  std::vector<Status> SetWaypointPaths(const std::vector<size_t> &planners,
                                       const std::vector<std::vector<VectorXd>> &waypoints,
                                       const std::vector<VectorXd> &max_velocity,
                                       const std::vector<VectorXd> &max_acceleration,
                                       const std::vector<VectorXd> &initial_velocity, double rounding = 0.2,
                                       double delta_parameter = 0.005);
  // The planner's resident spline (no path: empty) and its number of control points.
  Status GetPath(size_t planner, std::vector<double> *knots, std::vector<double> *control_points) const;
  size_t NumControlPoints(size_t planner) const;
  // The planner's trajectory (GetTime, GetPositions, ...): one download of its samples.
  Status GetTrajectory(size_t planner, PlannedTrajectory *out) const;
  // GetTrajectory for each listed planner (repeats allowed) in one call: one packed download
  // (tpamd_planner_set_download_trajectories). out->at(k) is planner planners[k]'s trajectory.
  Status GetTrajectories(const std::vector<size_t> &planners, std::vector<PlannedTrajectory> *out) const;
  // TrajectoryBuffer::Get{Position,Velocity,Acceleration}AtTime(start[k] + j step) of each listed
  // planner k for ticks j < ticks, on the device (tpamd_planner_set_sample_at_ticks): the same
  // values and statuses as the per-planner getters. A planner out of range, step <= 0 or ticks < 1
  // fails the call.
  Status GetSetpoints(const std::vector<size_t> &planners, const std::vector<Time> &start, Duration step, int ticks,
                      TrajectorySetpoints *out) const;
  // TrajectoryBuffer::StopBeforeTime(time[k], max_acceleration[k], time_step) on each listed
  // planner's trajectory as GetTrajectory gives it, loaded into a TrajectoryBuffer
  // (host/trajectory_buffer.h), on the device (tpamd_planner_set_stop_trajectories): per planner the
  // status, keep and the segment. No planner state changes; the next Plan is unaffected. A planner
  // out of range or a max_acceleration of the wrong size fails the call.
  Status StopTrajectoriesBeforeTime(const std::vector<size_t> &planners, const std::vector<Time> &time,
                                    const std::vector<VectorXd> &max_acceleration, double time_step,
                                    std::vector<StoppingSegment> *out) const;
  // Checks every window the set's Plan calls solve against its constraint rows, on the device
  // (tpamd_planner_set_set_checking; off by default). CheckResults: the record of each listed planner
  // over the windows of its last Plan call (listed once each; synchronises). CheckResultsDevice:
  // the same into device memory (planners_dev: device ids or null for planners 0 .. count-1),
  // enqueued on hip_stream behind a PlanDevice, no synchronisation.
  Status SetChecking(bool on);
  bool Checking() const { return tpamd_planner_set_checking(set_) != 0; }
  Status CheckResults(const std::vector<size_t> &planners, std::vector<tpamd_planner_check> *out) const;
  Status CheckResultsDevice(int count, const int32_t *planners_dev, tpamd_planner_check *out_dev, void *hip_stream) const;
  // Bytes the last Plan call moved over PCIe, both directions.
  size_t LastPlanBytesOverPcie() const;
  size_t DeviceBytes() const;
  // ---- moving planners between sets (tpamd_planner_set_export_state_host / _import_state_host /
  // _copy_planners; csrc/tpamd_state.h states the record format). A planner that was moved continues
  // bit for bit as it would have where it was. The receiving set must have the same kind, dofs, path
  // samples, sampling method, time step, constraint safety and initial-velocity tolerance; its
  // number of planners and capacities may differ (it grows as needed). A planner that waits for IK
  // rows (a suspended PlanStreaming) is refused with a failed precondition.
  struct PlannerStateBlob {
    std::vector<unsigned char> bytes;    // the records, packed
    std::vector<int64_t> offsets;        // [planners + 1]: record k is bytes[offsets[k] .. offsets[k + 1])
    std::vector<Status> status;          // [planners]: per planner, what ExportPlanners found
  };
  // The records of the listed planners, on the host. Synchronises.
  Status ExportPlanners(const std::vector<size_t> &planners, PlannerStateBlob *blob);
  // The listed planners (each listed once) take the records of `blob`, in order. Every id and record
  // is checked before anything changes (an invalid-argument status for all of them then). The
  // getters (GetEndTime, GetNumTimeSamples, ...) of a planner that took a record answer from it. A
  // planner that took a record loses its stream source: where the rows of a streamed Cartesian table
  // come from (the path object or the device fit) is this object's knowledge, not the record's, so a
  // PlanStreaming that needs further rows for it fails until it is given a path again.
  std::vector<Status> ImportPlanners(const std::vector<size_t> &planners, const PlannerStateBlob &blob);
  // Planner src_planners[k] of src becomes planner dst_planners[k] of dst; dst may be src (any
  // permutation). On one device nothing crosses PCIe but sizes and summaries; sets on different
  // devices go through host memory. Getters and stream sources of dst as for ImportPlanners.
  static std::vector<Status> CopyPlanners(PathTimingTrajectorySet *dst, const std::vector<size_t> &dst_planners,
                                          PathTimingTrajectorySet *src, const std::vector<size_t> &src_planners);
  // A planner written against the reference's API joins the set, and leaves it, without starting
  // from rest (planner_state.h: the record of a host PathTimingTrajectory with a
  // TimeableJointSplinePath). AdoptPlanner: planner `slot` takes the host planner's whole state
  // (path, limits, history, scalars, trajectory) and continues bit for bit as the host planner
  // would; the host planner is not changed. The options must agree (dofs, path samples, sampling
  // method, time step, initial-velocity tolerance, and the path's constraint safety with the set's).
  // ReleasePlanner: `planner` takes the state of planner `slot` (PlannerStateToHost says what a
  // record cannot restore), and the slot is reset. Joint sets only.
  Status AdoptPlanner(size_t slot, const PathTimingTrajectory &planner);
  Status ReleasePlanner(size_t slot, PathTimingTrajectory *planner);
  // The C-ABI set and its engine, for objects that work on the resident trajectories in place
  // (TrajectoryBufferSet::InsertFromPlannerSet). They stay owned by this set.
  tpamd_planner_set *native_handle() const { return set_; }
  tpamd_engine *engine() const { return lease_.get(); }

 private:
  const PathTimingTrajectoryOptions options_;
  const size_t num_planners_, num_control_points_;
  const double constraint_safety_;
  const bool cartesian_ = false;
  Status init_status_;
  ::tpamd::EngineLease lease_;
  tpamd_planner_set *set_ = nullptr;
  std::vector<tpamd_planner_summary> summary_;
  // streaming Cartesian sets: the path each planner's table is extended from (null: none)
  std::vector<TimeableCartesianSplinePath *> stream_paths_;
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> stream_keep_;
  int suspensions_ = 0;
  // PlanDevice: the summaries [planners] and the info record in device memory, the stream of the
  // call in flight
  void *plan_results_ = nullptr;
  void *plan_stream_ = nullptr;
  bool plan_pending_ = false;
  tpamd_plan_device_info plan_info_{};
  std::vector<double> retarget_position_, retarget_velocity_, retarget_stop_;
  double callback_seconds_ = 0.0;
  // streaming through the device chain: the fitted splines of one SetCartesianWaypointPaths call,
  // resident until none of its planners refers to them
  struct StreamFit;
  std::vector<std::shared_ptr<StreamFit>> stream_fits_;      // [planner] (null: none)
  std::vector<int> stream_fit_index_;                        // [planner] its path in the fit
  void ForgetStreamSource(size_t planner);                   // the planner's table was replaced
  Status WaypointPathsImpl(const std::vector<size_t> &planners, const std::vector<std::vector<Pose3d>> &pose_waypoints,
                           const std::vector<std::vector<VectorXd>> &joint_waypoints, const CartesianPathLimits &limits,
                           const DeviceSeededIkFunc &ik, bool streaming);
  Status ExtendOnDevice(const std::vector<int32_t> &need_first, const std::vector<int32_t> &need_count,
                        std::vector<Status> *failed);
  std::vector<Status> PlanStatuses() const;
  void TakeImported(const std::vector<size_t> &planners, const std::vector<int32_t> &status,
                    const std::vector<tpamd_planner_summary> &summary, std::vector<Status> *result);
};

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_PATH_TIMING_TRAJECTORY_SET_H_

#include "path_timing_trajectory_set.h"
#include "planner_state.h"

#include <chrono>

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <limits>
#include <string>

namespace trajectory_planning {

using ::tpamd::compat::DeadlineExceededError;
using ::tpamd::compat::FailedPreconditionError;
using ::tpamd::compat::InternalError;
using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::NotFoundError;
using ::tpamd::compat::OkStatus;
using ::tpamd::compat::OutOfRangeError;
using ::tpamd::compat::StatusOr;

namespace {
tpamd_planner_set_config SetConfig(const PathTimingTrajectoryOptions &options, size_t num_planners,
                                   size_t num_control_points, double constraint_safety) {
  tpamd_planner_set_config cfg{};
  cfg.num_planners = (int32_t)num_planners; cfg.num_dofs = (int32_t)options.GetNumDofs();
  cfg.num_samples = (int32_t)options.GetNumPathSamples(); cfg.num_points = (int32_t)num_control_points;
  cfg.history_capacity = 0; cfg.trajectory_capacity = 0;
  cfg.sampling_method =
      options.GetTimeSamplingMethod() == PathTimingTrajectoryOptions::TimeSamplingMethod::kUniformlyInTime ? 0 : 1;
  cfg.max_planning_iterations = options.GetMaxPlanningIterations();
  cfg.constraint_safety = constraint_safety;
  cfg.max_initial_velocity_error = options.GetMaxInitialVelocityError();
  cfg.time_step_ns = options.GetTimeStep().nanos();
  return cfg;
}
}  // namespace

PathTimingTrajectorySet::PathTimingTrajectorySet(const PathTimingTrajectoryOptions &options, size_t num_planners,
                                                 size_t num_control_points, double constraint_safety, int device)
    : options_(options), num_planners_(num_planners), num_control_points_(num_control_points),
      constraint_safety_(constraint_safety), summary_(num_planners) {
  lease_ = ::tpamd::acquire_engine(device);
  if (!lease_) { init_status_ = InternalError("no GPU engine"); return; }
  const tpamd_planner_set_config cfg = SetConfig(options, num_planners, num_control_points, constraint_safety);
  const int rc = tpamd_planner_set_create(lease_.get(), &cfg, &set_);
  if (rc != 0) init_status_ = InternalError(tpamd_error_string(rc));
}

PathTimingTrajectorySet::PathTimingTrajectorySet(const PathTimingTrajectoryOptions &options, size_t num_planners,
                                                 CartesianTableCapacity table_capacity, double constraint_safety,
                                                 int device)
    : options_(options), num_planners_(num_planners), num_control_points_(3), constraint_safety_(constraint_safety),
      cartesian_(true), summary_(num_planners) {
  lease_ = ::tpamd::acquire_engine(device);
  if (!lease_) { init_status_ = InternalError("no GPU engine"); return; }
  const tpamd_planner_set_config cfg = SetConfig(options, num_planners, 3, constraint_safety);
  const int rc = tpamd_planner_set_create_cartesian(lease_.get(), &cfg, (int)table_capacity.rows, &set_);
  if (rc != 0) init_status_ = InternalError(tpamd_error_string(rc));
}

PathTimingTrajectorySet::~PathTimingTrajectorySet() {
  if (plan_pending_) (void)hipStreamSynchronize((hipStream_t)plan_stream_);   // the call writes plan_results_
  if (set_) tpamd_planner_set_destroy(set_);     // before the engine goes back to the pool
  if (plan_results_) (void)hipFree(plan_results_);
}

namespace {
double NowSeconds() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
int StateCode(TimeablePath::State s) {
  switch (s) {
    case TimeablePath::State::kNewPath: return 1;
    case TimeablePath::State::kModifiedPath: return 2;
    case TimeablePath::State::kPathWasSampled: return 3;
    default: return 0;
  }
}
}  // namespace

Status PathTimingTrajectorySet::SetPath(size_t planner, const TimeableJointSplinePath &path) {
  if (!init_status_.ok()) return init_status_;
  if (cartesian_) return FailedPreconditionError("a Cartesian set takes IK tables (SetCartesianPath)");
  if (planner >= num_planners_) return InvalidArgumentError("no such planner");
  if (path.NumDofs() != options_.GetNumDofs()) return InvalidArgumentError("Path and planner disagree on the number of dofs");
  if (path.NumPathSamples() != options_.GetNumPathSamples())
    return InvalidArgumentError("Path and planner disagree on the number of path samples");
  if (path.num_control_points() < 3) return FailedPreconditionError("SetWaypoints / SwitchToWaypointPath first");
  if (path.options().constraint_safety() != constraint_safety_) return InvalidArgumentError("constraint safety differs");
  const int state = StateCode(path.GetState());
  if (state != 1 && state != 2) return FailedPreconditionError("SetWaypoints / SwitchToWaypointPath first");
  const int32_t id = (int32_t)planner, st = state, np = path.num_control_points();
  const double delta = path.GetPathSamplingDistance();
  const int rc = tpamd_planner_set_upload_paths_ragged(
      set_, 1, &id, &np, path.knots().data(), path.packed_control_points().data(), path.GetMaxJointVelocity().data(),
      path.GetMaxJointAcceleration().data(), &delta, path.GetInitialVelocity().data(), &st);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  summary_[planner].path_state = state;
  return OkStatus();
}

Status PathTimingTrajectorySet::SetCartesianPath(size_t planner, TimeableCartesianSplinePath &path, bool streaming) {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set takes joint spline paths (SetPath)");
  if (planner >= num_planners_) return InvalidArgumentError("no such planner");
  const size_t D = options_.GetNumDofs();
  if (path.NumDofs() != D || path.NumPathSamples() != options_.GetNumPathSamples() ||
      path.options().constraint_safety() != constraint_safety_)
    return InvalidArgumentError("path does not have the shape of the set");
  const int state = StateCode(path.GetState());
  if (state != 1 && state != 2) return FailedPreconditionError("SetWaypoints first");
  if (path.GetMaxJointVelocity().size() != D || path.GetMaxJointAcceleration().size() != D)
    return FailedPreconditionError("set the joint limits first");
  IkTables t;
  const double t0 = NowSeconds();
  if (Status st = streaming ? path.ExtendIkTable(0, (int)options_.GetNumPathSamples() - 1, &t.ik_positions, &t.jacobians)
                            : path.BuildIkTable(&t.ik_positions, &t.jacobians);
      !st.ok())
    return st;
  callback_seconds_ = NowSeconds() - t0;
  t.row_offsets = {0, (int32_t)(t.ik_positions.size() / D)};
  t.path_end = {path.knots().back()};
  t.max_translational_velocity = {path.max_translational_velocity()};
  t.max_rotational_velocity = {path.max_rotational_velocity()};
  t.delta = {path.GetPathSamplingDistance()};
  t.max_velocity.assign(path.GetMaxJointVelocity().begin(), path.GetMaxJointVelocity().end());
  t.max_acceleration.assign(path.GetMaxJointAcceleration().begin(), path.GetMaxJointAcceleration().end());
  if (path.GetInitialVelocity().size() == D)
    t.initial_velocity.assign(path.GetInitialVelocity().begin(), path.GetInitialVelocity().end());
  t.path_state = {state};
  const Status up = SetIkTables({planner}, t);
  if (up.ok() && streaming) stream_paths_[planner] = &path;      // SetIkTables forgot the planner's previous source
  return up;
}

Status PathTimingTrajectorySet::SetCartesianPaths(const std::vector<std::shared_ptr<TimeableCartesianSplinePath>> &paths,
                                                  bool streaming) {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set takes joint spline paths (SetPaths)");
  if (paths.size() > num_planners_) return InvalidArgumentError("more paths than planners");
  const size_t n = paths.size(), D = options_.GetNumDofs();
  IkTables t;
  std::vector<size_t> planners(n);
  t.row_offsets.assign(1, 0);
  t.initial_velocity.assign(n * D, 0.0);
  callback_seconds_ = 0.0;
  for (size_t k = 0; k < n; k++) {
    TimeableCartesianSplinePath &p = *paths[k];
    planners[k] = k;
    if (p.NumDofs() != D || p.NumPathSamples() != options_.GetNumPathSamples() ||
        p.options().constraint_safety() != constraint_safety_)
      return InvalidArgumentError("path does not have the shape of the set");
    const int state = StateCode(p.GetState());
    if (state != 1 && state != 2) return FailedPreconditionError("SetWaypoints first");
    if (p.GetMaxJointVelocity().size() != D || p.GetMaxJointAcceleration().size() != D)
      return FailedPreconditionError("set the joint limits first");
    const double t0 = NowSeconds();
    if (Status st = streaming ? p.ExtendIkTable(0, (int)options_.GetNumPathSamples() - 1, &t.ik_positions, &t.jacobians)
                              : p.BuildIkTable(&t.ik_positions, &t.jacobians);
        !st.ok())
      return st;
    callback_seconds_ += NowSeconds() - t0;
    t.row_offsets.push_back((int32_t)(t.ik_positions.size() / D));
    t.path_end.push_back(p.knots().back());
    t.max_translational_velocity.push_back(p.max_translational_velocity());
    t.max_rotational_velocity.push_back(p.max_rotational_velocity());
    t.delta.push_back(p.GetPathSamplingDistance());
    t.max_velocity.insert(t.max_velocity.end(), p.GetMaxJointVelocity().begin(), p.GetMaxJointVelocity().end());
    t.max_acceleration.insert(t.max_acceleration.end(), p.GetMaxJointAcceleration().begin(),
                              p.GetMaxJointAcceleration().end());
    if (p.GetInitialVelocity().size() == D)
      std::copy(p.GetInitialVelocity().begin(), p.GetInitialVelocity().end(), t.initial_velocity.begin() + k * D);
    t.path_state.push_back(state);
  }
  const Status up = SetIkTables(planners, t);
  for (size_t k = 0; k < n && up.ok() && streaming; k++) {     // SetIkTables forgot the planners' previous sources
    stream_paths_[k] = paths[k].get();
    stream_keep_[k] = paths[k];
  }
  return up;
}

Status PathTimingTrajectorySet::SetIkTables(const std::vector<size_t> &planners, const IkTables &t) {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set takes joint spline paths (SetPaths)");
  const size_t n = planners.size(), D = options_.GetNumDofs();
  if (t.row_offsets.size() != n + 1 || t.path_end.size() != n || t.max_translational_velocity.size() != n ||
      t.max_rotational_velocity.size() != n || t.delta.size() != n || t.max_velocity.size() != n * D ||
      t.max_acceleration.size() != n * D || (!t.initial_velocity.empty() && t.initial_velocity.size() != n * D) ||
      (!t.path_state.empty() && t.path_state.size() != n))
    return InvalidArgumentError("one entry per listed planner");
  if (n == 0) return OkStatus();
  const size_t rows = t.row_offsets.back() > 0 ? (size_t)t.row_offsets.back() : 0;
  if (t.ik_positions.size() != rows * D || t.jacobians.size() != rows * 6 * D)
    return InvalidArgumentError("the tables do not hold row_offsets.back() rows");
  std::vector<int32_t> ids(n), state(t.path_state.empty() ? std::vector<int32_t>(n, 1) : t.path_state);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    ids[k] = (int32_t)planners[k];
  }
  const int rc = tpamd_planner_set_upload_ik_tables(
      set_, (int)n, ids.data(), t.row_offsets.data(), t.ik_positions.data(), t.jacobians.data(), t.path_end.data(),
      t.max_velocity.data(), t.max_acceleration.data(), t.max_translational_velocity.data(),
      t.max_rotational_velocity.data(), t.delta.data(), t.initial_velocity.empty() ? nullptr : t.initial_velocity.data(),
      state.data());
  if (rc == TPAMD_E_INVALID_ARGUMENT)
    return InvalidArgumentError("a planner listed twice, a state other than new / modified, a table shorter than the "
                                "window, delta <= 0 or row offsets that do not start at 0 and increase");
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  for (size_t k = 0; k < n; k++) {
    summary_[planners[k]].path_state = state[k];
    ForgetStreamSource(planners[k]);
  }
  return OkStatus();
}

namespace {
// Device memory of one SetCartesianWaypointPaths call: freed when the call ends.
struct DeviceArrays {
  std::vector<void *> ptrs;
  bool failed = false;
  template <typename T>
  T *take(size_t count, const T *from = nullptr) {
    void *p = nullptr;
    if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) { failed = true; return nullptr; }
    ptrs.push_back(p);
    if (from && count && hipMemcpy(p, from, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) failed = true;
    return (T *)p;
  }
  // the allocation is no longer this object's to free
  void release(void *p) { ptrs.erase(std::remove(ptrs.begin(), ptrs.end(), p), ptrs.end()); }
  ~DeviceArrays() { for (void *p : ptrs) (void)hipFree(p); }
};
}  // namespace

// The fitted splines of the planners one streaming SetCartesianWaypointPaths call loaded, packed as the
// fit left them (paths without waypoints have no slots), each planner's last resident table row and
// the caller's IK.
struct PathTimingTrajectorySet::StreamFit {
  double *knots = nullptr, *trans = nullptr, *rot = nullptr, *joint_cp = nullptr, *delta = nullptr, *last = nullptr;
  std::vector<int32_t> num_points, planner;       // [m]
  DeviceSeededIkFunc ik;
  ~StreamFit() {
    for (void *p : {(void *)knots, (void *)trans, (void *)rot, (void *)joint_cp, (void *)delta, (void *)last})
      if (p) (void)hipFree(p);
  }
};

void PathTimingTrajectorySet::ForgetStreamSource(size_t planner) {
  stream_paths_.resize(num_planners_, nullptr);
  stream_keep_.resize(num_planners_);
  stream_fits_.resize(num_planners_);
  stream_fit_index_.resize(num_planners_, -1);
  stream_paths_[planner] = nullptr;
  stream_keep_[planner] = nullptr;
  stream_fits_[planner] = nullptr;
  stream_fit_index_[planner] = -1;
}

Status PathTimingTrajectorySet::SetCartesianWaypointPaths(const std::vector<size_t> &planners,
                                                          const std::vector<std::vector<Pose3d>> &pose_waypoints,
                                                          const std::vector<std::vector<VectorXd>> &joint_waypoints,
                                                          const CartesianPathLimits &lim, const DeviceIkFunc &ik) {
  if (!ik) return WaypointPathsImpl(planners, pose_waypoints, joint_waypoints, lim, nullptr, false);
  return WaypointPathsImpl(planners, pose_waypoints, joint_waypoints, lim,
                           [&ik](const double *pose_targets, const double *joint_targets,
                                 const std::vector<int32_t> &row_offsets, const double *, double *ik_positions,
                                 double *jacobians, void *hip_stream) {
                             return ik(pose_targets, joint_targets, row_offsets, ik_positions, jacobians, hip_stream);
                           },
                           false);
}

Status PathTimingTrajectorySet::SetCartesianWaypointPaths(const std::vector<size_t> &planners,
                                                          const std::vector<std::vector<Pose3d>> &pose_waypoints,
                                                          const std::vector<std::vector<VectorXd>> &joint_waypoints,
                                                          const CartesianPathLimits &lim, const DeviceSeededIkFunc &ik,
                                                          bool streaming) {
  return WaypointPathsImpl(planners, pose_waypoints, joint_waypoints, lim, ik, streaming);
}

Status PathTimingTrajectorySet::WaypointPathsImpl(const std::vector<size_t> &planners,
                                                  const std::vector<std::vector<Pose3d>> &pose_waypoints,
                                                  const std::vector<std::vector<VectorXd>> &joint_waypoints,
                                                  const CartesianPathLimits &lim, const DeviceSeededIkFunc &ik,
                                                  bool streaming) {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set takes joint spline paths (SetWaypointPaths)");
  const size_t n = planners.size(), D = options_.GetNumDofs(), N = options_.GetNumPathSamples();
  if (!ik) return InvalidArgumentError("no IK function");
  if (pose_waypoints.size() != n || joint_waypoints.size() != n || lim.max_velocity.size() != n ||
      lim.max_acceleration.size() != n || lim.max_translational_velocity.size() != n ||
      lim.max_rotational_velocity.size() != n || (!lim.initial_velocity.empty() && lim.initial_velocity.size() != n))
    return InvalidArgumentError("one waypoint list and one set of limits per listed planner");
  if (!(lim.delta_parameter > 0.0)) return InvalidArgumentError("delta_parameter must be positive");
  std::vector<char> seen(num_planners_, 0);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_ || seen[planners[k]]) return InvalidArgumentError("no such planner, or listed twice");
    seen[planners[k]] = 1;
    if (lim.max_velocity[k].size() != D || lim.max_acceleration[k].size() != D ||
        (!lim.initial_velocity.empty() && lim.initial_velocity[k].size() != D))
      return InvalidArgumentError("a limit or an initial velocity of the wrong dimension");
  }
  if (n == 0) return OkStatus();
  // the waypoints, packed; a planner whose lists do not fit goes to the device without waypoints
  std::vector<int32_t> offsets(n + 1, 0);
  std::vector<double> pose, joint;
  for (size_t k = 0; k < n; k++) {
    bool ok = pose_waypoints[k].size() == joint_waypoints[k].size();
    for (const VectorXd &w : joint_waypoints[k]) ok = ok && w.size() == D;
    if (ok) {
      for (const Pose3d &p : pose_waypoints[k]) {
        const Quaterniond &q = p.quaternion();
        const double row[7] = {p.translation()[0], p.translation()[1], p.translation()[2], q.w, q.x, q.y, q.z};
        pose.insert(pose.end(), row, row + 7);
      }
      for (const VectorXd &w : joint_waypoints[k]) joint.insert(joint.end(), w.begin(), w.end());
    }
    offsets[k + 1] = offsets[k] + (ok ? (int32_t)pose_waypoints[k].size() : 0);
  }
  int previous = 0;
  if (hipGetDevice(&previous) != hipSuccess || hipSetDevice(lease_.device()) != hipSuccess)
    return InternalError("no HIP device");
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{previous};
  hipStream_t st = nullptr;
  DeviceArrays mem;
  // 1. the fit
  size_t points = 0, knots = 0;
  for (size_t k = 0; k < n; k++) {
    const size_t W = (size_t)(offsets[k + 1] - offsets[k]);
    const size_t P = W < 1 ? 0 : (W == 1 ? 4 : 3 * W - 2);
    points += P;
    knots += P ? P + 3 : 0;
  }
  const std::vector<double> tr(n, lim.translation_rounding), rr(n, lim.rotation_rounding);
  double *d_pose = mem.take<double>(pose.size(), pose.data()), *d_joint = mem.take<double>(joint.size(), joint.data());
  double *d_tr = mem.take<double>(n, tr.data()), *d_rr = mem.take<double>(n, rr.data());
  double *d_knots = mem.take<double>(knots), *d_t = mem.take<double>(points * 3), *d_r = mem.take<double>(points * 4);
  double *d_j = mem.take<double>(points * D), *d_end = mem.take<double>(n);
  int32_t *d_np = mem.take<int32_t>(n), *d_st = mem.take<int32_t>(n);
  if (mem.failed) return InternalError("device memory for the fit");
  std::vector<int32_t> point_offsets(n + 1, 0), fit_status(n, 0);
  std::vector<double> path_end(n, 0.0);
  int rc = tpamd_fit_pose_waypoints_device(lease_.get(), (int)n, (int)D, offsets.data(), d_pose, d_joint, d_tr, d_rr,
                                           d_knots, d_t, d_r, d_j, d_np, point_offsets.data(), d_end, d_st, st);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  // 2. path_end and the statuses come down (n values each)
  if (hipMemcpy(path_end.data(), d_end, n * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess ||
      hipMemcpy(fit_status.data(), d_st, n * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess)
    return InternalError("reading the fit's results");
  // 3. the rows of every fitted planner; a planner without waypoints has no slots in the spline arrays
  std::vector<int32_t> ids, num_points, row_offsets(1, 0), state;
  std::vector<double> end_ok, vmax, amax, iv, vt, vr;
  Status first_bad = OkStatus();
  for (size_t k = 0; k < n; k++) {
    if (fit_status[k] != TPAMD_PLAN_OK) {
      if (first_bad.ok())
        first_bad = InvalidArgumentError("planner " + std::to_string(planners[k]) +
                                         ": no waypoints, or pose and joint waypoints that do not match");
      continue;
    }
    // streaming: the first window's rows only, as the path's first SamplePath solves them
    const int rows = streaming ? (int)N : tpamd_ik_table_rows(path_end[k], lim.delta_parameter, (int)N);
    if (rows < 0) return InternalError("tpamd_ik_table_rows");
    ids.push_back((int32_t)planners[k]);
    num_points.push_back(point_offsets[k + 1] - point_offsets[k]);
    row_offsets.push_back(row_offsets.back() + rows);
    end_ok.push_back(path_end[k]);
    vmax.insert(vmax.end(), lim.max_velocity[k].begin(), lim.max_velocity[k].end());
    amax.insert(amax.end(), lim.max_acceleration[k].begin(), lim.max_acceleration[k].end());
    if (!lim.initial_velocity.empty()) iv.insert(iv.end(), lim.initial_velocity[k].begin(), lim.initial_velocity[k].end());
    vt.push_back(lim.max_translational_velocity[k]);
    vr.push_back(lim.max_rotational_velocity[k]);
    state.push_back(1);                 // kNewPath
  }
  const size_t m = ids.size(), rows = (size_t)row_offsets.back();
  if (m == 0) return first_bad;
  const std::vector<double> dl(m, lim.delta_parameter);
  double *d_dl = mem.take<double>(m, dl.data()), *d_end_ok = mem.take<double>(m, end_ok.data());
  double *d_vmax = mem.take<double>(m * D, vmax.data()), *d_amax = mem.take<double>(m * D, amax.data());
  double *d_iv = iv.empty() ? nullptr : mem.take<double>(m * D, iv.data());
  double *d_vt = mem.take<double>(m, vt.data()), *d_vr = mem.take<double>(m, vr.data());
  int32_t *d_state = mem.take<int32_t>(m, state.data());
  double *d_pose_t = mem.take<double>(rows * 7), *d_joint_t = mem.take<double>(rows * D);
  double *d_q = mem.take<double>(rows * D), *d_J = mem.take<double>(rows * 6 * D);
  if (mem.failed) return InternalError("device memory for the targets and the tables");
  // 4. the targets, 5. the caller's IK, 6. the tables
  rc = tpamd_sample_ik_targets_device(lease_.get(), (int)m, (int)D, num_points.data(), row_offsets.data(), d_knots, d_t,
                                      d_r, d_j, d_dl, d_pose_t, d_joint_t, st);
  if (rc != 0) {
    (void)hipDeviceSynchronize();
    return InternalError(tpamd_error_string(rc));
  }
  const Status ik_status = ik(d_pose_t, d_joint_t, row_offsets, nullptr, d_q, d_J, st);
  if (!ik_status.ok()) {
    (void)hipDeviceSynchronize();
    return ik_status;
  }
  std::shared_ptr<StreamFit> fit;
  if (streaming) {
    // the splines stay; every planner's last resident row is the seed of its first extension
    fit = std::make_shared<StreamFit>();
    fit->num_points = num_points;
    fit->planner = ids;
    fit->ik = ik;
    bool ok = hipMalloc((void **)&fit->last, m * D * sizeof(double)) == hipSuccess &&
              hipMalloc((void **)&fit->delta, m * sizeof(double)) == hipSuccess &&
              hipMemcpyAsync(fit->delta, d_dl, m * sizeof(double), hipMemcpyDeviceToDevice, st) == hipSuccess;
    for (size_t k = 0; k < m && ok; k++)
      ok = hipMemcpyAsync(fit->last + k * D, d_q + ((size_t)row_offsets[k + 1] - 1) * D, D * sizeof(double),
                          hipMemcpyDeviceToDevice, st) == hipSuccess;
    if (!ok) {
      (void)hipDeviceSynchronize();
      return InternalError("device memory for the resident splines");
    }
  }
  rc = tpamd_planner_set_upload_ik_tables_device(set_, (int)m, ids.data(), row_offsets.data(), d_q, d_J, d_end_ok, d_vmax,
                                                 d_amax, d_vt, d_vr, d_dl, d_iv, d_state, st);
  if (hipDeviceSynchronize() != hipSuccess) return InternalError("the device chain failed");   // before mem goes
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  for (size_t k = 0; k < m; k++) {
    summary_[ids[k]].path_state = 1;
    ForgetStreamSource((size_t)ids[k]);
    if (fit) {
      stream_fits_[ids[k]] = fit;
      stream_fit_index_[ids[k]] = (int)k;
    }
  }
  if (fit) {
    for (double *p : {d_knots, d_t, d_r, d_j}) mem.release(p);
    fit->knots = d_knots; fit->trans = d_t; fit->rot = d_r; fit->joint_cp = d_j;
  }
  return first_bad;
}

// One round of extensions through the device chain: every waiting planner whose path came from a
// streaming SetCartesianWaypointPaths call gets the rows it lacks. A fit's paths are sampled in place
// (the planners that do not wait take no rows), so nothing is repacked.
Status PathTimingTrajectorySet::ExtendOnDevice(const std::vector<int32_t> &need_first,
                                               const std::vector<int32_t> &need_count, std::vector<Status> *failed) {
  const size_t D = options_.GetNumDofs();
  std::vector<std::shared_ptr<StreamFit>> fits;
  for (size_t b = 0; b < num_planners_; b++)
    if (need_count[b] > 0 && (*failed)[b].ok() && b < stream_fits_.size() && stream_fits_[b] &&
        std::find(fits.begin(), fits.end(), stream_fits_[b]) == fits.end())
      fits.push_back(stream_fits_[b]);
  if (fits.empty()) return OkStatus();
  int previous = 0;
  if (hipGetDevice(&previous) != hipSuccess || hipSetDevice(lease_.device()) != hipSuccess)
    return InternalError("no HIP device");
  struct Restore { int d; ~Restore() { (void)hipSetDevice(d); } } restore{previous};
  hipStream_t st = nullptr;
  for (const std::shared_ptr<StreamFit> &fit : fits) {
    const size_t m = fit->planner.size();
    std::vector<int32_t> rows_of(m + 1, 0), first_row(m, 0), ids, run(1, 0), kept(1, 0);
    std::vector<size_t> which;
    for (size_t k = 0; k < m; k++) {
      const size_t b = (size_t)fit->planner[k];
      const bool waits = stream_fits_[b] == fit && stream_fit_index_[b] == (int)k && need_count[b] > 0 && (*failed)[b].ok();
      rows_of[k + 1] = rows_of[k] + (waits ? need_count[b] + 1 : 0);     // the last resident row once more, then the new rows
      if (!waits) continue;
      first_row[k] = need_first[b] - 1;
      ids.push_back((int32_t)b);
      which.push_back(k);
      run.push_back(rows_of[k + 1]);
      kept.push_back(kept.back() + need_count[b]);
    }
    const size_t w = ids.size(), rows = (size_t)rows_of[m], keep = (size_t)kept.back();
    if (w == 0) continue;
    DeviceArrays mem;
    double *d_pose_t = mem.take<double>(rows * 7), *d_joint_t = mem.take<double>(rows * D);
    double *d_q = mem.take<double>(rows * D), *d_J = mem.take<double>(rows * 6 * D), *d_seed = mem.take<double>(w * D);
    double *d_q2 = mem.take<double>(keep * D), *d_J2 = mem.take<double>(keep * 6 * D);
    Status bad = mem.failed ? InternalError("device memory for the new rows") : OkStatus();
    int rc = 0;
    if (bad.ok()) {
      rc = tpamd_sample_ik_target_rows_device(lease_.get(), (int)m, (int)D, fit->num_points.data(), rows_of.data(),
                                              first_row.data(), fit->knots, fit->trans, fit->rot, fit->joint_cp, fit->delta,
                                              d_pose_t, d_joint_t, st);
      if (rc != 0) bad = InternalError(tpamd_error_string(rc));
    }
    for (size_t k = 0; k < w && bad.ok(); k++)
      if (hipMemcpyAsync(d_seed + k * D, fit->last + which[k] * D, D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        bad = InternalError("copying the seed rows");
    if (bad.ok()) bad = fit->ik(d_pose_t, d_joint_t, run, d_seed, d_q, d_J, st);
    for (size_t k = 0; k < w && bad.ok(); k++) {
      // without the re-evaluated first row; the run's last row is the next seed
      const size_t from = (size_t)run[k] + 1, n = (size_t)(kept[k + 1] - kept[k]);
      if (hipMemcpyAsync(d_q2 + (size_t)kept[k] * D, d_q + from * D, n * D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(d_J2 + (size_t)kept[k] * 6 * D, d_J + from * 6 * D, n * 6 * D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess ||
          hipMemcpyAsync(fit->last + which[k] * D, d_q + ((size_t)run[k + 1] - 1) * D, D * sizeof(double), hipMemcpyDeviceToDevice, st) != hipSuccess)
        bad = InternalError("packing the new rows");
    }
    if (bad.ok()) {
      rc = tpamd_planner_set_append_ik_rows_device(set_, (int)w, ids.data(), kept.data(), d_q2, d_J2, st);
      if (rc != 0) bad = InternalError(tpamd_error_string(rc));
    }
    if (hipDeviceSynchronize() != hipSuccess && bad.ok()) bad = InternalError("the device chain failed");   // before mem goes
    if (!bad.ok())
      for (int32_t b : ids) (*failed)[b] = bad;
    else
      suspensions_ += (int)w;
  }
  return OkStatus();
}

int PathTimingTrajectorySet::GetIkTableRows(size_t planner) const {
  int32_t rows = 0;
  if (!init_status_.ok() || !cartesian_ || planner >= num_planners_ ||
      tpamd_planner_set_ik_table_info(set_, (int)planner, nullptr, &rows, nullptr) != 0)
    return -1;
  return rows;                // the path rows supplied so far, whether the front ones are still resident or not
}

Status PathTimingTrajectorySet::GetIkTable(size_t planner, std::vector<double> *ik_positions,
                                           std::vector<double> *jacobians) const {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set has no IK tables (GetPath)");
  if (planner >= num_planners_) return InvalidArgumentError("no such planner");
  int32_t rows = 0;
  int rc = tpamd_planner_set_download_ik_table(set_, (int)planner, &rows, nullptr, nullptr, 0);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  const size_t D = options_.GetNumDofs();
  ik_positions->assign((size_t)rows * D, 0.0);
  jacobians->assign((size_t)rows * 6 * D, 0.0);
  if (rows == 0) return OkStatus();
  rc = tpamd_planner_set_download_ik_table(set_, (int)planner, &rows, ik_positions->data(), jacobians->data(), rows);
  return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc));
}

Status PathTimingTrajectorySet::SetPaths(const std::vector<std::shared_ptr<TimeableJointSplinePath>> &paths) {
  if (!init_status_.ok()) return init_status_;
  if (cartesian_) return FailedPreconditionError("a Cartesian set takes IK tables (SetCartesianPaths)");
  if (paths.size() > num_planners_) return InvalidArgumentError("more paths than planners");
  const size_t n = paths.size(), D = options_.GetNumDofs();
  std::vector<double> knots, cps, vmax(n * D), amax(n * D), dl(n), iv(n * D);
  std::vector<int32_t> st(n), np(n);
  for (size_t k = 0; k < n; k++) {
    const TimeableJointSplinePath &p = *paths[k];
    if (p.NumDofs() != D || p.NumPathSamples() != options_.GetNumPathSamples() ||
        p.options().constraint_safety() != constraint_safety_)
      return InvalidArgumentError("path does not have the shape of the set");
    st[k] = StateCode(p.GetState());
    if (st[k] != 1 && st[k] != 2) return FailedPreconditionError("SetWaypoints / SwitchToWaypointPath first");
    np[k] = p.num_control_points();
    if (np[k] < 3) return FailedPreconditionError("SetWaypoints / SwitchToWaypointPath first");
    knots.insert(knots.end(), p.knots().begin(), p.knots().end());       // packed back to back
    cps.insert(cps.end(), p.packed_control_points().begin(), p.packed_control_points().end());
    for (size_t d = 0; d < D; d++) {
      vmax[k * D + d] = p.GetMaxJointVelocity()[d];
      amax[k * D + d] = p.GetMaxJointAcceleration()[d];
      iv[k * D + d] = p.GetInitialVelocity()[d];
    }
    dl[k] = p.GetPathSamplingDistance();
  }
  const int rc = tpamd_planner_set_upload_paths_ragged(set_, (int)n, nullptr, np.data(), knots.data(), cps.data(),
                                                       vmax.data(), amax.data(), dl.data(), iv.data(), st.data());
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  for (size_t k = 0; k < n; k++) summary_[k].path_state = st[k];
  return OkStatus();
}

void PathTimingTrajectorySet::Reset(size_t planner) {
  if (!set_ || planner >= num_planners_) return;
  const int32_t id = (int32_t)planner;
  tpamd_planner_set_reset(set_, 1, &id);
  summary_[planner] = tpamd_planner_summary{};
}

std::vector<Status> PathTimingTrajectorySet::Plan(Time start, Duration time_horizon) {
  return Plan(std::vector<Time>(num_planners_, start), std::vector<Duration>(num_planners_, time_horizon));
}

std::vector<Status> PathTimingTrajectorySet::Plan(const std::vector<Time> &start,
                                                  const std::vector<Duration> &time_horizon) {
  std::vector<Status> result(num_planners_, OkStatus());
  if (!init_status_.ok() || start.size() != num_planners_ || time_horizon.size() != num_planners_) {
    const Status st = init_status_.ok() ? InvalidArgumentError("one start time and horizon per planner") : init_status_;
    std::fill(result.begin(), result.end(), st);
    return result;
  }
  std::vector<int64_t> s(num_planners_), h(num_planners_);
  for (size_t b = 0; b < num_planners_; b++) {
    s[b] = ::tpamd::compat::ToUnixNanos(start[b]);
    h[b] = time_horizon[b].nanos();
  }
  const int rc = tpamd_planner_set_plan(set_, s.data(), h.data(), summary_.data());
  if (rc != 0) {
    std::fill(result.begin(), result.end(), InternalError(tpamd_error_string(rc)));
    return result;
  }
  return PlanStatuses();
}

Status PathTimingTrajectorySet::Reserve(int history, int trajectory) {
  if (!init_status_.ok()) return init_status_;
  if (plan_pending_) return FailedPreconditionError("a PlanDevice call is in flight (FinishPlanDevice)");
  const int rc = tpamd_planner_set_reserve(set_, history, trajectory);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  if (!plan_results_ &&
      hipMalloc(&plan_results_, num_planners_ * sizeof(tpamd_planner_summary) + sizeof(tpamd_plan_device_info)) != hipSuccess)
    return InternalError("no device memory for the summaries");
  return OkStatus();
}

Status PathTimingTrajectorySet::GetCapacity(int *history, int *trajectory) const {
  if (!init_status_.ok()) return init_status_;
  int32_t h = 0, t = 0;
  const int rc = tpamd_planner_set_capacity(set_, &h, &t);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  if (history) *history = h;
  if (trajectory) *trajectory = t;
  return OkStatus();
}

Status PathTimingTrajectorySet::PlanDevice(const int64_t *start_ns_dev, const int64_t *horizon_ns_dev, int max_windows,
                                           void *hip_stream) {
  if (!init_status_.ok()) return init_status_;
  if (plan_pending_) return FailedPreconditionError("a PlanDevice call is in flight (FinishPlanDevice)");
  if (!start_ns_dev || !horizon_ns_dev || max_windows < 1)
    return InvalidArgumentError("device arrays of start times and horizons, max_windows >= 1");
  if (!plan_results_) {        // not reserved: the buffer for the summaries and the info is made here
    const Status st = Reserve(0, 0);
    if (!st.ok()) return st;
  }
  auto *summary = (tpamd_planner_summary *)plan_results_;
  auto *info = (tpamd_plan_device_info *)(summary + num_planners_);
  const int rc = tpamd_planner_set_plan_device(set_, start_ns_dev, horizon_ns_dev, max_windows, summary, info, hip_stream);
  if (rc == TPAMD_E_INVALID_ARGUMENT) return InvalidArgumentError(tpamd_error_string(rc));
  // any other error may have left work enqueued: FinishPlanDevice still waits for it
  plan_pending_ = true;
  plan_stream_ = hip_stream;
  return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc));
}

std::vector<Status> PathTimingTrajectorySet::FinishPlanDevice() {
  std::vector<Status> result(num_planners_, OkStatus());
  if (!init_status_.ok() || !plan_pending_) {
    std::fill(result.begin(), result.end(),
              init_status_.ok() ? FailedPreconditionError("no PlanDevice call is in flight") : init_status_);
    return result;
  }
  plan_pending_ = false;
  const size_t bytes = num_planners_ * sizeof(tpamd_planner_summary);
  hipStream_t st = (hipStream_t)plan_stream_;
  if (hipMemcpyAsync(summary_.data(), plan_results_, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(&plan_info_, (const char *)plan_results_ + bytes, sizeof(plan_info_), hipMemcpyDeviceToHost, st) !=
          hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    std::fill(result.begin(), result.end(), InternalError("could not read the summaries back"));
    return result;
  }
  return PlanStatuses();
}

std::vector<Status> PathTimingTrajectorySet::PlanStatuses() const {
  std::vector<Status> result(num_planners_, OkStatus());
  for (size_t b = 0; b < num_planners_; b++) {
    switch (summary_[b].status) {
      case TPAMD_PLAN_OK: break;
      case TPAMD_PLAN_FAILED_PRECONDITION: result[b] = FailedPreconditionError("No path set / nothing to connect to."); break;
      case TPAMD_PLAN_OUT_OF_RANGE: result[b] = OutOfRangeError("start outside the previous plan"); break;
      case TPAMD_PLAN_INVALID_ARGUMENT:
        result[b] = InvalidArgumentError("start time / duration / initial velocity not acceptable"); break;
      case TPAMD_PLAN_DEADLINE_EXCEEDED: result[b] = DeadlineExceededError("Reached maximum number of planning loops"); break;
      case TPAMD_PLAN_NEEDS_ROWS: result[b] = InternalError("IK solution does not cover the sampled window"); break;
      case TPAMD_PLAN_RESOURCE_EXHAUSTED:
        result[b] = ::tpamd::compat::ResourceExhaustedError("history or trajectory capacity exhausted (Reserve, Reset, new path)"); break;
      default: result[b] = InternalError("Error optimizing path parameter"); break;
    }
  }
  return result;
}

std::vector<Status> PathTimingTrajectorySet::PlanStreaming(Time start, Duration time_horizon, bool discard) {
  return PlanStreaming(std::vector<Time>(num_planners_, start), std::vector<Duration>(num_planners_, time_horizon),
                       discard);
}

StatusOr<std::vector<int32_t>> PathTimingTrajectorySet::DiscardIkRows() {
  if (!init_status_.ok()) return init_status_;
  if (!cartesian_) return FailedPreconditionError("a joint set has no IK tables (DiscardIkRows)");
  std::vector<int32_t> first(num_planners_, 0), ids, out;
  for (size_t b = 0; b < num_planners_; b++) {
    int32_t rows = 0;
    if (tpamd_planner_set_ik_table_info(set_, (int)b, nullptr, &rows, nullptr) == 0 && rows > 0) ids.push_back((int32_t)b);
  }
  out.resize(ids.size());
  const int rc = tpamd_planner_set_discard_ik_rows(set_, (int)ids.size(), ids.data(), nullptr, out.data());
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  for (size_t k = 0; k < ids.size(); k++) first[ids[k]] = out[k];
  return first;
}

Status PathTimingTrajectorySet::GetIkTableInfo(size_t planner, int32_t *first_row, int32_t *rows,
                                               int32_t *capacity) const {
  if (!init_status_.ok()) return init_status_;
  if (planner >= num_planners_) return InvalidArgumentError("no such planner");
  const int rc = tpamd_planner_set_ik_table_info(set_, (int)planner, first_row, rows, capacity);
  return rc == 0 ? OkStatus() : FailedPreconditionError("a joint set has no IK tables");
}

std::vector<Status> PathTimingTrajectorySet::PlanStreaming(const std::vector<Time> &start,
                                                           const std::vector<Duration> &time_horizon, bool discard) {
  std::vector<Status> result(num_planners_, OkStatus());
  Status bad = init_status_;
  if (bad.ok() && !cartesian_) bad = FailedPreconditionError("a joint set has no IK tables (Plan)");
  if (bad.ok() && (start.size() != num_planners_ || time_horizon.size() != num_planners_))
    bad = InvalidArgumentError("one start time and horizon per planner");
  if (!bad.ok()) {
    std::fill(result.begin(), result.end(), bad);
    return result;
  }
  std::vector<int64_t> s(num_planners_), h(num_planners_);
  for (size_t b = 0; b < num_planners_; b++) {
    s[b] = ::tpamd::compat::ToUnixNanos(start[b]);
    h[b] = time_horizon[b].nanos();
  }
  std::vector<int32_t> need_first(num_planners_), need_count(num_planners_);
  int32_t waiting = 0;
  suspensions_ = 0;
  int rc = tpamd_planner_set_plan_streaming(set_, s.data(), h.data(), summary_.data(), need_first.data(),
                                            need_count.data(), &waiting);
  std::vector<Status> ik_failed(num_planners_, OkStatus());
  callback_seconds_ = 0.0;
  const size_t D = options_.GetNumDofs();
  while (rc == 0 && waiting > 0) {
    // host route: every waiting planner's path extends its IK solution as SamplePath would for that
    // window. A planner whose IK failed is not asked again: it keeps waiting, and the next Plan drops
    // it, as after a failed SamplePath.
    std::vector<int32_t> ids, offsets(1, 0);
    std::vector<double> q, J;
    for (size_t b = 0; b < num_planners_; b++) {
      if (need_count[b] <= 0 || !ik_failed[b].ok()) continue;
      if (b < stream_fits_.size() && stream_fits_[b]) continue;                  // device route below
      TimeableCartesianSplinePath *path = b < stream_paths_.size() ? stream_paths_[b] : nullptr;
      const double t0 = NowSeconds();
      const Status st = path ? path->ExtendIkTable(need_first[b], need_first[b] + need_count[b] - 1, &q, &J)
                             : InternalError("IK solution does not cover the sampled window");
      callback_seconds_ += NowSeconds() - t0;
      if (!st.ok()) {
        ik_failed[b] = st;
        q.resize((size_t)offsets.back() * D);
        J.resize((size_t)offsets.back() * 6 * D);
        continue;
      }
      ids.push_back((int32_t)b);
      offsets.push_back((int32_t)(q.size() / D));
    }
    if (!ids.empty()) {
      suspensions_ += (int)ids.size();
      rc = tpamd_planner_set_append_ik_rows(set_, (int)ids.size(), ids.data(), offsets.data(), q.data(), J.data());
    }
    // device route
    if (rc == 0)
      if (const Status st = ExtendOnDevice(need_first, need_count, &ik_failed); !st.ok()) {
        std::fill(result.begin(), result.end(), st);
        return result;
      }
    bool progress = false;
    for (size_t b = 0; b < num_planners_; b++) progress = progress || (need_count[b] > 0 && ik_failed[b].ok());
    if (!progress) break;
    if (rc == 0) rc = tpamd_planner_set_plan_resume(set_, summary_.data(), need_first.data(), need_count.data(), &waiting);
  }
  if (rc != 0) {
    std::fill(result.begin(), result.end(), InternalError(tpamd_error_string(rc)));
    return result;
  }
  result = PlanStatuses();
  for (size_t b = 0; b < num_planners_; b++)
    if (!ik_failed[b].ok()) result[b] = ik_failed[b];
  if (discard && waiting == 0) {            // a completed call: nobody waits for rows
    const StatusOr<std::vector<int32_t>> first = DiscardIkRows();
    if (!first.ok()) std::fill(result.begin(), result.end(), first.status());
  }
  return result;
}

namespace {
StatusOr<double> StopResult(int32_t status, double stop_parameter, int64_t time_ns) {
  if (status == TPAMD_PLAN_OK) return stop_parameter;
  if (status == TPAMD_PLAN_INVALID_ARGUMENT) {      // path_timing_trajectory.cc:245-249
    char msg[96];
    std::snprintf(msg, sizeof msg, "Time %g not in timed path range", (double)time_ns / 1e9);
    return InvalidArgumentError(msg);
  }
  return InternalError("stop parameter query failed");
}
}  // namespace

StatusOr<double> PathTimingTrajectorySet::GetPathStopParameter(size_t planner, Time time) const {
  if (!init_status_.ok()) return init_status_;
  if (planner >= num_planners_) return InvalidArgumentError("no such planner");
  const int32_t id = (int32_t)planner;
  const int64_t t = ::tpamd::compat::ToUnixNanos(time);
  double s = 0.0;
  int32_t st = 0;
  const int rc = tpamd_planner_set_stop_parameters(set_, 1, &id, &t, &s, nullptr, &st);
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  return StopResult(st, s, t);
}

std::vector<StatusOr<double>> PathTimingTrajectorySet::GetPathStopParameters(const std::vector<Time> &time) const {
  if (!init_status_.ok() || time.size() != num_planners_) {
    const Status st = init_status_.ok() ? InvalidArgumentError("one time per planner") : init_status_;
    return std::vector<StatusOr<double>>(num_planners_, st);
  }
  const size_t n = num_planners_;
  std::vector<int64_t> t(n);
  for (size_t b = 0; b < n; b++) t[b] = ::tpamd::compat::ToUnixNanos(time[b]);
  std::vector<double> s(n);
  std::vector<int32_t> st(n);
  const int rc = tpamd_planner_set_stop_parameters(set_, (int)n, nullptr, t.data(), s.data(), nullptr, st.data());
  if (rc != 0) return std::vector<StatusOr<double>>(n, InternalError(tpamd_error_string(rc)));
  std::vector<StatusOr<double>> out;
  out.reserve(n);
  for (size_t b = 0; b < n; b++) out.push_back(StopResult(st[b], s[b], t[b]));
  return out;
}

std::vector<Status> PathTimingTrajectorySet::SwitchToWaypointPaths(const std::vector<size_t> &planners,
                                                                  const std::vector<Time> &time,
                                                                  const std::vector<std::vector<VectorXd>> &waypoints) {
  return SwitchToWaypointPaths(planners, time, waypoints, 0.2);      // the PathOptions default
}

std::vector<Status> PathTimingTrajectorySet::SwitchToWaypointPaths(const std::vector<size_t> &planners,
                                                                  const std::vector<Time> &time,
                                                                  const std::vector<std::vector<VectorXd>> &waypoints,
                                                                  double rounding) {
  const size_t n = planners.size(), D = options_.GetNumDofs();
  if (!init_status_.ok()) return std::vector<Status>(n, init_status_);
  if (cartesian_) return std::vector<Status>(n, FailedPreconditionError("a Cartesian set has no joint spline to switch"));
  if (time.size() != n || waypoints.size() != n)
    return std::vector<Status>(n, InvalidArgumentError("one time and one waypoint list per planner"));
  std::vector<int32_t> ids(n), offsets(n + 1, 0), np(n), st(n);
  std::vector<int64_t> t(n);
  std::vector<double> wps, stop(n);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return std::vector<Status>(n, InvalidArgumentError("no such planner"));
    ids[k] = (int32_t)planners[k];
    t[k] = ::tpamd::compat::ToUnixNanos(time[k]);
    for (const VectorXd &w : waypoints[k]) {
      if (w.size() != D) return std::vector<Status>(n, InvalidArgumentError("waypoint has the wrong dimension"));
      wps.insert(wps.end(), w.begin(), w.end());
    }
    offsets[k + 1] = offsets[k] + (int32_t)waypoints[k].size();
  }
  if (wps.empty()) wps.push_back(0.0);      // the entry takes a non-NULL array even without rows
  const int rc = tpamd_planner_set_switch_paths_rounded(set_, (int)n, ids.data(), t.data(), nullptr, offsets.data(),
                                                        wps.data(), rounding, stop.data(), np.data(), st.data());
  if (rc != 0) return std::vector<Status>(n, rc == TPAMD_E_INVALID_ARGUMENT ? InvalidArgumentError(tpamd_error_string(rc))
                                                                           : InternalError(tpamd_error_string(rc)));
  std::vector<Status> result(n, OkStatus());
  for (size_t k = 0; k < n; k++) {
    switch (st[k]) {
      case TPAMD_PLAN_OK: summary_[planners[k]].path_state = 2; break;     // kModifiedPath
      case TPAMD_PLAN_FAILED_PRECONDITION: result[k] = FailedPreconditionError("no path or no plan to switch from"); break;
      case TPAMD_PLAN_OUT_OF_RANGE: result[k] = OutOfRangeError("switch time or parameter outside the path"); break;
      case TPAMD_PLAN_INVALID_ARGUMENT: result[k] = InvalidArgumentError("Time not in timed path range / no waypoints left"); break;
      default: result[k] = InternalError("path switch failed"); break;
    }
  }
  return result;
}

std::vector<Status> PathTimingTrajectorySet::SetWaypointPaths(const std::vector<size_t> &planners,
                                                             const std::vector<std::vector<VectorXd>> &waypoints,
                                                             const std::vector<VectorXd> &max_velocity,
                                                             const std::vector<VectorXd> &max_acceleration,
                                                             const std::vector<VectorXd> &initial_velocity,
                                                             double rounding, double delta_parameter) {
  const size_t n = planners.size(), D = options_.GetNumDofs();
  if (!init_status_.ok()) return std::vector<Status>(n, init_status_);
  if (cartesian_) return std::vector<Status>(n, FailedPreconditionError("a Cartesian set takes IK tables"));
  if (waypoints.size() != n || max_velocity.size() != n || max_acceleration.size() != n ||
      (!initial_velocity.empty() && initial_velocity.size() != n))
    return std::vector<Status>(n, InvalidArgumentError("one waypoint list and one set of limits per planner"));
  std::vector<int32_t> ids(n), offsets(n + 1, 0), np(n), st(n);
  std::vector<double> wps, vmax(n * D, 0.0), amax(n * D, 0.0), iv(n * D, 0.0), dl(n, delta_parameter);
  std::vector<Status> result(n, OkStatus());
  std::vector<char> seen(num_planners_, 0);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_ || seen[planners[k]])
      return std::vector<Status>(n, InvalidArgumentError("no such planner, or listed twice"));
    seen[planners[k]] = 1;
    ids[k] = (int32_t)planners[k];
    // SetWaypoints' dimension check, then the limits' and the initial velocity's: a planner that
    // fails one of them goes to the device without waypoints (it keeps its state)
    bool ok = true;
    for (const VectorXd &w : waypoints[k])
      if (w.size() != D) ok = false;
    if (!ok) result[k] = InvalidArgumentError("waypoint has the wrong dimension");
    if (ok && (max_velocity[k].size() != D || max_acceleration[k].size() != D)) {
      result[k] = InvalidArgumentError("max_velocity / max_acceleration has the wrong dimension");
      ok = false;
    }
    if (ok && !initial_velocity.empty() && initial_velocity[k].size() != D) {
      result[k] = InvalidArgumentError("Velocity dimension doesn't match number of dofs.");
      ok = false;
    }
    if (ok) {
      for (const VectorXd &w : waypoints[k]) wps.insert(wps.end(), w.begin(), w.end());
      for (size_t d = 0; d < D; d++) {
        vmax[k * D + d] = max_velocity[k][d];
        amax[k * D + d] = max_acceleration[k][d];
        if (!initial_velocity.empty()) iv[k * D + d] = initial_velocity[k][d];
      }
    }
    offsets[k + 1] = offsets[k] + (ok ? (int32_t)waypoints[k].size() : 0);
  }
  if (n == 0) return result;
  const int rc = tpamd_planner_set_set_waypoints(set_, (int)n, ids.data(), offsets.data(), wps.data(), rounding,
                                                 vmax.data(), amax.data(), dl.data(), iv.data(), np.data(), st.data());
  if (rc != 0) return std::vector<Status>(n, rc == TPAMD_E_INVALID_ARGUMENT ? InvalidArgumentError(tpamd_error_string(rc))
                                                                           : InternalError(tpamd_error_string(rc)));
  for (size_t k = 0; k < n; k++) {
    if (!result[k].ok()) continue;
    if (st[k] == TPAMD_PLAN_OK) summary_[planners[k]].path_state = 1;      // kNewPath
    else result[k] = InvalidArgumentError("Control point vector empty.");
  }
  return result;
}

std::vector<Status> PathTimingTrajectorySet::RetargetWaypointPaths(
    const std::vector<size_t> &planners, const std::vector<Time> &time, const std::vector<std::vector<VectorXd>> &waypoints,
    const std::vector<VectorXd> &max_velocity, const std::vector<VectorXd> &max_acceleration, double rounding,
    double delta_parameter, const std::vector<VectorXd> &stopping_acceleration) {
  const size_t n = planners.size(), D = options_.GetNumDofs();
  if (!init_status_.ok()) return std::vector<Status>(n, init_status_);
  if (cartesian_) return std::vector<Status>(n, FailedPreconditionError("a Cartesian set takes IK tables"));
  if (time.size() != n || waypoints.size() != n || max_velocity.size() != n || max_acceleration.size() != n ||
      (!stopping_acceleration.empty() && stopping_acceleration.size() != n))
    return std::vector<Status>(n, InvalidArgumentError("one time, one waypoint list and one set of limits per planner"));
  std::vector<int32_t> ids(n), offsets(n + 1, 0), np(n), st(n);
  std::vector<int64_t> t(n);
  std::vector<double> wps, vmax(n * D, 0.0), amax(n * D, 0.0), sacc(n * D, 0.0), dl(n, delta_parameter);
  std::vector<Status> result(n, OkStatus());
  std::vector<char> seen(num_planners_, 0);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_ || seen[planners[k]])
      return std::vector<Status>(n, InvalidArgumentError("no such planner, or listed twice"));
    seen[planners[k]] = 1;
    ids[k] = (int32_t)planners[k];
    t[k] = ::tpamd::compat::ToUnixNanos(time[k]);
    bool ok = true;
    for (const VectorXd &w : waypoints[k])
      if (w.size() != D) ok = false;
    if (!ok) result[k] = InvalidArgumentError("waypoint has the wrong dimension");
    if (ok && (max_velocity[k].size() != D || max_acceleration[k].size() != D)) {
      result[k] = InvalidArgumentError("max_velocity / max_acceleration has the wrong dimension");
      ok = false;
    }
    if (ok && !stopping_acceleration.empty() && stopping_acceleration[k].size() != D) {
      result[k] = InvalidArgumentError("position.size != acceleration.size.");
      ok = false;
    }
    if (ok) {
      for (const VectorXd &w : waypoints[k]) wps.insert(wps.end(), w.begin(), w.end());
      for (size_t d = 0; d < D; d++) {
        vmax[k * D + d] = max_velocity[k][d];
        amax[k * D + d] = max_acceleration[k][d];
        sacc[k * D + d] = stopping_acceleration.empty() ? max_acceleration[k][d] : stopping_acceleration[k][d];
      }
    }
    // a planner that failed a check goes to the device with a zero stopping acceleration: it is
    // refused there before anything is written and keeps its state
    offsets[k + 1] = offsets[k] + (ok ? (int32_t)waypoints[k].size() : 0);
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  retarget_position_.assign(n * D, nan);
  retarget_velocity_.assign(n * D, nan);
  retarget_stop_.assign(n * D, nan);
  if (n == 0) return result;
  if (wps.empty()) wps.push_back(0.0);
  const int rc = tpamd_planner_set_retarget(set_, (int)n, ids.data(), t.data(), offsets.data(), wps.data(), rounding,
                                            vmax.data(), amax.data(), dl.data(), sacc.data(), np.data(), st.data(),
                                            retarget_position_.data(), retarget_velocity_.data(), retarget_stop_.data());
  if (rc != 0) return std::vector<Status>(n, rc == TPAMD_E_INVALID_ARGUMENT ? InvalidArgumentError(tpamd_error_string(rc))
                                                                           : InternalError(tpamd_error_string(rc)));
  for (size_t k = 0; k < n; k++) {
    if (!result[k].ok()) continue;
    switch (st[k]) {
      case TPAMD_PLAN_OK: summary_[planners[k]].path_state = 1; break;     // kNewPath
      case TPAMD_PLAN_FAILED_PRECONDITION: result[k] = FailedPreconditionError("No samples."); break;
      case TPAMD_PLAN_OUT_OF_RANGE: result[k] = OutOfRangeError("retarget time outside the trajectory"); break;
      case TPAMD_PLAN_INVALID_ARGUMENT:
        result[k] = InvalidArgumentError("Acceleration limits must be strictly positive.");
        break;
      default: result[k] = InternalError("retarget failed"); break;
    }
  }
  return result;
}

namespace {
Status StateStatus(int32_t st) {
  switch (st) {
    case TPAMD_PLAN_OK: return OkStatus();
    case TPAMD_PLAN_FAILED_PRECONDITION: return FailedPreconditionError("the planner waits for IK rows");
    case TPAMD_PLAN_RESOURCE_EXHAUSTED: return ::tpamd::compat::ResourceExhaustedError("the record does not fit");
    case TPAMD_PLAN_INVALID_ARGUMENT: return InvalidArgumentError("no such planner, or not a record for this set");
    default: return InternalError("state transfer failed");
  }
}
Status StateCallStatus(int rc) {
  return rc == TPAMD_E_INVALID_ARGUMENT ? InvalidArgumentError(tpamd_error_string(rc)) : InternalError(tpamd_error_string(rc));
}
}  // namespace

Status PathTimingTrajectorySet::ExportPlanners(const std::vector<size_t> &planners, PlannerStateBlob *blob) {
  if (!init_status_.ok()) return init_status_;
  if (!blob) return InvalidArgumentError("no blob");
  const size_t n = planners.size();
  blob->bytes.clear();
  blob->offsets.assign(n + 1, 0);
  blob->status.assign(n, OkStatus());
  if (n == 0) return OkStatus();
  std::vector<int32_t> ids(n), st(n);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    ids[k] = (int32_t)planners[k];
  }
  std::vector<tpamd_planner_state_info> info(n);
  int rc = tpamd_planner_set_state_info(set_, (int)n, ids.data(), info.data());
  if (rc != 0) return StateCallStatus(rc);
  // a planner that refuses (it waits for rows) gets no room: the export reports it
  for (size_t k = 0; k < n; k++) blob->offsets[k + 1] = blob->offsets[k] + (info[k].status == TPAMD_PLAN_OK ? info[k].bytes : 0);
  blob->bytes.assign((size_t)blob->offsets[n] + 16, 0);
  rc = tpamd_planner_set_export_state_host(set_, (int)n, ids.data(), blob->bytes.data(), blob->offsets.data(), st.data());
  if (rc != 0) return StateCallStatus(rc);
  blob->bytes.resize((size_t)blob->offsets[n]);
  for (size_t k = 0; k < n; k++) blob->status[k] = StateStatus(st[k]);
  return OkStatus();
}

void PathTimingTrajectorySet::TakeImported(const std::vector<size_t> &planners, const std::vector<int32_t> &status,
                                           const std::vector<tpamd_planner_summary> &summary,
                                           std::vector<Status> *result) {
  for (size_t k = 0; k < planners.size(); k++) {
    (*result)[k] = StateStatus(status[k]);
    if (status[k] != TPAMD_PLAN_OK) continue;
    summary_[planners[k]] = summary[k];
    ForgetStreamSource(planners[k]);
  }
}

std::vector<Status> PathTimingTrajectorySet::ImportPlanners(const std::vector<size_t> &planners,
                                                            const PlannerStateBlob &blob) {
  const size_t n = planners.size();
  if (!init_status_.ok()) return std::vector<Status>(n, init_status_);
  std::vector<Status> result(n, OkStatus());
  if (n == 0) return result;
  if (blob.offsets.size() != n + 1 || blob.offsets[0] < 0 || (size_t)blob.offsets[n] > blob.bytes.size())
    return std::vector<Status>(n, InvalidArgumentError("the blob does not hold one record per listed planner"));
  std::vector<int32_t> ids(n), st(n, -1);
  for (size_t k = 0; k < n; k++) ids[k] = planners[k] < num_planners_ ? (int32_t)planners[k] : -1;
  std::vector<tpamd_planner_summary> summary(n);
  const int rc = tpamd_planner_set_import_state_host(set_, (int)n, ids.data(), blob.bytes.data(), blob.offsets.data(),
                                                     summary.data(), st.data());
  if (rc != 0) return std::vector<Status>(n, StateCallStatus(rc));
  TakeImported(planners, st, summary, &result);
  return result;
}

std::vector<Status> PathTimingTrajectorySet::CopyPlanners(PathTimingTrajectorySet *dst,
                                                          const std::vector<size_t> &dst_planners,
                                                          PathTimingTrajectorySet *src,
                                                          const std::vector<size_t> &src_planners) {
  const size_t n = dst_planners.size();
  if (!dst || !src || src_planners.size() != n)
    return std::vector<Status>(n, InvalidArgumentError("two sets and as many source as destination planners"));
  if (!dst->init_status_.ok()) return std::vector<Status>(n, dst->init_status_);
  if (!src->init_status_.ok()) return std::vector<Status>(n, src->init_status_);
  std::vector<Status> result(n, OkStatus());
  if (n == 0) return result;
  std::vector<int32_t> di(n), si(n), st(n, -1);
  for (size_t k = 0; k < n; k++) {
    di[k] = dst_planners[k] < dst->num_planners_ ? (int32_t)dst_planners[k] : -1;
    si[k] = src_planners[k] < src->num_planners_ ? (int32_t)src_planners[k] : -1;
  }
  std::vector<tpamd_planner_summary> summary(n);
  const int rc = tpamd_planner_set_copy_planners(dst->set_, di.data(), src->set_, si.data(), (int)n, summary.data(), st.data());
  if (rc != 0) return std::vector<Status>(n, StateCallStatus(rc));
  dst->TakeImported(dst_planners, st, summary, &result);
  return result;
}

Status PathTimingTrajectorySet::AdoptPlanner(size_t slot, const PathTimingTrajectory &planner) {
  if (!init_status_.ok()) return init_status_;
  if (cartesian_) return FailedPreconditionError("a Cartesian set takes IK tables");
  if (slot >= num_planners_) return InvalidArgumentError("no such planner");
  PlannerStateBlob blob;
  if (Status st = PlannerStateFromHost(planner, &blob.bytes, constraint_safety_); !st.ok()) return st;
  blob.offsets = {0, (int64_t)blob.bytes.size()};
  return ImportPlanners({slot}, blob)[0];
}

Status PathTimingTrajectorySet::ReleasePlanner(size_t slot, PathTimingTrajectory *planner) {
  if (!init_status_.ok()) return init_status_;
  if (cartesian_) return FailedPreconditionError("a Cartesian set's planners have no host form");
  if (slot >= num_planners_ || !planner) return InvalidArgumentError("no such planner");
  PlannerStateBlob blob;
  if (Status st = ExportPlanners({slot}, &blob); !st.ok()) return st;
  if (!blob.status[0].ok()) return blob.status[0];
  if (Status st = PlannerStateToHost(blob.bytes.data(), blob.bytes.size(), planner); !st.ok()) return st;
  Reset(slot);
  return OkStatus();
}

Status PathTimingTrajectorySet::GetPath(size_t planner, std::vector<double> *knots,
                                        std::vector<double> *control_points) const {
  if (!init_status_.ok()) return init_status_;
  if (cartesian_) return FailedPreconditionError("a Cartesian set has IK tables (GetIkTable)");
  if (planner >= num_planners_ || !knots || !control_points) return InvalidArgumentError("no such planner");
  const size_t P = NumControlPoints(planner), D = options_.GetNumDofs();
  knots->assign(P ? P + 3 : 0, 0.0);
  control_points->assign(P * D, 0.0);
  if (P == 0) return OkStatus();
  int32_t got = 0;
  const int rc = tpamd_planner_set_download_path(set_, (int)planner, &got, knots->data(), control_points->data(), (int)P);
  return rc == 0 && (size_t)got == P ? OkStatus() : InternalError(tpamd_error_string(rc));
}

size_t PathTimingTrajectorySet::NumControlPoints(size_t planner) const {
  if (!init_status_.ok() || planner >= num_planners_ || cartesian_) return 0;
  int32_t np = 0;
  tpamd_planner_set_download_path(set_, (int)planner, &np, nullptr, nullptr, 0);   // host copy: no transfer
  return (size_t)np;
}

Status PathTimingTrajectorySet::GetTrajectory(size_t planner, PlannedTrajectory *out) const {
  if (!init_status_.ok()) return init_status_;
  if (plan_pending_) return FailedPreconditionError("a PlanDevice call is in flight (FinishPlanDevice)");
  if (planner >= num_planners_ || !out) return InvalidArgumentError("no such planner");
  const size_t n = (size_t)summary_[planner].num_samples, D = options_.GetNumDofs();
  out->time.resize(n); out->path_parameter.resize(n); out->path_parameter_derivative.resize(n);
  out->second_path_parameter_derivative.resize(n);
  out->positions.resize(n * D); out->velocities.resize(n * D); out->accelerations.resize(n * D);
  if (n == 0) return OkStatus();
  const int rc = tpamd_planner_set_download_trajectory(
      set_, (int)planner, 0, (int)n, out->time.data(), out->path_parameter.data(), out->path_parameter_derivative.data(),
      out->second_path_parameter_derivative.data(), out->positions.data(), out->velocities.data(),
      out->accelerations.data());
  return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc));
}

Status PathTimingTrajectorySet::GetTrajectories(const std::vector<size_t> &planners,
                                                std::vector<PlannedTrajectory> *out) const {
  if (!init_status_.ok()) return init_status_;
  if (plan_pending_) return FailedPreconditionError("a PlanDevice call is in flight (FinishPlanDevice)");
  if (!out) return InvalidArgumentError("no output");
  const size_t n = planners.size(), D = options_.GetNumDofs();
  std::vector<int32_t> ids(n);
  size_t rows = 0;      // the summaries' sample counts: the packed size, unless the set changed since
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    ids[k] = (int32_t)planners[k];
    rows += (size_t)summary_[planners[k]].num_samples;
  }
  std::vector<int64_t> offsets(n + 1);
  std::vector<double> t, s, sd, sdd, q, qd, qdd;
  for (int attempt = 0;; attempt++) {
    const size_t r = std::max<size_t>(rows, 1);
    t.resize(r); s.resize(r); sd.resize(r); sdd.resize(r); q.resize(r * D); qd.resize(r * D); qdd.resize(r * D);
    const int rc = tpamd_planner_set_download_trajectories(set_, (int)n, ids.data(), offsets.data(), (int64_t)rows,
                                                           t.data(), s.data(), sd.data(), sdd.data(), q.data(),
                                                           qd.data(), qdd.data());
    if (rc == 0) break;
    if (rc != TPAMD_E_INVALID_ARGUMENT || attempt > 0 || (size_t)offsets[n] <= rows)
      return InternalError(tpamd_error_string(rc));
    rows = (size_t)offsets[n];           // grow to the total and go again
  }
  out->assign(n, PlannedTrajectory());
  for (size_t k = 0; k < n; k++) {
    const size_t a = (size_t)offsets[k], b = (size_t)offsets[k + 1];
    PlannedTrajectory &o = (*out)[k];
    o.time.assign(t.begin() + a, t.begin() + b);
    o.path_parameter.assign(s.begin() + a, s.begin() + b);
    o.path_parameter_derivative.assign(sd.begin() + a, sd.begin() + b);
    o.second_path_parameter_derivative.assign(sdd.begin() + a, sdd.begin() + b);
    o.positions.assign(q.begin() + a * D, q.begin() + b * D);
    o.velocities.assign(qd.begin() + a * D, qd.begin() + b * D);
    o.accelerations.assign(qdd.begin() + a * D, qdd.begin() + b * D);
  }
  return OkStatus();
}

Status PathTimingTrajectorySet::GetSetpoints(const std::vector<size_t> &planners, const std::vector<Time> &start,
                                             Duration step, int ticks, TrajectorySetpoints *out) const {
  if (!init_status_.ok()) return init_status_;
  if (!out || start.size() != planners.size()) return InvalidArgumentError("one start time per planner");
  if (step.nanos() <= 0 || ticks < 1) return InvalidArgumentError("step and ticks must be positive");
  const size_t n = planners.size(), D = options_.GetNumDofs(), T = (size_t)ticks;
  std::vector<int32_t> ids(n);
  std::vector<int64_t> s(n);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    ids[k] = (int32_t)planners[k];
    s[k] = ::tpamd::compat::ToUnixNanos(start[k]);
  }
  const double nan = std::numeric_limits<double>::quiet_NaN();
  out->num_planners = n; out->num_ticks = T; out->num_dofs = D;
  out->positions.assign(n * T * D, nan);
  out->velocities.assign(n * T * D, nan);
  out->accelerations.assign(n * T * D, nan);
  out->status.assign(n * T, OkStatus());
  if (n == 0) return OkStatus();
  std::vector<int32_t> st(n * T);
  const int rc = tpamd_planner_set_sample_at_ticks(set_, (int)n, ids.data(), s.data(), step.nanos(), ticks,
                                                   out->positions.data(), out->velocities.data(),
                                                   out->accelerations.data(), st.data());
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  for (size_t i = 0; i < n * T; i++) {
    switch (st[i]) {
      case TPAMD_PLAN_OK: break;
      case TPAMD_PLAN_FAILED_PRECONDITION: out->status[i] = FailedPreconditionError("No samples."); break;
      case TPAMD_PLAN_OUT_OF_RANGE: out->status[i] = OutOfRangeError("Time outside the trajectory"); break;
      case TPAMD_PLAN_INVALID_ARGUMENT: out->status[i] = InvalidArgumentError("no such planner"); break;
      default: out->status[i] = InternalError("setpoint query failed"); break;
    }
  }
  return OkStatus();
}

Status PathTimingTrajectorySet::StopTrajectoriesBeforeTime(const std::vector<size_t> &planners,
                                                           const std::vector<Time> &time,
                                                           const std::vector<VectorXd> &max_acceleration,
                                                           double time_step, std::vector<StoppingSegment> *out) const {
  if (!init_status_.ok()) return init_status_;
  const size_t n = planners.size(), D = options_.GetNumDofs();
  if (!out || time.size() != n || max_acceleration.size() != n)
    return InvalidArgumentError("one time and one max_acceleration per planner");
  std::vector<int32_t> ids(n), st(n), keep(n);
  std::vector<int64_t> t(n), offsets(n + 1);
  std::vector<double> amax(n * D);
  for (size_t k = 0; k < n; k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    if (max_acceleration[k].size() != D) return InvalidArgumentError("max_acceleration has the wrong dimension");
    ids[k] = (int32_t)planners[k];
    t[k] = ::tpamd::compat::ToUnixNanos(time[k]);
    std::copy(max_acceleration[k].begin(), max_acceleration[k].end(), amax.begin() + k * D);
  }
  out->assign(n, StoppingSegment());
  if (n == 0) return OkStatus();
  // The segments' total is known only after the stop: a first call without room reports it (and
  // the statuses), the second writes the rows. Segments are short next to the trajectories, so
  // sizing the arrays exactly beats a generous first guess.
  std::vector<double> tm, q, qd, qdd;
  size_t rows = 0;
  for (int attempt = 0;; attempt++) {
    const size_t r = std::max<size_t>(rows, 1);
    tm.resize(r); q.resize(r * D); qd.resize(r * D); qdd.resize(r * D);
    const int rc = tpamd_planner_set_stop_trajectories(set_, (int)n, ids.data(), t.data(), amax.data(), time_step,
                                                       st.data(), keep.data(), offsets.data(), (int64_t)rows,
                                                       tm.data(), q.data(), qd.data(), qdd.data());
    if (rc == 0) break;
    if (rc != TPAMD_E_INVALID_ARGUMENT || attempt > 0 || (size_t)offsets[n] <= rows)
      return InternalError(tpamd_error_string(rc));
    rows = (size_t)offsets[n];           // grow to the total and go again
  }
  for (size_t k = 0; k < n; k++) {
    StoppingSegment &o = (*out)[k];
    switch (st[k]) {
      case TPAMD_PLAN_OK: o.status = OkStatus(); break;
      case TPAMD_PLAN_OUT_OF_RANGE: o.status = OutOfRangeError("stop index or time out of range"); break;
      case TPAMD_PLAN_INVALID_ARGUMENT: o.status = InvalidArgumentError("invalid stop arguments or samples"); break;
      case TPAMD_PLAN_NOT_FOUND:
        o.status = NotFoundError("No safe stopping trajectory found (likely not enough time).");
        break;
      default: o.status = InternalError("no stopping trajectory"); break;
    }
    o.keep = (size_t)keep[k];
    const size_t a = (size_t)offsets[k], b = (size_t)offsets[k + 1];
    o.time.assign(tm.begin() + a, tm.begin() + b);
    o.positions.assign(q.begin() + a * D, q.begin() + b * D);
    o.velocities.assign(qd.begin() + a * D, qd.begin() + b * D);
    o.accelerations.assign(qdd.begin() + a * D, qdd.begin() + b * D);
  }
  return OkStatus();
}

size_t PathTimingTrajectorySet::LastPlanBytesOverPcie() const {
  size_t up = 0, down = 0;
  tpamd_planner_set_last_plan_bytes(set_, &up, &down);
  return up + down;
}

Status PathTimingTrajectorySet::SetChecking(bool on) {
  if (!init_status_.ok()) return init_status_;
  if (plan_pending_) return FailedPreconditionError("a PlanDevice call is in flight (FinishPlanDevice)");
  const int rc = tpamd_planner_set_set_checking(set_, on ? 1 : 0);
  return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc));
}

Status PathTimingTrajectorySet::CheckResults(const std::vector<size_t> &planners,
                                             std::vector<tpamd_planner_check> *out) const {
  if (!init_status_.ok()) return init_status_;
  if (!out) return InvalidArgumentError("no output");
  std::vector<int32_t> ids(planners.size());
  for (size_t k = 0; k < planners.size(); k++) {
    if (planners[k] >= num_planners_) return InvalidArgumentError("no such planner");
    ids[k] = (int32_t)planners[k];
  }
  std::vector<tpamd_planner_check> records(std::max<size_t>(planners.size(), 1));
  const int rc = tpamd_planner_set_check_results(set_, (int)ids.size(), ids.data(), records.data());
  if (rc == TPAMD_E_INVALID_ARGUMENT) return InvalidArgumentError("more planners than the set has, or one listed twice");
  if (rc != 0) return InternalError(tpamd_error_string(rc));
  records.resize(planners.size());
  out->swap(records);
  return OkStatus();
}

Status PathTimingTrajectorySet::CheckResultsDevice(int count, const int32_t *planners_dev, tpamd_planner_check *out_dev,
                                                   void *hip_stream) const {
  if (!init_status_.ok()) return init_status_;
  const int rc = tpamd_planner_set_check_results_device(set_, count, planners_dev, out_dev, hip_stream);
  if (rc == TPAMD_E_INVALID_ARGUMENT) return InvalidArgumentError("no output, or a count outside 0 .. NumPlanners()");
  return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc));
}

size_t PathTimingTrajectorySet::DeviceBytes() const { return tpamd_planner_set_device_bytes(set_); }

}  // namespace trajectory_planning

// GPU test of PathTimingTrajectorySet::SetCartesianWaypointPaths (run by
// tests/test_gpu_cartesian_waypoint_set.py): Cartesian sets of 6 planners, D = 6 and 7, N = 64, 2..4
// pose waypoints per planner. The device IK returns the joint targets unchanged and one fixed
// Jacobian per planner, so the whole chain is bit-exact:
//   - the resident table (GetIkTable) equals the table built on the host: the fit through
//     tpamd_fit_pose_waypoints_host (the same kernel), rows from tpamd_ik_table_rows, the oracle's
//     tpo_eval_curve at r * delta below path_end - delta and the last joint control point from there on;
//   - the first Plan and two replans equal one oracle IK-table planner per planner
//     (tpo_planner_set_ik_table + tpo_planner_plan), summaries and trajectories bit for bit;
//   - a planner with an empty waypoint list makes the call return InvalidArgument, keeps its path and
//     its plan, and does not disturb the others;
//   - on a joint set the method returns FailedPrecondition.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/host/engine_handle.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"

#define TEST_SUPPORT_SEED 20261018ULL
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::Pose3d;
using tpamd::compat::Quaterniond;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using tpamd::compat::Vector3d;

static const int kB = 6, kN = 64;
static const double kDelta = 0.1, kSafety = 0.8, kMaxIvError = 1e-3;
static const int kMaxIter = 10000;

struct Goal {
  std::vector<Pose3d> poses;
  std::vector<VectorXd> joints;
  std::vector<double> jacobian;     // [6][D], fixed
};

static Goal MakeGoal(int W, int D) {
  Goal g;
  for (int i = 0; i < W; i++) {
    double q[4], n = 0.0;
    for (double &x : q) { x = 2.0 * Rnd() - 1.0; n += x * x; }
    n = std::sqrt(n);
    g.poses.push_back(Pose3d(Quaterniond(q[0] / n, q[1] / n, q[2] / n, q[3] / n),
                             Vector3d(2.0 * Rnd() - 1.0, 2.0 * Rnd() - 1.0, 2.0 * Rnd() - 1.0)));
    VectorXd j(D);
    for (int d = 0; d < D; d++) j[d] = 2.0 * Rnd() - 1.0;
    g.joints.push_back(j);
  }
  g.jacobian.resize((size_t)6 * D);
  for (int r = 0; r < 6; r++)
    for (int d = 0; d < D; d++) g.jacobian[(size_t)r * D + d] = 0.25 * (2.0 * Rnd() - 1.0) + (r == d % 6 ? 1.0 : 0.0);
  return g;
}

// The table the chain must leave for one goal, built on the host.
struct Table {
  int rows = 0;
  double path_end = 0.0;
  std::vector<double> q, J;
};

static Table HostTable(tpamd_engine *e, const Goal &g, int D, double tr, double rr) {
  Table t;
  const int W = (int)g.poses.size(), P = W == 1 ? 4 : 3 * W - 2;
  std::vector<double> pose, joint;
  for (int i = 0; i < W; i++) {
    const Quaterniond &q = g.poses[i].quaternion();
    const Vector3d &v = g.poses[i].translation();
    const double row[7] = {v[0], v[1], v[2], q.w, q.x, q.y, q.z};
    pose.insert(pose.end(), row, row + 7);
    joint.insert(joint.end(), g.joints[i].begin(), g.joints[i].end());
  }
  const int32_t off[2] = {0, W};
  std::vector<double> knots(P + 3), tp((size_t)3 * P), rp((size_t)4 * P), jc((size_t)P * D);
  int32_t np = 0, po[2] = {0, 0}, st = -1;
  CHECK(tpamd_fit_pose_waypoints_host(e, 1, D, off, pose.data(), joint.data(), &tr, &rr, knots.data(), tp.data(),
                                      rp.data(), jc.data(), &np, po, &t.path_end, &st) == 0);
  CHECK(np == P && st == TPAMD_PLAN_OK && po[1] == P && t.path_end == knots[P + 2]);
  t.rows = tpamd_ik_table_rows(t.path_end, kDelta, kN);
  CHECK(t.rows == (int)std::round(t.path_end / kDelta) + kN + 1);
  t.q.resize((size_t)t.rows * D);
  for (int r = 0; r < t.rows; r++) {
    const double parameter = r * kDelta;
    if (parameter < knots[P + 2] - kDelta)
      CHECK(tpo_eval_curve(knots.data(), P + 3, 2, jc.data(), D, parameter, &t.q[(size_t)r * D]) == 0);
    else
      std::memcpy(&t.q[(size_t)r * D], &jc[(size_t)(P - 1) * D], D * 8);
    t.J.insert(t.J.end(), g.jacobian.begin(), g.jacobian.end());
  }
  return t;
}

static int Compare(const PathTimingTrajectorySet &set, int b, const tpo_planner *p, int D) {
  const size_t n = (size_t)tpo_planner_num_samples(p);
  if (set.GetNumTimeSamples(b) != n) return 1;
  int bad = 0;
  bad |= (ToUnixNanos(set.GetEndTime(b)) != tpo_planner_end_time(p)) << 1;
  bad |= (ToUnixNanos(set.GetFinalDecelStart(b)) != tpo_planner_final_decel_start(p)) << 2;
  PlannedTrajectory t;
  if (!set.GetTrajectory(b, &t).ok()) return bad | (1 << 3);
  bad |= !SameBits(t.time, tpo_planner_time(p), n) << 4;
  bad |= !SameBits(t.path_parameter, tpo_planner_path_parameter(p), n) << 5;
  bad |= !SameBits(t.positions, tpo_planner_positions(p), n * D) << 6;
  bad |= !SameBits(t.velocities, tpo_planner_velocities(p), n * D) << 7;
  bad |= !SameBits(t.accelerations, tpo_planner_accelerations(p), n * D) << 8;
  return bad;
}

static void Scenario(int D) {
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(4)).SetMaxInitialVelocityError(kMaxIvError)
      .SetMaxPlanningLoops(kMaxIter);
  PathTimingTrajectorySet set(opt, kB, CartesianTableCapacity{(size_t)kN}, kSafety);
  CHECK(set.status().ok() && set.is_cartesian());
  if (!set.status().ok()) return;
  std::vector<Goal> goals;
  std::vector<size_t> all;
  CartesianPathLimits lim;
  lim.delta_parameter = kDelta;
  lim.translation_rounding = 0.05;
  lim.rotation_rounding = 0.2;
  for (int b = 0; b < kB; b++) {
    goals.push_back(MakeGoal(2 + b % 3, D));
    all.push_back(b);
    VectorXd v(D), a(D);
    for (int d = 0; d < D; d++) { v[d] = 0.6 + 0.5 * Rnd(); a[d] = 1.5 + 1.5 * Rnd(); }
    lim.max_velocity.push_back(v);
    lim.max_acceleration.push_back(a);
    lim.max_translational_velocity.push_back(0.4 + 0.2 * Rnd());
    lim.max_rotational_velocity.push_back(0.8 + 0.4 * Rnd());
  }
  // the device IK: the joint targets unchanged, planner k's fixed Jacobian on each of its rows
  std::vector<size_t> listed;       // planners of the call in flight, in row_offsets order
  int ik_calls = 0;
  const DeviceIkFunc ik = [&](const double *pose_targets, const double *joint_targets,
                              const std::vector<int32_t> &row_offsets, double *q, double *J, void *stream) {
    ik_calls++;
    CHECK(pose_targets != nullptr && row_offsets.size() == listed.size() + 1);
    const size_t rows = (size_t)row_offsets.back();
    if (hipMemcpyAsync(q, joint_targets, rows * D * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
      return tpamd::compat::InternalError("copy");
    std::vector<double> host;
    for (size_t k = 0; k + 1 < row_offsets.size(); k++)
      for (int r = row_offsets[k]; r < row_offsets[k + 1]; r++)
        host.insert(host.end(), goals[listed[k]].jacobian.begin(), goals[listed[k]].jacobian.end());
    if (hipMemcpy(J, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
      return tpamd::compat::InternalError("copy");
    return tpamd::compat::OkStatus();
  };
  listed = all;
  std::vector<std::vector<Pose3d>> poses;
  std::vector<std::vector<VectorXd>> joints;
  for (const Goal &g : goals) { poses.push_back(g.poses); joints.push_back(g.joints); }
  CHECK(set.SetCartesianWaypointPaths(all, poses, joints, lim, ik).ok());
  CHECK(ik_calls == 1);
  // the resident tables against the host-built ones; the oracle planners
  std::vector<Table> tables;
  std::vector<tpo_planner *> orc;
  {
    tpamd::EngineLease lease = tpamd::acquire_engine();
    CHECK((bool)lease);
    if (!lease) return;
    for (int b = 0; b < kB; b++) tables.push_back(HostTable(lease.get(), goals[b], D, 0.05, 0.2));
  }
  int tables_equal = 0;
  for (int b = 0; b < kB; b++) {
    std::vector<double> q, J;
    CHECK(set.GetIkTable(b, &q, &J).ok());
    const bool same = SameBits(q, tables[b].q.data(), tables[b].q.size()) && SameBits(J, tables[b].J.data(), tables[b].J.size());
    CHECK(same);
    tables_equal += same;
    tpo_planner *p = tpo_planner_create(D, kN, kDelta, kSafety, 4 * kMs, 0, kMaxIter, kMaxIvError);
    tpo_planner_set_limits(p, lim.max_velocity[b].data(), lim.max_acceleration[b].data());
    tpo_planner_set_ik_table(p, tables[b].q.data(), tables[b].J.data(), tables[b].rows, tables[b].path_end,
                             lim.max_translational_velocity[b], lim.max_rotational_velocity[b], 1);
    orc.push_back(p);
  }
  std::printf("D %d: %d of %d resident tables equal the host-built ones\n", D, tables_equal, kB);
  // the first Plan and two replans
  std::vector<int64_t> start(kB, 0);
  int plans_equal = 0, replan_windows = 0;
  for (int step = 0; step < 3; step++) {
    std::vector<Time> st;
    for (int b = 0; b < kB; b++) st.push_back(FromUnixNanos(start[b]));
    const auto got = set.Plan(st, std::vector<tpamd::compat::Duration>(kB, Milliseconds(1500)));
    for (int b = 0; b < kB; b++) {
      const int rc = tpo_planner_plan(orc[b], start[b], 1500 * kMs);
      CHECK(rc == TPO_PLAN_OK && got[b].ok());
      const int bad = Compare(set, b, orc[b], D);
      if (bad) std::printf("  step %d planner %d differs: %x\n", step, b, bad);
      CHECK(bad == 0);
      plans_equal += bad == 0;
      CHECK(set.WindowsOfLastPlan(b) == tpo_planner_windows(orc[b]));
      if (step > 0) replan_windows += tpo_planner_windows(orc[b]);
      start[b] = std::min<int64_t>(tpo_planner_end_time(orc[b]), start[b] + 400 * kMs);
    }
  }
  CHECK(replan_windows > 0);        // the replans are not all of the "planned enough" kind
  std::printf("D %d: %d of %d plans equal the oracle planners\n", D, plans_equal, 3 * kB);
  // an empty waypoint list: planner 2 keeps path and plan, planners 0 and 4 get new goals
  {
    const std::vector<size_t> some = {0, 2, 4};
    Goal g0 = MakeGoal(3, D), g4 = MakeGoal(4, D);
    CartesianPathLimits l2 = lim;
    l2.max_velocity = {lim.max_velocity[0], lim.max_velocity[2], lim.max_velocity[4]};
    l2.max_acceleration = {lim.max_acceleration[0], lim.max_acceleration[2], lim.max_acceleration[4]};
    l2.max_translational_velocity = {lim.max_translational_velocity[0], lim.max_translational_velocity[2],
                                     lim.max_translational_velocity[4]};
    l2.max_rotational_velocity = {lim.max_rotational_velocity[0], lim.max_rotational_velocity[2],
                                  lim.max_rotational_velocity[4]};
    goals[0] = g0;
    goals[4] = g4;
    listed = {0, 4};
    std::vector<double> before_q, before_J;
    CHECK(set.GetIkTable(2, &before_q, &before_J).ok());
    PlannedTrajectory before;
    CHECK(set.GetTrajectory(2, &before).ok());
    const Status st = set.SetCartesianWaypointPaths(some, {g0.poses, {}, g4.poses}, {g0.joints, {}, g4.joints}, l2, ik);
    CHECK(st.code() == StatusCode::kInvalidArgument && ik_calls == 2);
    std::vector<double> after_q, after_J;
    CHECK(set.GetIkTable(2, &after_q, &after_J).ok());
    PlannedTrajectory after;
    CHECK(set.GetTrajectory(2, &after).ok());
    const bool kept = after_q == before_q && after_J == before_J && after.time == before.time &&
                      after.positions == before.positions;
    CHECK(kept);
    tpamd::EngineLease lease = tpamd::acquire_engine();
    CHECK((bool)lease);
    bool loaded = (bool)lease;
    for (int b : {0, 4}) {
      if (!lease) break;
      const Table t = HostTable(lease.get(), goals[b], D, 0.05, 0.2);
      std::vector<double> q, J;
      CHECK(set.GetIkTable(b, &q, &J).ok());
      loaded = loaded && SameBits(q, t.q.data(), t.q.size()) && SameBits(J, t.J.data(), t.J.size());
    }
    CHECK(loaded);
    // untouched planners keep planning exactly as the oracle does
    std::vector<Time> tm;
    for (int b = 0; b < kB; b++) tm.push_back(FromUnixNanos(start[b]));   // 0 and 4 start their new paths here
    const auto got = set.Plan(tm, std::vector<tpamd::compat::Duration>(kB, Milliseconds(1500)));
    bool others = true;
    for (int b : {1, 2, 3, 5}) {
      CHECK(tpo_planner_plan(orc[b], start[b], 1500 * kMs) == TPO_PLAN_OK && got[b].ok());
      others = others && Compare(set, b, orc[b], D) == 0;
    }
    CHECK(others && got[0].ok() && got[4].ok());
    if (kept && loaded && others)
      std::printf("D %d: empty waypoint list: InvalidArgument, planner kept, others loaded and undisturbed\n", D);
  }
  for (tpo_planner *p : orc) tpo_planner_destroy(p);
}

static void JointSetRefuses() {
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(7).SetNumPathSamples(kN).SetTimeStep(Milliseconds(4));
  PathTimingTrajectorySet set(opt, 2, 8);
  CHECK(set.status().ok() && !set.is_cartesian());
  if (!set.status().ok()) return;
  Goal g = MakeGoal(3, 7);
  CartesianPathLimits lim;
  lim.max_velocity = {VectorXd(7, 1.0)};
  lim.max_acceleration = {VectorXd(7, 1.0)};
  lim.max_translational_velocity = {0.5};
  lim.max_rotational_velocity = {1.0};
  int calls = 0;
  const DeviceIkFunc ik = [&](const double *, const double *, const std::vector<int32_t> &, double *, double *, void *) {
    calls++;
    return tpamd::compat::OkStatus();
  };
  const Status st = set.SetCartesianWaypointPaths({0}, {g.poses}, {g.joints}, lim, ik);
  CHECK(st.code() == StatusCode::kFailedPrecondition && calls == 0);
  if (st.code() == StatusCode::kFailedPrecondition) std::printf("SetCartesianWaypointPaths on a joint set: refused\n");
}

int main() {
  if (tpamd::device_count() < 1) {
    std::printf("no GPU\n");
    return 1;
  }
  Scenario(6);
  Scenario(7);
  JointSetRefuses();
  if (g_fail) {
    std::printf("%d CHECKS FAILED\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

// GPU test of streaming IK tables through the mirror's device chain (run by
// tests/test_gpu_cartesian_stream.py): PathTimingTrajectorySet::SetCartesianWaypointPaths(..., ik,
// streaming) uploads rows 0 .. N-1 only and keeps the fitted splines in device memory; PlanStreaming
// extends a waiting planner's table through tpamd_sample_ik_target_rows_device, the caller's device IK
// (which now receives the seed row) and tpamd_planner_set_append_ik_rows_device. Held against the
// non-streaming SetCartesianWaypointPaths set of the same goals: every Plan's summaries and
// trajectories up to the target, bit for bit; the streamed tables are a prefix of the whole ones;
// every seed row is the table's last row.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/tpamd.h"
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


static bool Same(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
}

static void Scenario(int D, bool skip) {
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(4)).SetMaxInitialVelocityError(kMaxIvError)
      .SetMaxPlanningLoops(kMaxIter);
  if (skip) opt.SetTimeSamplingMethod(PathTimingTrajectoryOptions::TimeSamplingMethod::kSkipSamplesCloserThanTimeStep);
  PathTimingTrajectorySet whole(opt, kB, CartesianTableCapacity{(size_t)kN}, kSafety),
      stream(opt, kB, CartesianTableCapacity{(size_t)kN}, kSafety);
  CHECK(whole.status().ok() && stream.status().ok());
  if (!whole.status().ok() || !stream.status().ok()) return;
  std::vector<Goal> goals;
  std::vector<size_t> all;
  CartesianPathLimits lim;
  lim.delta_parameter = kDelta;
  for (int b = 0; b < kB; b++) {
    goals.push_back(MakeGoal(3 + b % 3, D));
    all.push_back(b);
    VectorXd v(D), a(D);
    for (int d = 0; d < D; d++) { v[d] = 0.6 + 0.5 * Rnd(); a[d] = 1.5 + 1.5 * Rnd(); }
    lim.max_velocity.push_back(v);
    lim.max_acceleration.push_back(a);
    lim.max_translational_velocity.push_back(0.4 + 0.2 * Rnd());
    lim.max_rotational_velocity.push_back(0.8 + 0.4 * Rnd());
  }
  // the device IK: the joint targets unchanged, one fixed Jacobian on every row
  const std::vector<double> &jac = goals[0].jacobian;
  int calls = 0, seeded_calls = 0, seeds_checked = 0, seeds_equal = 0;
  auto solve = [&](const double *joint_targets, const std::vector<int32_t> &row_offsets, double *q, double *J, void *stream_) {
    const size_t rows = (size_t)row_offsets.back();
    if (hipMemcpyAsync(q, joint_targets, rows * D * 8, hipMemcpyDeviceToDevice, (hipStream_t)stream_) != hipSuccess)
      return tpamd::compat::InternalError("copy");
    std::vector<double> host;
    for (size_t r = 0; r < rows; r++) host.insert(host.end(), jac.begin(), jac.end());
    if (hipMemcpy(J, host.data(), host.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
      return tpamd::compat::InternalError("copy");
    return tpamd::compat::OkStatus();
  };
  const DeviceIkFunc ik = [&](const double *, const double *joint_targets, const std::vector<int32_t> &row_offsets, double *q,
                              double *J, void *s) { return solve(joint_targets, row_offsets, q, J, s); };
  const DeviceSeededIkFunc seeded = [&](const double *pose_targets, const double *joint_targets,
                                        const std::vector<int32_t> &row_offsets, const double *seed_rows, double *q,
                                        double *J, void *s) {
    calls++;
    CHECK(pose_targets != nullptr);
    if (seed_rows) {
      // the seed of every run is the table's last row, whose targets the run's first row repeats
      seeded_calls++;
      const size_t w = row_offsets.size() - 1;
      std::vector<double> seed(w * D), firsts(D);
      CHECK(hipMemcpyAsync(seed.data(), seed_rows, w * D * 8, hipMemcpyDeviceToHost, (hipStream_t)s) == hipSuccess);
      CHECK(hipStreamSynchronize((hipStream_t)s) == hipSuccess);
      for (size_t k = 0; k < w; k++) {
        CHECK(row_offsets[k + 1] - row_offsets[k] >= 2);
        CHECK(hipMemcpy(firsts.data(), joint_targets + (size_t)row_offsets[k] * D, D * 8, hipMemcpyDeviceToHost) == hipSuccess);
        seeds_checked++;
        seeds_equal += std::memcmp(firsts.data(), &seed[k * D], D * 8) == 0;
      }
    }
    return solve(joint_targets, row_offsets, q, J, s);
  };
  std::vector<std::vector<Pose3d>> poses;
  std::vector<std::vector<VectorXd>> joints;
  for (const Goal &g : goals) { poses.push_back(g.poses); joints.push_back(g.joints); }
  CHECK(whole.SetCartesianWaypointPaths(all, poses, joints, lim, ik).ok());
  CHECK(stream.SetCartesianWaypointPaths(all, poses, joints, lim, seeded, /*streaming=*/true).ok());
  CHECK(calls == 1 && seeded_calls == 0);
  for (int b = 0; b < kB; b++) CHECK(stream.GetIkTableRows(b) == kN && whole.GetIkTableRows(b) > 2 * kN);
  std::vector<int64_t> start(kB, 0);
  int plans = 0, equal = 0, suspensions = 0;
  PlannedTrajectory tw, ts;
  for (int step = 0; step < 300; step++) {
    std::vector<Time> st;
    for (int b = 0; b < kB; b++) st.push_back(FromUnixNanos(start[b]));
    const std::vector<tpamd::compat::Duration> hz(kB, Milliseconds(750));
    const auto sw = whole.Plan(st, hz);
    const auto ss = stream.PlanStreaming(st, hz);
    suspensions += stream.SuspensionsOfLastPlan();
    plans++;
    bool same = true, done = true;
    for (int b = 0; b < kB; b++) {
      CHECK(sw[b].ok() && ss[b].ok());
      same = same && whole.GetNumTimeSamples(b) == stream.GetNumTimeSamples(b) &&
             ToUnixNanos(whole.GetEndTime(b)) == ToUnixNanos(stream.GetEndTime(b)) &&
             ToUnixNanos(whole.GetFinalDecelStart(b)) == ToUnixNanos(stream.GetFinalDecelStart(b)) &&
             whole.IsTrajectoryAtEnd(b) == stream.IsTrajectoryAtEnd(b) && whole.WindowsOfLastPlan(b) == stream.WindowsOfLastPlan(b);
      CHECK(whole.GetTrajectory(b, &tw).ok() && stream.GetTrajectory(b, &ts).ok());
      same = same && Same(tw.time, ts.time) && Same(tw.path_parameter, ts.path_parameter) && Same(tw.positions, ts.positions) &&
             Same(tw.velocities, ts.velocities) && Same(tw.accelerations, ts.accelerations);
      if (!whole.IsTrajectoryAtEnd(b)) {
        start[b] = std::min<int64_t>(ToUnixNanos(whole.GetEndTime(b)), start[b] + 200 * kMs);
        done = false;
      }
    }
    CHECK(same);
    equal += same;
    if (done) break;
  }
  int at_end = 0, prefixes = 0;
  for (int b = 0; b < kB; b++) {
    at_end += whole.IsTrajectoryAtEnd(b) && stream.IsTrajectoryAtEnd(b);
    std::vector<double> qw, Jw, qs, Js;
    CHECK(whole.GetIkTable(b, &qw, &Jw).ok() && stream.GetIkTable(b, &qs, &Js).ok());
    const bool prefix = qs.size() > (size_t)kN * D && qs.size() < qw.size() &&
                        std::memcmp(qs.data(), qw.data(), qs.size() * 8) == 0 && std::memcmp(Js.data(), Jw.data(), Js.size() * 8) == 0;
    CHECK(prefix);
    prefixes += prefix;
  }
  CHECK(at_end == kB && equal == plans && suspensions >= kB && seeded_calls > 0 && seeds_checked == seeds_equal);
  CHECK(seeds_checked == suspensions);
  std::printf("waypoint streaming D %d %s: %d of %d Plan calls equal, %d suspensions in %d seeded IK calls, %d of %d seeds equal "
              "the table's last row, %d of %d streamed tables are shorter prefixes, %d at the end\n",
              D, skip ? "skip" : "uniform", equal, plans, suspensions, seeded_calls, seeds_equal, seeds_checked, prefixes, kB, at_end);
  // a whole-table call for a planner forgets its streaming source: raw tables from now on
  {
    std::vector<double> q, J;
    CHECK(whole.GetIkTable(0, &q, &J).ok());
    IkTables t;
    t.ik_positions.assign(q.begin(), q.begin() + (size_t)kN * D);
    t.jacobians.assign(J.begin(), J.begin() + (size_t)kN * 6 * D);
    t.row_offsets = {0, kN};
    t.path_end = {1e9};                       // far away: the first Plan must run past row N - 1
    t.max_translational_velocity = {lim.max_translational_velocity[0]};
    t.max_rotational_velocity = {lim.max_rotational_velocity[0]};
    t.delta = {kDelta};
    t.max_velocity.assign(lim.max_velocity[0].begin(), lim.max_velocity[0].end());
    t.max_acceleration.assign(lim.max_acceleration[0].begin(), lim.max_acceleration[0].end());
    stream.Reset(0);
    CHECK(stream.SetIkTables({0}, t).ok());
    const int before = calls;
    const auto st = stream.PlanStreaming(FromUnixNanos(0), Milliseconds(60000));
    CHECK(!st[0].ok() && calls == before);    // nothing extends it: no stale splines, no IK call
    std::printf("SetIkTables after a streaming goal: the planner's splines are forgotten\n");
  }
}

int main() {
  Scenario(7, false);
  Scenario(6, true);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

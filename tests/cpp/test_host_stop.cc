// GPU test of GetPathStopParameter in the host mirror (run by tests/test_gpu_fastest_stop.py):
// PathTimingTrajectory::GetPathStopParameter (host) on the reference's own cases, and
// PathTimingTrajectorySet::GetPathStopParameters (one kernel launch over the resident
// trajectories) against one mirror planner per set member, driven identically.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::StatusCode;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static Time TimeFromSec(double s) { return FromUnixNanos((int64_t)(s * 1e9)); }
static VectorXd V3(double x, double y, double z) { VectorXd v(3); v[0] = x; v[1] = y; v[2] = z; return v; }
static bool SameBits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// path_timing_trajectory_test.cc:942-992 (GetPathStopParameterWorksInSimpleCase)
static void TestSimpleCase(Method method) {
  const int D = 3, N = 500;
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_constraint_safety(1.0).set_num_path_samples(N));
  PathTimingTrajectory planner(PathTimingTrajectoryOptions().SetTimeStep(Milliseconds(1)).SetNumDofs(D)
                                   .SetNumPathSamples(N).SetTimeSamplingMethod(method));
  std::vector<double> vmax(D, 1.0), amax(D, 2.0);
  const std::vector<VectorXd> wps = {V3(0, 0, 0), V3(1, 1, 1), V3(2, 2, 2)};
  CHECK(planner.SetPath(path).ok());
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  // no plan yet: the beginning of the path
  auto before = planner.GetPathStopParameter(TimeFromSec(0.0));
  CHECK(before.ok() && *before == 0.0);
  Time start = TimeFromSec(0.0);
  CHECK(planner.Plan(start, Milliseconds(750)).ok());
  auto stop = planner.GetPathStopParameter(start);
  CHECK(stop.ok());
  std::vector<double> s = planner.GetPathParameters();
  const int stop_index = (int)(std::upper_bound(s.begin(), s.end(), *stop) - s.begin());
  CHECK(stop_index <= 3);
  const double last = planner.GetTime().back();
  stop = planner.GetPathStopParameter(TimeFromSec(last));
  CHECK(stop.ok() && *stop == s.back());
  CHECK(std::upper_bound(s.begin(), s.end(), *stop) == s.end());
  auto after = planner.GetPathStopParameter(TimeFromSec(last + 1.0));
  CHECK(!after.ok() && after.status().code() == StatusCode::kInvalidArgument);
  std::printf("simple case (%s): stop index %d at the start\n",
              method == Method::kUniformlyInTime ? "uniform" : "skip", stop_index);
}

// path_timing_trajectory_test.cc:298-420 (SwitchToNewJointWaypointPathWorks) with the real stop
// parameter: plan until the robot moves at a good fraction of its velocity limit, switch to new
// waypoints at the point it could stop at, keep planning to the end.
static void TestSwitchAtStopParameter(Method method) {
  const int D = 3, N = 1000;
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(0.001));
  PathTimingTrajectory planner(PathTimingTrajectoryOptions().SetTimeStep(Milliseconds(4)).SetNumDofs(D)
                                   .SetNumPathSamples(N).SetTimeSamplingMethod(method));
  const std::vector<VectorXd> wps = {V3(1, 2, 3), V3(-1, -2, -3), V3(0.5, 1.0, 1.5)};
  const std::vector<VectorXd> new_wps = {V3(1, 2, 3), V3(0.5, 1.0, 5.5)};
  std::vector<double> vmax(D, 1.0), amax(D, 2.0);
  CHECK(planner.SetPath(path).ok());
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  Time start = TimeFromSec(0.0);
  for (int loop = 0; !planner.IsTrajectoryAtEnd() && loop < 100; loop++) {
    CHECK(planner.Plan(start, Milliseconds(750)).ok());
    start = planner.GetNextPlanStartTime(start + Milliseconds(200));
    double closest = 1e300;     // stop after reaching a significant fraction of the velocity limit
    for (int d = 0; d < D; d++) closest = std::min(closest, std::fabs(std::fabs(planner.GetVelocities().front()[d]) - vmax[d]));
    if (closest < 0.3) break;
  }
  CHECK(!planner.IsTrajectoryAtEnd());
  auto stop = planner.GetPathStopParameter(start);
  CHECK(stop.ok());
  if (!stop.ok()) return;
  // the robot's velocity at the next start (the sample at or after it)
  const std::vector<double> &t = planner.GetTime();
  const double start_sec = (double)tpamd::compat::ToUnixNanos(start) / 1e9;
  const size_t k = std::lower_bound(t.begin(), t.end(), start_sec) - t.begin();
  CHECK(k < t.size());
  const VectorXd v_now = planner.GetVelocities()[std::min(k, t.size() - 1)];
  // the stop parameter lies ahead of the robot and before the old path's end
  CHECK(*stop >= planner.GetPathParameters()[std::min(k, t.size() - 1)]);
  CHECK(*stop < path->knots().back());
  CHECK(path->SwitchToWaypointPath(*stop, {new_wps.data(), new_wps.size()}).ok());
  CHECK(path->SetInitialVelocity({v_now.data(), v_now.size()}).ok());
  int loops = 0;
  while (!planner.IsTrajectoryAtEnd() && loops < 200) {
    const bool ok = planner.Plan(start, Milliseconds(750)).ok();
    CHECK(ok);
    if (!ok) break;
    start = planner.GetNextPlanStartTime(start + Milliseconds(200));
    loops++;
  }
  CHECK(planner.IsTrajectoryAtEnd());
  for (int d = 0; d < D; d++) {
    CHECK(std::fabs(planner.GetPositions().back()[d] - new_wps.back()[d]) < 1e-10);
    CHECK(planner.GetVelocities().back()[d] == 0.0);
  }
  std::printf("switch at the stop parameter (%s): s_stop %.6f, %d plans after the switch\n",
              method == Method::kUniformlyInTime ? "uniform" : "skip", *stop, loops);
}

static std::shared_ptr<TimeableJointSplinePath> RandomPath(int D, int N, int W, double fraction,
                                                           unsigned long long *seed) {
  auto rnd = [&]() { *seed = *seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(*seed >> 11) / 9007199254740992.0; };
  std::vector<VectorXd> wps;
  for (int i = 0; i < W; i++) { VectorXd v(D); for (int d = 0; d < D; d++) v[d] = 5.0 * rnd() - 2.5; wps.push_back(v); }
  auto probe = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
  probe->SetWaypoints({wps.data(), wps.size()});
  const double delta = fraction * probe->knots().back() / (N - 1);
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta));
  std::vector<double> vmax(D), amax(D);
  for (int d = 0; d < D; d++) { vmax[d] = 1.0 + rnd(); amax[d] = 2.0 + 2.0 * rnd(); }
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  return path;
}

// A set of planners against one mirror planner each: after every Plan, GetPathStopParameters
// at times before, on, between and after the samples must equal the mirrors' answers bit for bit.
static void TestSetAgainstMirrors(Method method) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, K = 256, D = 7, N = 300, W = 5, P = 3 * W - 2;   // planners K..B-1 never get a path
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet set(opt, B, P);
  CHECK(set.status().ok());
  if (!set.status().ok()) return;
  unsigned long long seed = skip ? 4242 : 777;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(K);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < K; b++) paths[b] = RandomPath(D, N, W, 0.3 + 0.4 * (b % 7) / 7.0, &seed);
  CHECK(set.SetPaths(paths).ok());
  for (int b = 0; b < B; b++) {
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    if (b < K) CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  std::vector<bool> planned(B, false);    // false: left out of the mirrors' PlanBatch
  for (int b = 0; b < K; b++) planned[b] = true;
  int compared = 0, mid = 0, invalid = 0, unplanned = 0;
  auto compare = [&](int round, const std::vector<Time> &times) {
    const auto got = set.GetPathStopParameters(times);
    CHECK(got.size() == (size_t)B);
    for (int b = 0; b < B; b++) {
      const auto want = mirrors[b]->GetPathStopParameter(times[b]);
      CHECK(got[b].ok() == want.ok());
      if (got[b].ok() != want.ok()) { std::printf("  planner %d round %d: status differs\n", b, round); continue; }
      if (!want.ok()) { CHECK(got[b].status().code() == want.status().code()); invalid++; continue; }
      CHECK(SameBits(*got[b], *want));
      if (!SameBits(*got[b], *want)) std::printf("  planner %d round %d: %.17g vs %.17g\n", b, round, *got[b], *want);
      const auto one = set.GetPathStopParameter(b, times[b]);
      if (b % 37 == 0) CHECK(one.ok() && SameBits(*one, *want));
      if (mirrors[b]->GetNumTimeSamples() == 0) unplanned++;
      else if (*want != mirrors[b]->GetPathParameters().back()) mid++;
      compared++;
    }
  };
  int64_t start = 2000 * kMs;
  for (int round = 0; round < 8; round++) {
    const int64_t horizon = round == 5 ? (int64_t)100000 * kMs : 500 * kMs;
    const auto st = set.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    std::vector<PathTimingTrajectory *> batch;
    std::vector<int> ids;
    for (int b = 0; b < K; b++) if (planned[b]) { batch.push_back(mirrors[b].get()); ids.push_back(b); }
    const auto ms = PathTimingTrajectory::PlanBatch(batch, FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    for (size_t i = 0; i < ids.size(); i++) {
      CHECK(st[ids[i]].code() == ms[i].code());
      CHECK(set.GetNumTimeSamples(ids[i]) == mirrors[ids[i]]->GetNumTimeSamples());
    }
    // query times: per planner one of the start, a sample, between two samples, the last sample,
    // after the end, before the trajectory
    std::vector<Time> times(B);
    for (int b = 0; b < B; b++) {
      const std::vector<double> &t = mirrors[b]->GetTime();
      const int kind = (b + round) % 6;
      double q = (double)start / 1e9;
      if (!t.empty()) {
        const size_t i = (size_t)((b * 7919 + round * 104729) % t.size());
        if (kind == 1) q = t[i];
        else if (kind == 2 && i + 1 < t.size()) q = 0.5 * (t[i] + t[i + 1]);
        else if (kind == 3) q = t.back();
        else if (kind == 4) q = t.back() + 0.01;
        else if (kind == 5) q = t.front() - 0.5;
      }
      times[b] = TimeFromSec(q);
    }
    compare(round, times);
    if (round == 3) {        // two planners are Reset: no plan, 0.0 (path_timing_trajectory.cc:239-242)
      for (int b : {5, 77}) {
        set.Reset(b);
        mirrors[b]->Reset();
        planned[b] = false;
      }
      compare(round, times);
    }
    start += round >= 5 ? 3000 * kMs : 150 * kMs;
  }
  int at_end = 0;
  for (int b = 0; b < K; b++) at_end += planned[b] && mirrors[b]->IsTrajectoryAtEnd();
  CHECK(at_end > K / 2);
  CHECK(mid > 0 && invalid > 0 && unplanned > 0);
  std::printf("set vs mirrors (%s): %d answers bit-equal (%d inside the trajectory), %d out of range, "
              "%d planners without a plan, %d at the end\n",
              skip ? "skip" : "uniform", compared, mid, invalid, unplanned, at_end);
}

// A stop query between two Plan calls changes nothing the next Plan computes.
static void TestQueryLeavesPlansUnchanged() {
  const int B = 8, D = 7, N = 300, W = 5, P = 3 * W - 2;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(1));
  PathTimingTrajectorySet a(opt, B, P), b(opt, B, P);
  CHECK(a.status().ok() && b.status().ok());
  unsigned long long seed = 99;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  for (int k = 0; k < B; k++) paths[k] = RandomPath(D, N, W, 0.4, &seed);
  CHECK(a.SetPaths(paths).ok() && b.SetPaths(paths).ok());
  int64_t start = 1000 * kMs;
  for (int round = 0; round < 4; round++) {
    a.Plan(FromUnixNanos(start), Milliseconds(400));
    b.Plan(FromUnixNanos(start), Milliseconds(400));
    std::vector<Time> times(B, FromUnixNanos(start + 50 * kMs));
    a.GetPathStopParameters(times);
    a.GetPathStopParameter(3, FromUnixNanos(start));
    start += 150 * kMs;
  }
  a.Plan(FromUnixNanos(start), Milliseconds(400));
  b.Plan(FromUnixNanos(start), Milliseconds(400));
  for (int k = 0; k < B; k++) {
    PlannedTrajectory ta, tb;
    CHECK(a.GetTrajectory(k, &ta).ok() && b.GetTrajectory(k, &tb).ok());
    CHECK(ta.time.size() > 0 && ta.time == tb.time && ta.path_parameter == tb.path_parameter);
    CHECK(ta.positions == tb.positions && ta.velocities == tb.velocities && ta.accelerations == tb.accelerations);
  }
}

// Call-level errors of the set entry: a bad id fails the whole call before anything runs.
static void TestSetErrors() {
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(3).SetNumPathSamples(100).SetTimeStep(Milliseconds(1));
  PathTimingTrajectorySet set(opt, 4, 5);
  CHECK(set.status().ok());
  CHECK(!set.GetPathStopParameter(4, FromUnixNanos(0)).ok());
  CHECK(set.GetPathStopParameters(std::vector<Time>(3)).size() == 4);
  CHECK(!set.GetPathStopParameters(std::vector<Time>(3))[0].ok());
  auto fresh = set.GetPathStopParameters(std::vector<Time>(4, FromUnixNanos(0)));
  for (auto &r : fresh) CHECK(r.ok() && *r == 0.0);
  // the C-ABI: every id is checked before anything runs
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) return;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = 4; cfg.num_dofs = 3; cfg.num_samples = 100; cfg.num_points = 5;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = kMs;
  tpamd_planner_set *ps = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &ps) == 0);
  if (ps) {
    const int32_t good[2] = {0, 3}, bad[2] = {1, 4}, neg[1] = {-1};
    const int64_t t[2] = {0, 0};
    double s[2] = {-1.0, -1.0}, dur[2];
    int32_t st[2] = {-1, -1};
    CHECK(tpamd_planner_set_stop_parameters(ps, 2, bad, t, s, dur, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(st[0] == -1 && s[0] == -1.0);                   // nothing was written
    CHECK(tpamd_planner_set_stop_parameters(ps, 1, neg, t, s, dur, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_parameters(ps, 5, nullptr, t, s, dur, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_parameters(ps, 2, good, nullptr, s, dur, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_parameters(ps, 2, good, t, s, nullptr, st) == 0);
    CHECK(st[0] == TPAMD_PLAN_OK && st[1] == TPAMD_PLAN_OK && s[0] == 0.0 && s[1] == 0.0);
    tpamd_planner_set_destroy(ps);
  }
  tpamd_engine_destroy(e);
}

int main() {
  for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) {
    TestSimpleCase(m);
    TestSwitchAtStopParameter(m);
    TestSetAgainstMirrors(m);
  }
  TestQueryLeavesPlansUnchanged();
  TestSetErrors();
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("%d CHECKS FAILED\n", g_fail);
  return g_fail == 0 ? 0 : 1;
}

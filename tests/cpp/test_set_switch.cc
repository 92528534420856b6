// GPU test of the planner-set path switch (run by tests/test_gpu_set_switch.py):
// PathTimingTrajectorySet::SwitchToWaypointPaths (tpamd_planner_set_switch_paths: stop parameter,
// velocity at the switch time and the spline edit on the device) against one mirror planner per
// set member running the reference's flow (path_timing_trajectory_test.cc:298-420):
//   GetPathStopParameter(t) -> path->SwitchToWaypointPath(stop, waypoints) ->
//   path->SetInitialVelocity(GetVelocityAtTime(t)) -> Plan.
// At every Plan each planner's status, summary, trajectory and resident spline must equal its
// mirror's bit for bit. A few planners are also followed by the oracle's planner (tp_oracle.h) on
// the mirror's spline. The set starts with paths of different sizes (SetPaths with any P) and a
// per-planner capacity below them; repeated switches grow it further. Also: call-level errors and
// per-planner failures leave the planners unchanged.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static std::vector<VectorXd> RandomWaypoints(int W, int D) {
  std::vector<VectorXd> w;
  for (int i = 0; i < W; i++) {
    VectorXd v(D);
    for (int d = 0; d < D; d++) v[d] = 5.0 * Rnd() - 2.5;
    w.push_back(v);
  }
  return w;
}

static std::shared_ptr<TimeableJointSplinePath> RandomPath(int D, int N, int W, double fraction) {
  std::vector<VectorXd> wps = RandomWaypoints(W, D);
  auto probe = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
  probe->SetWaypoints({wps.data(), wps.size()});
  const double delta = fraction * probe->knots().back() / (N - 1);
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta));
  std::vector<double> vmax(D), amax(D);
  for (int d = 0; d < D; d++) { vmax[d] = 1.0 + Rnd(); amax[d] = 2.0 + 2.0 * Rnd(); }
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  return path;
}

static void CompareOracle(const PathTimingTrajectory &m, const tpo_planner *o, int D) {
  const int M = tpo_planner_num_samples(o);
  CHECK((int)m.GetTime().size() == M);
  if ((int)m.GetTime().size() != M) return;
  int bad = 0;
  for (int i = 0; i < M; i++) {
    bad += m.GetTime()[i] != tpo_planner_time(o)[i];
    bad += m.GetPathParameters()[i] != tpo_planner_path_parameter(o)[i];
    for (int d = 0; d < D; d++) {
      bad += m.GetPositions()[i][d] != tpo_planner_positions(o)[(size_t)i * D + d];
      bad += m.GetVelocities()[i][d] != tpo_planner_velocities(o)[(size_t)i * D + d];
    }
  }
  CHECK(bad == 0);
  CHECK(ToUnixNanos(m.GetEndTime()) == tpo_planner_end_time(o));
}

static void TestSwitchAgainstMirrors(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, P0 = 3 * 3 - 2;     // capacity to start with: below most paths
  g_seed = 1000 + D * 7 + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet set(opt, B, P0);
  CHECK(set.status().ok());
  if (!set.status().ok()) return;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) paths[b] = RandomPath(D, N, RndInt(3, 7), 0.3 + 0.4 * (b % 7) / 7.0);
  CHECK(set.SetPaths(paths).ok());                 // paths of 7 .. 19 control points
  for (int b = 0; b < B; b++) {
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  const int kOracle[3] = {0, 101, 259};
  std::vector<tpo_planner *> oracle;
  for (int b : kOracle) {
    tpo_planner *o = tpo_planner_create(D, N, paths[b]->GetPathSamplingDistance(), paths[b]->options().constraint_safety(),
                                        opt.GetTimeStep().nanos(), skip ? 1 : 0, opt.GetMaxPlanningIterations(),
                                        opt.GetMaxInitialVelocityError());
    tpo_planner_set_limits(o, paths[b]->GetMaxJointVelocity().data(), paths[b]->GetMaxJointAcceleration().data());
    tpo_planner_set_spline(o, paths[b]->knots().data(), (int)paths[b]->knots().size(),
                           paths[b]->packed_control_points().data(), paths[b]->num_control_points(), TPO_PATH_NEW);
    oracle.push_back(o);
  }
  std::vector<bool> diverged(B, false);   // compared no further (a failed mirror edit or first window)
  std::vector<int> last_switch(B, -1);   // the mirror's path edit failed after changing its state
  int64_t start = 2000 * kMs;
  int switched = 0, failed = 0, compared = 0, max_points = 0, plans = 0, reported = 0, failed_plans = 0;
  for (int round = 0; round < 14; round++) {
    const bool to_end = round >= 9;
    const int64_t horizon = to_end ? (int64_t)100000 * kMs : 500 * kMs;
    const auto st = set.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    std::vector<PathTimingTrajectory *> batch;
    for (int b = 0; b < B; b++) batch.push_back(mirrors[b].get());
    const auto ms = PathTimingTrajectory::PlanBatch(batch, FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    plans++;
    for (size_t i = 0; i < oracle.size(); i++) {
      const int b = kOracle[i];
      const int rc = tpo_planner_plan(oracle[i], start, horizon);
      if (diverged[b]) continue;
      CHECK((rc == TPO_PLAN_OK) == ms[b].ok());
      if (rc == TPO_PLAN_OK && ms[b].ok()) CompareOracle(*mirrors[b], oracle[i], D);
    }
    for (int b = 0; b < B; b++) {
      if (diverged[b]) continue;
      CHECK(st[b].code() == ms[b].code());
      const int bad = CompareOne(set, b, *mirrors[b], paths[b].get()) |
                      (set.NumControlPoints(b) != (size_t)paths[b]->num_control_points()) << 14;
      CHECK(bad == 0);
      if (bad && ++reported <= 12)
        std::printf("  D %d %s round %d planner %d: differences 0x%x (status %d / mirror %d '%s', samples %zu / %zu, "
                    "windows %d, switched in round %d, P %d)\n", D, skip ? "skip" : "uniform", round, b, bad,
                    (int)st[b].code(), (int)ms[b].code(), ms[b].message().c_str(), set.GetNumTimeSamples(b),
                    mirrors[b]->GetNumTimeSamples(), set.WindowsOfLastPlan(b), last_switch[b], paths[b]->num_control_points());
      compared++;
      // A Plan whose first window of a new or modified path fails (here: the start velocity does not
      // fit the new path's tangent, :387-392) leaves the path sampled on the device, as the
      // reference's SamplePath does, but not in the mirror, which adopts samples only from a solved
      // window. The two part ways from then on: such planners are compared no further.
      if (ms[b].code() == StatusCode::kInvalidArgument && st[b].code() == StatusCode::kInvalidArgument) {
        diverged[b] = true;
        failed_plans++;
      }
    }
    const int64_t next = start + 150 * kMs;
    if (!to_end && round % 2 == 1) {
      // a seeded subset switches at its stop parameter at the next start time, W = 1..6
      std::vector<size_t> ids;
      std::vector<Time> times;
      std::vector<std::vector<VectorXd>> wps;
      for (int b = 0; b < B; b++) {
        if (diverged[b] || Rnd() > 0.4) continue;
        ids.push_back(b);
        times.push_back(FromUnixNanos(next));
        wps.push_back(RandomWaypoints(RndInt(1, 6), D));
      }
      const auto got = set.SwitchToWaypointPaths(ids, times, wps);
      CHECK(got.size() == ids.size());
      for (size_t k = 0; k < ids.size(); k++) {
        const int b = (int)ids[k];
        PathTimingTrajectory &m = *mirrors[b];
        auto stop = m.GetPathStopParameter(times[k]);
        StatusCode want = StatusCode::kOk;
        if (!stop.ok()) {
          want = stop.status().code();
        } else {
          const auto v = m.GetVelocityAtTime(times[k]);
          if (!v.ok()) want = v.status().code();
          else {
            const auto e = paths[b]->SwitchToWaypointPath(*stop, {wps[k].data(), wps[k].size()});
            if (!e.ok()) {
              want = e.code();
              diverged[b] = true;      // the mirror's path state changed anyway
            } else {
              CHECK(paths[b]->SetInitialVelocity({(*v).data(), (*v).size()}).ok());
            }
          }
        }
        CHECK(got[k].code() == want);
        if (got[k].code() != want) std::printf("  planner %d: switch status %d vs %d\n", b, (int)got[k].code(), (int)want);
        if (want == StatusCode::kOk) {
          switched++;
          last_switch[b] = round;
          max_points = std::max(max_points, paths[b]->num_control_points());
          std::vector<double> kn, cp;
          CHECK(set.GetPath(b, &kn, &cp).ok());
          CHECK(SameBits(kn, paths[b]->knots()) && SameBits(cp, paths[b]->packed_control_points()));
          for (size_t i = 0; i < oracle.size(); i++)
            if (kOracle[i] == b) {
              tpo_planner_set_spline(oracle[i], paths[b]->knots().data(), (int)paths[b]->knots().size(),
                                     paths[b]->packed_control_points().data(), paths[b]->num_control_points(),
                                     TPO_PATH_MODIFIED);
              tpo_planner_set_initial_velocity(oracle[i], paths[b]->GetInitialVelocity().data());
            }
        } else {
          failed++;
        }
      }
    }
    start = to_end ? start + 3000 * kMs : next;
  }
  int at_end = 0, div = 0;
  for (int b = 0; b < B; b++) {
    at_end += mirrors[b]->IsTrajectoryAtEnd() && !diverged[b];
    div += diverged[b];
  }
  CHECK(switched > B / 2);
  CHECK(max_points > 2 * P0);
  CHECK(at_end > B / 2);
  CHECK(div < B / 2);
  for (auto *o : oracle) tpo_planner_destroy(o);
  std::printf("switch vs mirrors (D %d, %s): %d plans, %d planner states bit-equal, %d switches (%d failed alike), "
              "largest P %d (capacity started at %d), %d at the end, %d left out after a failed mirror edit or first window "
              "(%d plans failed alike)\n",
              D, skip ? "skip" : "uniform", plans, compared, switched, failed, max_points, P0, at_end, div, failed_plans);
}

// Call-level errors change nothing; per-planner failures leave those planners unchanged; planners
// that are not listed are untouched; a keep_path_until array replaces the stop query.
static void TestSwitchErrors() {
  const int B = 6, D = 3, N = 200;
  g_seed = 77;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(1));
  PathTimingTrajectorySet set(opt, B, 7), twin(opt, B, 7);
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  for (int b = 0; b < B; b++) paths[b] = RandomPath(D, N, 4, 0.5);
  CHECK(set.SetPaths(paths).ok() && twin.SetPaths(paths).ok());
  auto same_paths = [&]() {
    for (int b = 0; b < B; b++) {
      std::vector<double> k1, c1, k2, c2;
      CHECK(set.GetPath(b, &k1, &c1).ok() && twin.GetPath(b, &k2, &c2).ok());
      if (!SameBits(k1, k2) || !SameBits(c1, c2)) return false;
    }
    return true;
  };
  // before any plan: FAILED_PRECONDITION per planner, nothing changes
  const int64_t t0 = 1000 * kMs;
  std::vector<std::vector<VectorXd>> wps = {RandomWaypoints(3, D), RandomWaypoints(2, D)};
  auto r = set.SwitchToWaypointPaths({0, 1}, {FromUnixNanos(t0), FromUnixNanos(t0)}, wps);
  CHECK(r.size() == 2 && r[0].code() == StatusCode::kFailedPrecondition && r[1].code() == StatusCode::kFailedPrecondition);
  CHECK(same_paths());
  set.Plan(FromUnixNanos(t0), Milliseconds(400));
  twin.Plan(FromUnixNanos(t0), Milliseconds(400));
  PlannedTrajectory tr;
  CHECK(set.GetTrajectory(2, &tr).ok() && !tr.time.empty());
  const int64_t after_end = (int64_t)llround(tr.time.back() * 1e9) + 50 * kMs;
  // the C-ABI's call-level errors
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 10;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = kMs;
  tpamd_planner_set *ps = nullptr;
  if (e) CHECK(tpamd_planner_set_create(e, &cfg, &ps) == 0);
  if (ps) {
    const int32_t dup[2] = {1, 1}, bad[2] = {0, 6}, good[2] = {0, 1}, off_bad[3] = {0, 3, 2}, off_ok[3] = {0, 1, 2},
                  off_nz[3] = {1, 2, 3};
    const int64_t t[2] = {t0, t0};
    double w[9] = {0}, stop[2] = {-1, -1};
    int32_t np[2] = {-1, -1}, st[2] = {-9, -9};
    CHECK(tpamd_planner_set_switch_paths(ps, 2, dup, t, nullptr, off_ok, w, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_switch_paths(ps, 2, bad, t, nullptr, off_ok, w, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_switch_paths(ps, 2, good, t, nullptr, off_ok, nullptr, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_switch_paths(ps, 2, good, t, nullptr, off_bad, w, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_switch_paths(ps, 2, good, t, nullptr, off_nz, w, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_switch_paths(ps, 7, nullptr, t, nullptr, off_ok, w, stop, np, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(st[0] == -9 && np[0] == -1 && stop[0] == -1);      // nothing was written
    // no path: FAILED_PRECONDITION; the download reports no path
    CHECK(tpamd_planner_set_switch_paths(ps, 2, good, t, nullptr, off_ok, w, stop, np, st) == 0);
    CHECK(st[0] == TPAMD_PLAN_FAILED_PRECONDITION && st[1] == TPAMD_PLAN_FAILED_PRECONDITION);
    int32_t n = -1;
    CHECK(tpamd_planner_set_download_path(ps, 0, &n, nullptr, nullptr, 0) == 0 && n == 0);
    tpamd_planner_set_destroy(ps);
  }
  if (e) tpamd_engine_destroy(e);
  // mirror-level: a bad id fails the whole call
  auto rb = set.SwitchToWaypointPaths({0, 9}, {FromUnixNanos(t0), FromUnixNanos(t0)}, wps);
  CHECK(rb.size() == 2 && rb[0].code() == StatusCode::kInvalidArgument);
  // a time after the end (stop query: INVALID_ARGUMENT), no waypoints (INVALID_ARGUMENT), a time
  // before the trajectory (velocity: OUT_OF_RANGE) -- all unchanged
  auto rt = set.SwitchToWaypointPaths({2, 3, 4}, {FromUnixNanos(after_end), FromUnixNanos(t0 + 100 * kMs), FromUnixNanos(t0 - 10 * kMs)},
                                      {RandomWaypoints(2, D), {}, RandomWaypoints(2, D)});
  CHECK(rt.size() == 3 && rt[0].code() == StatusCode::kInvalidArgument && rt[1].code() == StatusCode::kInvalidArgument &&
        rt[2].code() == StatusCode::kOutOfRange);
  CHECK(same_paths());
  // the next plan of the failed planners equals the twin's
  set.Plan(FromUnixNanos(t0 + 150 * kMs), Milliseconds(400));
  twin.Plan(FromUnixNanos(t0 + 150 * kMs), Milliseconds(400));
  for (int b = 0; b < B; b++) {
    PlannedTrajectory a, c;
    CHECK(set.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok());
    CHECK(SameBits(a.time, c.time) && SameBits(a.positions, c.positions) && SameBits(a.velocities, c.velocities));
  }
  // one planner switches; the others stay bit for bit as the twin's
  auto ro = set.SwitchToWaypointPaths({5}, {FromUnixNanos(t0 + 200 * kMs)}, {RandomWaypoints(3, D)});
  CHECK(ro.size() == 1 && ro[0].ok());
  set.Plan(FromUnixNanos(t0 + 200 * kMs), Milliseconds(400));
  twin.Plan(FromUnixNanos(t0 + 200 * kMs), Milliseconds(400));
  for (int b = 0; b < 5; b++) {
    PlannedTrajectory a, c;
    CHECK(set.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok());
    CHECK(SameBits(a.time, c.time) && SameBits(a.positions, c.positions) && SameBits(a.accelerations, c.accelerations));
    std::vector<double> k1, c1, k2, c2;
    CHECK(set.GetPath(b, &k1, &c1).ok() && twin.GetPath(b, &k2, &c2).ok() && SameBits(k1, k2) && SameBits(c1, c2));
  }
  CHECK(set.NumControlPoints(5) != twin.NumControlPoints(5));
  std::printf("switch errors: ok\n");
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) TestSwitchAgainstMirrors(m, D);
  TestSwitchErrors();
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("%d CHECKS FAILED\n", g_fail);
  return g_fail == 0 ? 0 : 1;
}

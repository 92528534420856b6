// Online path switch of a planner set, run on the GPU machine (g++ -O2 -std=c++17 -ffp-contract=off
// tools/switch_bench.cc -L<host> -ltp_host -L<csrc> -ltpamd; argv: planners, trials). 1024 planners x 7 joints, 10 waypoints, N = 1000 path samples, 4 ms
// time step; after one Plan(t0, 750 ms) every planner switches at t0 + 200 ms to 4 new waypoints.
//   device  PathTimingTrajectorySet::SwitchToWaypointPaths: stop parameter, velocity and spline
//           edit on the device (tpamd_planner_set_switch_paths)
//   host    the flow without it: GetTrajectory per planner, FastestStopAtTime + GetVelocityAtTime
//           + TimeableJointSplinePath::SwitchToWaypointPath on the host, then SetPaths
// Both start from the same resident state (SetPaths of the original paths between trials leaves the
// trajectories alone), and must give the same splines. Then the Plan(t0 + 200 ms, 750 ms) after the
// switch, and a first Plan of a mixed-P set (W = 5..15, P = 13..43) against a uniform-P set
// (W = 10, P = 28). One JSON line; times are medians over the trials, host clock around each call.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/fastest_stop.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"

#define BENCH_SUPPORT_SEED 20261015
#include "bench_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

static std::vector<VectorXd> waypoints(int W, int D) {
  std::vector<VectorXd> w;
  for (int i = 0; i < W; i++) {
    VectorXd v(D);
    for (int d = 0; d < D; d++) v[d] = 4.0 * rnd() - 2.0;
    w.push_back(v);
  }
  return w;
}
static std::shared_ptr<TimeableJointSplinePath> make_path(int D, int N, int W) {
  auto p = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(0.01));
  std::vector<double> vmax(D), amax(D);
  for (int d = 0; d < D; d++) { vmax[d] = 1.0 + rnd(); amax[d] = 2.0 + 2.0 * rnd(); }
  p->SetMaxJointVelocity({vmax.data(), vmax.size()});
  p->SetMaxJointAcceleration({amax.data(), amax.size()});
  const auto w = waypoints(W, D);
  p->SetWaypoints({w.data(), w.size()});
  return p;
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int D = 7, N = 1000, W = 10, Wnew = 4, trials = argc > 2 ? std::atoi(argv[2]) : 5;
  const int64_t kMs = 1000000, t0 = 1000 * kMs, ts = t0 + 200 * kMs;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  std::vector<std::shared_ptr<TimeableJointSplinePath>> orig(B);
  for (int b = 0; b < B; b++) orig[b] = make_path(D, N, W);
  std::vector<std::vector<VectorXd>> new_wps(B);
  for (int b = 0; b < B; b++) new_wps[b] = waypoints(Wnew, D);
  std::vector<size_t> ids(B);
  for (int b = 0; b < B; b++) ids[b] = b;
  const std::vector<Time> times(B, FromUnixNanos(ts));

  PathTimingTrajectorySet set(opt, B, 3 * W - 2);
  if (!set.status().ok()) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  set.SetPaths(orig);
  set.Plan(FromUnixNanos(t0), Milliseconds(750));
  std::vector<double> t_dev, t_host;
  int ok_dev = 0, equal = 0;
  for (int trial = 0; trial < trials; trial++) {
    set.SetPaths(orig);                        // the same spline before every switch; trajectories stay
    double a = now();
    const auto st = set.SwitchToWaypointPaths(ids, times, new_wps);
    t_dev.push_back(now() - a);
    ok_dev = 0;
    for (const auto &s : st) ok_dev += s.ok();
    std::vector<std::vector<double>> dk(B), dc(B);
    if (trial == 0)
      for (int b = 0; b < B; b++) set.GetPath(b, &dk[b], &dc[b]);
    // the host flow from the same state
    set.SetPaths(orig);
    std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
    for (int b = 0; b < B; b++) paths[b] = std::make_shared<TimeableJointSplinePath>(*orig[b]);
    a = now();
    for (int b = 0; b < B; b++) {
      PlannedTrajectory tr;
      set.GetTrajectory(b, &tr);
      const int n = (int)tr.time.size();
      double stop = 0, dur = 0;
      int idx = 0;
      const double q = (double)ts / 1e9;
      FastestStopAtTime(n, D, tr.time.data(), tr.path_parameter.data(), tr.velocities.data(), tr.accelerations.data(),
                        paths[b]->GetMaxJointAcceleration().data(), q, &stop, &idx, &dur, nullptr);
      // GetVelocityAtTime on the downloaded samples
      const size_t u = std::upper_bound(tr.time.begin(), tr.time.end(), q) - tr.time.begin();
      std::vector<double> v(D);
      for (int d = 0; d < D; d++) {
        if (u == tr.time.size()) { v[d] = tr.velocities[(u - 1) * D + d]; continue; }
        const double f = (q - tr.time[u - 1]) / (tr.time[u] - tr.time[u - 1]);
        const double lo = tr.velocities[(u - 1) * D + d], hi = tr.velocities[u * D + d];
        v[d] = lo + f * (hi - lo);
      }
      paths[b]->SwitchToWaypointPath(stop, {new_wps[b].data(), new_wps[b].size()});
      paths[b]->SetInitialVelocity({v.data(), v.size()});
    }
    set.SetPaths(paths);
    t_host.push_back(now() - a);
    if (trial == 0)
      for (int b = 0; b < B; b++)
        equal += dk[b] == paths[b]->knots() && dc[b] == paths[b]->packed_control_points();
  }
  // the Plan after the switch
  set.SetPaths(orig);
  set.SwitchToWaypointPaths(ids, times, new_wps);
  double a = now();
  set.Plan(FromUnixNanos(ts), Milliseconds(750));
  const double t_plan_after = now() - a;
  int maxp = 0, minp = 1 << 30;
  for (int b = 0; b < B; b++) {
    maxp = std::max<int>(maxp, (int)set.NumControlPoints(b));
    minp = std::min<int>(minp, (int)set.NumControlPoints(b));
  }
  // first Plan of a uniform-P and a mixed-P set
  std::vector<double> t_uni, t_mix;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> mixed(B);
  for (int b = 0; b < B; b++) mixed[b] = make_path(D, N, 5 + b % 11);
  for (int trial = 0; trial < trials; trial++) {
    for (int kind = 0; kind < 2; kind++) {
      PathTimingTrajectorySet s(opt, B, 3 * W - 2);
      s.SetPaths(kind ? mixed : orig);
      a = now();
      s.Plan(FromUnixNanos(t0), Milliseconds(750));
      (kind ? t_mix : t_uni).push_back(now() - a);
    }
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"new_waypoints\": %d, \"trials\": %d, "
              "\"switch_device_ms\": %.3f, \"switch_host_flow_ms\": %.3f, \"speedup\": %.1f, \"switched_ok\": %d, "
              "\"splines_equal\": %d, \"points_after_switch\": [%d, %d], \"plan_after_switch_ms\": %.3f, "
              "\"first_plan_uniform_p_ms\": %.3f, \"first_plan_mixed_p_ms\": %.3f, "
              "\"switch_bytes_up_per_planner\": %d, \"switch_bytes_down_per_planner\": 16}\n",
              B, D, N, Wnew, trials, 1e3 * median(t_dev), 1e3 * median(t_host), median(t_host) / median(t_dev), ok_dev,
              equal, minp, maxp, 1e3 * t_plan_after, 1e3 * median(t_uni), 1e3 * median(t_mix), 16 + Wnew * D * 8);
  return 0;
}

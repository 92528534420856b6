// GetPathStopParameter for a fleet of planners (built and run by tools/gpu_stop_bench.py):
// PathTimingTrajectorySet::GetPathStopParameters (one launch over the resident trajectories)
// against the mirror's host GetPathStopParameter looped over the same planners on one thread.
// Prints one JSON line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/fastest_stop.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

using namespace trajectory_planning;
using Clock = std::chrono::steady_clock;

static double Median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024, D = 7, N = 400, W = 5, P = 3 * W - 2;
  const int reps = argc > 2 ? std::atoi(argv[2]) : 200;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(tpamd::compat::Milliseconds(1));
  PathTimingTrajectorySet set(opt, B, P);
  if (!set.status().ok()) { std::fprintf(stderr, "no set\n"); return 1; }
  unsigned long long seed = 2024;
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  std::vector<std::vector<double>> vmax(B, std::vector<double>(D));
  for (int b = 0; b < B; b++) {
    std::vector<VectorXd> wps;
    for (int i = 0; i < W; i++) { VectorXd v(D); for (int d = 0; d < D; d++) v[d] = 5.0 * rnd() - 2.5; wps.push_back(v); }
    auto probe = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
    probe->SetWaypoints({wps.data(), wps.size()});
    auto path = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N)
                                                              .set_delta_parameter(probe->knots().back() / (N - 1)));
    std::vector<double> amax(D);
    for (int d = 0; d < D; d++) { vmax[b][d] = 1.0 + rnd(); amax[d] = 2.0 + 2.0 * rnd(); }
    path->SetMaxJointVelocity({vmax[b].data(), (size_t)D});
    path->SetMaxJointAcceleration({amax.data(), amax.size()});
    path->SetWaypoints({wps.data(), wps.size()});
    paths[b] = path;
  }
  if (!set.SetPaths(paths).ok()) return 1;
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  std::vector<PathTimingTrajectory *> raw(B);
  for (int b = 0; b < B; b++) {
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    mirrors[b]->SetPath(paths[b]);
    raw[b] = mirrors[b].get();
  }
  const Time start = tpamd::compat::FromUnixNanos(1000000000LL);
  const auto horizon = tpamd::compat::Milliseconds(100000);   // the whole path: resampled at 1 ms
  set.Plan(start, horizon);
  PathTimingTrajectory::PlanBatch(raw, start, horizon);
  // per planner: the first sample at which some joint moves at >= 50 % of its velocity limit
  std::vector<Time> times(B);
  double mean_speed = 0.0;
  for (int b = 0; b < B; b++) {
    const auto &t = mirrors[b]->GetTime();
    const auto &v = mirrors[b]->GetVelocities();
    size_t i = 0;
    double ratio = 0.0;
    for (; i < t.size(); i++) {
      ratio = 0.0;
      for (int d = 0; d < D; d++) ratio = std::max(ratio, std::fabs(v[i][d]) / vmax[b][d]);
      if (ratio >= 0.5) break;
    }
    i = std::min(i, t.size() - 1);
    mean_speed += ratio / B;
    times[b] = tpamd::compat::FromUnixNanos((int64_t)std::ceil(t[i] * 1e9));
  }
  // braking length in samples (host function on the mirrors' trajectories)
  double mean_len = 0.0, mean_samples = 0.0;
  for (int b = 0; b < B; b++) {
    const auto &t = mirrors[b]->GetTime();
    const size_t n = t.size();
    std::vector<double> qd(n * D), qdd(n * D);
    for (size_t i = 0; i < n; i++)
      for (int d = 0; d < D; d++) { qd[i * D + d] = mirrors[b]->GetVelocities()[i][d]; qdd[i * D + d] = mirrors[b]->GetAccelerations()[i][d]; }
    double sp, dur;
    int idx;
    const double q = (double)tpamd::compat::ToUnixNanos(times[b]) / 1e9;
    FastestStopAtTime((int)n, D, t.data(), mirrors[b]->GetPathParameters().data(), qd.data(), qdd.data(),
                      paths[b]->GetMaxJointAcceleration().data(), q, &sp, &idx, &dur, nullptr);
    const int off = (int)(std::lower_bound(t.begin(), t.end(), q) - t.begin());
    mean_len += (double)(idx - off) / B;
    mean_samples += (double)n / B;
  }
  // equality, then timing
  auto got = set.GetPathStopParameters(times);
  int equal = 0;
  for (int b = 0; b < B; b++) {
    const auto want = mirrors[b]->GetPathStopParameter(times[b]);
    equal += got[b].ok() && want.ok() && std::memcmp(&*got[b], &*want, 8) == 0;
  }
  std::vector<double> set_us, host_us;
  for (int r = 0; r < reps; r++) {
    const auto t0 = Clock::now();
    got = set.GetPathStopParameters(times);
    set_us.push_back(std::chrono::duration<double, std::micro>(Clock::now() - t0).count());
  }
  double sink = 0.0;
  for (int r = 0; r < std::max(5, reps / 20); r++) {
    const auto t0 = Clock::now();
    for (int b = 0; b < B; b++) sink += *mirrors[b]->GetPathStopParameter(times[b]);
    host_us.push_back(std::chrono::duration<double, std::micro>(Clock::now() - t0).count());
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"time_step_ms\": 1, \"mean_trajectory_samples\": %.1f, "
              "\"mean_speed_fraction_at_query\": %.3f, \"mean_braking_samples\": %.2f, \"bit_equal\": %d, "
              "\"set_call_us_median\": %.1f, \"set_call_us_min\": %.1f, \"host_loop_us_median\": %.1f, "
              "\"speedup\": %.2f, \"checksum\": %.6f}\n",
              B, D, mean_samples, mean_speed, mean_len, equal, Median(set_us),
              *std::min_element(set_us.begin(), set_us.end()), Median(host_us), Median(host_us) / Median(set_us),
              sink);
  return equal == B ? 0 : 1;
}

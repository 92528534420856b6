// GPU test of a skip-method PathTimingTrajectorySet whose histories start above 32768 samples
// (run by tests/test_gpu_set_skip_long_mirror.py). The mirror's sets take the default history
// capacity, 8 * num_path_samples: with 4100 path samples that is 32800, more than the index list
// of the former resample kernel could hold, so the first Plan of such a set used to fail. Three
// planners (D = 3) with seeded waypoint paths some two windows long plan to their ends and replan
// twice; every Plan of the set must equal one mirror PathTimingTrajectory per planner, bit for bit.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

#define TEST_SUPPORT_SEED 20261019
#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::ToUnixNanos;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

int main() {
  const int B = 3, D = 3, N = 4100;
  const double delta = 0.002, rounding = 0.2;
  static_assert(8 * N > 32768, "the default history capacity must be above the former limit");
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(
      Method::kSkipSamplesCloserThanTimeStep);
  PathTimingTrajectorySet set(opt, B, 16);
  CHECK(set.status().ok());
  if (!set.status().ok()) {
    std::printf("FAILED: no set\n");
    return 1;
  }
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) {
    std::vector<VectorXd> wps;
    for (int i = 0; i < 4 + b; i++) {
      VectorXd v(D);
      for (int d = 0; d < D; d++) v[d] = 5.0 * Rnd() - 2.5;
      wps.push_back(v);
    }
    VectorXd vmax(D), amax(D);
    for (int d = 0; d < D; d++) {
      vmax[d] = 1.0 + Rnd();
      amax[d] = 2.0 + 2.0 * Rnd();
    }
    paths[b] = std::make_shared<TimeableJointSplinePath>(
        JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta).set_rounding(rounding));
    CHECK(paths[b]->SetWaypoints({wps.data(), wps.size()}).ok());
    CHECK(paths[b]->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
    CHECK(paths[b]->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  CHECK(set.SetPaths(paths).ok());
  int64_t start = 2000 * kMs;
  int compared = 0, windows = 0, skipped_some = 0;
  for (int round = 0; round < 3; round++) {
    const auto horizon = tpamd::compat::Nanoseconds((int64_t)100000 * kMs);
    const auto ss = set.Plan(FromUnixNanos(start), horizon);
    std::vector<PathTimingTrajectory *> batch;
    for (int b = 0; b < B; b++) batch.push_back(mirrors[b].get());
    const auto ms = PathTimingTrajectory::PlanBatch(batch, FromUnixNanos(start), horizon);
    for (int b = 0; b < B; b++) {
      CHECK(ss[b].ok() && ms[b].ok());
      const int bad = CompareOne(set, b, *mirrors[b]);
      CHECK(bad == 0);
      if (bad) std::printf("  round %d planner %d: differences 0x%x\n", round, b, bad);
      compared += bad == 0;
      windows += set.WindowsOfLastPlan(b);
      // more path samples than trajectory samples: the resampler dropped some
      skipped_some += set.GetNumTimeSamples(b) > 64 && (int)set.GetNumTimeSamples(b) < set.WindowsOfLastPlan(b) * N;
    }
    start += 150 * kMs;
  }
  CHECK(compared == 3 * B);
  CHECK(windows >= 2 * B);
  CHECK(skipped_some >= B);
  std::printf("skip-method set at history capacity %d: %d plans bit-equal to the mirrors, %d windows\n", 8 * N,
              compared, windows);
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("FAILED: %d checks\n", g_fail);
  return g_fail != 0;
}

// GPU test of discarding consumed IK rows through the host mirror (run by
// tests/test_gpu_cartesian_discard.py): PlanStreaming(start, horizon, /*discard=*/true) equals
// PlanStreaming without the flag, bit for bit at every step until every planner is at its end, over
// both families (sampling methods) of tests/cpp/test_cartesian_stream_mirror_gpu.cc, whose paths,
// split-dependent IK callback and comparison helpers are included. Both sets are also held against
// one mirror PathTimingTrajectory per planner. The discarding set ends with every first resident
// row above 0 and with a smaller table.
#define main test_cartesian_stream_mirror_gpu_main
#include "test_cartesian_stream_mirror_gpu.cc"
#undef main

static void TestDiscardFamily(Method method) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 6;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet disc(opt, B, CartesianTableCapacity{(size_t)N}), twin(opt, B, CartesianTableCapacity{(size_t)N});
  CHECK(disc.status().ok() && twin.status().ok());
  if (!disc.status().ok() || !twin.status().ok()) return;
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> disc_paths(B), twin_paths(B), mirror_paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) {
    const double frac = (b % 2) ? 0.25 : 0.4;
    disc_paths[b] = MakePath(b / 2, frac);
    twin_paths[b] = MakePath(b / 2, frac);
    mirror_paths[b] = MakePath(b / 2, frac);
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(mirror_paths[b]).ok());
  }
  CHECK(disc.SetCartesianPaths(disc_paths, /*streaming=*/true).ok());
  CHECK(twin.SetCartesianPaths(twin_paths, /*streaming=*/true).ok());
  std::vector<int64_t> start(B, 0);
  std::vector<PlannedTrajectory> td(B), tt(B);
  std::vector<int32_t> first(B, 0);
  int plans = 0, equal = 0, suspensions = 0, advanced = 0;
  for (int step = 0; step < 300; step++) {
    std::vector<Time> st(B);
    for (int b = 0; b < B; b++) st[b] = FromUnixNanos(start[b]);
    const std::vector<tpamd::compat::Duration> hz(B, Milliseconds(750));
    const auto sd = disc.PlanStreaming(st, hz, /*discard=*/true);
    const int susp_d = disc.SuspensionsOfLastPlan();
    const auto sw = twin.PlanStreaming(st, hz);
    CHECK(susp_d == twin.SuspensionsOfLastPlan());
    suspensions += susp_d;
    plans++;
    bool all_done = true;
    for (int b = 0; b < B; b++) {
      const Status ms = mirrors[b]->Plan(st[b], Milliseconds(750));
      CHECK(ms.ok() && sd[b].ok() && sw[b].ok());
      CHECK(CompareOne(disc, b, *mirrors[b], nullptr, &td[b]) == 0 && CompareOne(twin, b, *mirrors[b], nullptr, &tt[b]) == 0);
      const bool same = disc.GetNumTimeSamples(b) == twin.GetNumTimeSamples(b) &&
                        ToUnixNanos(disc.GetEndTime(b)) == ToUnixNanos(twin.GetEndTime(b)) &&
                        ToUnixNanos(disc.GetFinalDecelStart(b)) == ToUnixNanos(twin.GetFinalDecelStart(b)) &&
                        disc.IsTrajectoryAtEnd(b) == twin.IsTrajectoryAtEnd(b) && SameBits(td[b].time, tt[b].time) &&
                        SameBits(td[b].path_parameter, tt[b].path_parameter) &&
                        SameBits(td[b].path_parameter_derivative, tt[b].path_parameter_derivative) &&
                        SameBits(td[b].positions, tt[b].positions) && SameBits(td[b].velocities, tt[b].velocities) &&
                        SameBits(td[b].accelerations, tt[b].accelerations);
      CHECK(same);
      equal += same;
      int32_t f = -1, r = -1, c = -1, rt = -1;
      CHECK(disc.GetIkTableInfo(b, &f, &r, &c).ok() && twin.GetIkTableInfo(b, nullptr, &rt, nullptr).ok());
      CHECK(f >= first[b] && f <= r - 1 && r == rt);
      advanced += f > first[b];
      first[b] = f;
    }
    for (int b = 0; b < B; b++)
      if (!mirrors[b]->IsTrajectoryAtEnd()) {
        start[b] = std::min<int64_t>(ToUnixNanos(mirrors[b]->GetEndTime()), start[b] + 200 * kMs);
        all_done = false;
      }
    if (all_done) break;
  }
  int positive = 0;
  int32_t cap_d = 0, cap_t = 0;
  for (int b = 0; b < B; b++) {
    CHECK(mirrors[b]->IsTrajectoryAtEnd() && disc.IsTrajectoryAtEnd(b));
    positive += first[b] > 0;
    int32_t ft = -1;
    CHECK(disc.GetIkTableInfo(b, nullptr, nullptr, &cap_d).ok() && twin.GetIkTableInfo(b, &ft, nullptr, &cap_t).ok() && ft == 0);
  }
  // a discard on its own: nothing is left below the floor, the first rows come back as they are
  const auto again = disc.DiscardIkRows();
  CHECK(again.ok() && *again == first);
  CHECK(plans > 4 && equal == plans * B && suspensions >= B && positive == B && cap_d < cap_t);
  std::printf("discard mirror family (%s): %d Plan calls, %d planner-plans equal with and without the discard flag, "
              "%d suspensions, %d first rows advanced, table capacity %d against %d\n", skip ? "skip" : "uniform", plans, equal,
              suspensions, advanced, (int)cap_d, (int)cap_t);
}

int main() {
  TestDiscardFamily(Method::kUniformlyInTime);
  TestDiscardFamily(Method::kSkipSamplesCloserThanTimeStep);
  {
    PathTimingTrajectoryOptions opt;
    opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
    PathTimingTrajectorySet joint(opt, 2, 8);
    CHECK(joint.status().ok());
    CHECK(joint.DiscardIkRows().status().code() == StatusCode::kFailedPrecondition);
    std::printf("DiscardIkRows on a joint set: refused\n");
  }
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

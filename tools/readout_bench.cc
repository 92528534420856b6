// Bulk readout of a planner set, run on the GPU machine (g++ -O2 -std=c++17 -ffp-contract=off
// -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/readout_bench.cc -L<host> -ltp_host -L<csrc> -ltpamd
// -L<rocm>/lib -lamdhip64; argv: planners, trials). The tools/plan_bench.cc workload: 1024 planners
// x 7 joints, 10 waypoints, N = 1000 path samples, 4 ms time step, one Plan(t0, 750 ms). Then:
//   (a) get_trajectory_loop  PathTimingTrajectorySet::GetTrajectory for every planner
//   (b) get_trajectories     PathTimingTrajectorySet::GetTrajectories for all planners (one call)
//   (c) get_setpoints        GetSetpoints, 50 ticks at 4 ms from each planner's start time
//   (d) the _device variants of (b) and (c) on a non-blocking stream into device memory, timed with
//       HIP events around the call (a raw C-ABI set with the same paths and Plan)
// Times are medians over the trials (host clock around each call for (a)-(c)). Bytes are what
// crosses PCIe per call. (b) must equal (a) byte for byte. One JSON line.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"

#define BENCH_SUPPORT_SEED 20261016
#define BENCH_SUPPORT_MIRROR
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

#define HIPCHECK(x)                                                        \
  do {                                                                     \
    if ((x) != hipSuccess) {                                               \
      std::printf("{\"error\": \"HIP call failed at line %d\"}\n", __LINE__); \
      return 1;                                                            \
    }                                                                      \
  } while (0)

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int trials = argc > 2 ? std::atoi(argv[2]) : 5;
  const int D = 7, N = 1000, W = 10, ticks = 50;
  const int64_t kMs = 1000000, t0 = 1000 * kMs, step = 4 * kMs;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  for (int b = 0; b < B; b++) paths[b] = make_path(D, N, W);
  PathTimingTrajectorySet set(opt, B, 3 * W - 2);
  if (!set.status().ok()) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  set.SetPaths(paths);
  set.Plan(FromUnixNanos(t0), Milliseconds(750));
  std::vector<size_t> ids(B);
  for (int b = 0; b < B; b++) ids[b] = b;
  std::vector<Time> starts(B);
  size_t rows = 0;
  for (int b = 0; b < B; b++) {
    starts[b] = set.GetStartTime(b);
    rows += set.GetNumTimeSamples(b);
  }
  std::vector<double> ta, tb, tc;
  int equal = 0, ok_ticks = 0;
  for (int trial = 0; trial < trials; trial++) {
    std::vector<PlannedTrajectory> one(B), all;
    double a = now();
    for (int b = 0; b < B; b++) set.GetTrajectory(b, &one[b]);
    ta.push_back(now() - a);
    a = now();
    set.GetTrajectories(ids, &all);
    tb.push_back(now() - a);
    TrajectorySetpoints sp;
    a = now();
    set.GetSetpoints(ids, starts, tpamd::compat::Nanoseconds(step), ticks, &sp);
    tc.push_back(now() - a);
    if (trial == 0) {
      for (int b = 0; b < B && all.size() == (size_t)B; b++)
        equal += one[b].time == all[b].time && one[b].positions == all[b].positions &&
                 one[b].velocities == all[b].velocities && one[b].accelerations == all[b].accelerations &&
                 one[b].path_parameter == all[b].path_parameter;
      for (const auto &s : sp.status) ok_ticks += s.ok();
    }
  }

  // (d) the _device variants on a raw set with the same paths and Plan
  tpamd_engine *e = nullptr;
  tpamd_planner_set *ps = nullptr;
  if (tpamd_engine_create(0, &e) != 0) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 3 * W - 2;
  cfg.max_planning_iterations = opt.GetMaxPlanningIterations(); cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = opt.GetMaxInitialVelocityError(); cfg.time_step_ns = step;
  if (tpamd_planner_set_create(e, &cfg, &ps) != 0) { std::printf("{\"error\": \"set\"}\n"); return 1; }
  {
    std::vector<int32_t> np(B), st(B, 1);
    std::vector<double> kn, cp, vmax, amax, dl, iv(B * D, 0.0);
    for (int b = 0; b < B; b++) {
      np[b] = paths[b]->num_control_points();
      kn.insert(kn.end(), paths[b]->knots().begin(), paths[b]->knots().end());
      cp.insert(cp.end(), paths[b]->packed_control_points().begin(), paths[b]->packed_control_points().end());
      vmax.insert(vmax.end(), paths[b]->GetMaxJointVelocity().begin(), paths[b]->GetMaxJointVelocity().end());
      amax.insert(amax.end(), paths[b]->GetMaxJointAcceleration().begin(), paths[b]->GetMaxJointAcceleration().end());
      dl.push_back(paths[b]->GetPathSamplingDistance());
    }
    tpamd_planner_set_upload_paths_ragged(ps, B, nullptr, np.data(), kn.data(), cp.data(), vmax.data(), amax.data(),
                                          dl.data(), iv.data(), st.data());
    std::vector<int64_t> s(B, t0), h(B, 750 * kMs);
    tpamd_planner_set_plan(ps, s.data(), h.data(), nullptr);
  }
  hipStream_t stream;
  hipEvent_t ev0, ev1;
  HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  const size_t nt = (size_t)B * ticks;
  int64_t *d_start = nullptr, *d_off = nullptr;
  int32_t *d_st = nullptr;
  double *d_q = nullptr, *d_rows = nullptr;
  HIPCHECK(hipMalloc(&d_start, B * 8));
  HIPCHECK(hipMalloc(&d_off, (B + 1) * 8));
  HIPCHECK(hipMalloc(&d_st, nt * 4));
  HIPCHECK(hipMalloc(&d_q, nt * D * 8 * 3));
  HIPCHECK(hipMalloc(&d_rows, rows * (4 + 3 * D) * 8));
  {
    std::vector<int64_t> s(B);
    for (int b = 0; b < B; b++) s[b] = tpamd::compat::ToUnixNanos(starts[b]);
    HIPCHECK(hipMemcpy(d_start, s.data(), B * 8, hipMemcpyHostToDevice));
  }
  double *r = d_rows;
  std::vector<double> td_pack, td_ticks;
  for (int trial = 0; trial < trials + 1; trial++) {     // the first is a warm-up
    float ms = 0.f;
    HIPCHECK(hipEventRecord(ev0, stream));
    if (tpamd_planner_set_download_trajectories_device(ps, B, nullptr, d_off, (int64_t)rows, r, r + rows, r + 2 * rows,
                                                       r + 3 * rows, r + 4 * rows, r + (4 + D) * rows,
                                                       r + (4 + 2 * D) * rows, stream) != 0)
      return 1;
    HIPCHECK(hipEventRecord(ev1, stream));
    HIPCHECK(hipEventSynchronize(ev1));
    HIPCHECK(hipEventElapsedTime(&ms, ev0, ev1));
    if (trial) td_pack.push_back(ms * 1e-3);
    HIPCHECK(hipEventRecord(ev0, stream));
    if (tpamd_planner_set_sample_at_ticks_device(ps, B, nullptr, d_start, step, ticks, d_q, d_q + nt * D,
                                                 d_q + 2 * nt * D, d_st, stream) != 0)
      return 1;
    HIPCHECK(hipEventRecord(ev1, stream));
    HIPCHECK(hipEventSynchronize(ev1));
    HIPCHECK(hipEventElapsedTime(&ms, ev0, ev1));
    if (trial) td_ticks.push_back(ms * 1e-3);
  }
  int64_t total = -1;
  HIPCHECK(hipMemcpy(&total, d_off + B, 8, hipMemcpyDeviceToHost));
  for (void *p : {(void *)d_start, (void *)d_off, (void *)d_st, (void *)d_q, (void *)d_rows}) HIPCHECK(hipFree(p));
  HIPCHECK(hipEventDestroy(ev0));
  HIPCHECK(hipEventDestroy(ev1));
  HIPCHECK(hipStreamDestroy(stream));
  tpamd_planner_set_destroy(ps);
  tpamd_engine_destroy(e);

  const size_t row_bytes = (4 + 3 * D) * 8;
  const size_t bytes_a = (size_t)B * 8 + rows * row_bytes;          // t_first / t_count, then the rows
  const size_t bytes_b = (size_t)(B + 1) * 8 + rows * row_bytes;    // offsets, then the rows (ids: 4 B up)
  const size_t bytes_c = (size_t)B * 12 + nt * 4 + nt * 3 * D * 8;  // start times + ids up; statuses + values
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"time_step_ms\": 4, \"horizon_ms\": 750, "
              "\"trials\": %d, \"samples\": %zu, \"ticks\": %d, "
              "\"get_trajectory_loop_ms\": %.3f, \"get_trajectories_ms\": %.3f, \"speedup_b_over_a\": %.1f, "
              "\"get_setpoints_ms\": %.3f, \"download_trajectories_device_ms\": %.4f, "
              "\"sample_at_ticks_device_ms\": %.4f, \"trajectories_equal\": %d, \"ok_ticks\": %d, "
              "\"device_rows\": %lld, \"pcie_bytes_a\": %zu, \"pcie_copies_a\": %d, \"pcie_bytes_b\": %zu, "
              "\"pcie_bytes_c\": %zu, \"device_bytes_written_b\": %zu, \"device_bytes_written_c\": %zu}\n",
              B, D, N, trials, rows, ticks, 1e3 * median(ta), 1e3 * median(tb), median(ta) / median(tb), 1e3 * median(tc),
              1e3 * median(td_pack), 1e3 * median(td_ticks), equal, ok_ticks, (long long)total, bytes_a, 9 * B, bytes_b,
              bytes_c, rows * row_bytes + (B + 1) * 8, nt * 4 + nt * 3 * D * 8);
  return 0;
}

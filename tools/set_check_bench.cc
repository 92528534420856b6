// What planner-set checking costs (tpamd_planner_set_set_checking), run on the GPU machine; argv:
// planners, trials, path samples. Build: g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include
// tools/set_check_bench.cc -L<csrc> -ltpamd -L/opt/rocm/lib -lamdhip64 -ldl -Wl,-rpath,<csrc>.
// The workload of tools/set_plan_async_bench.cc: 1024 planners x 7 joints, N = 1000 path samples, planned 400 ms ahead and replanned every 20 ms (a steady
// receding-horizon replan: most planners solve one window per call). In the same process, sets of
// their own with the same paths and the same first plan:
//   tpamd_planner_set_plan                                   checking off | on
//   tpamd_planner_set_plan_device (max_windows 2) + stream synchronise   checking off | on
// One JSON line: wall time per call, median / min / max over the trials (two warm-up rounds are
// dropped), and what the checked sets found. The checking entries are looked up at run time, so
// the same program runs against a library without them (then only the "off" columns are measured):
// that is how "off" is compared with the library of the commit before.
#include <dlfcn.h>
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/tpamd.h"

#define BENCH_SUPPORT_SEED 20261019
#define BENCH_SUPPORT_HIP
#include "bench_support.h"

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static void report(const char *name, std::vector<double> v) {
  if (v.empty()) { std::printf("\"%s_ms\": null, ", name); return; }
  std::sort(v.begin(), v.end());
  std::printf("\"%s_ms\": %.4f, \"%s_min_ms\": %.4f, \"%s_max_ms\": %.4f, ", name, 1e3 * v[v.size() / 2], name, 1e3 * v.front(),
              name, 1e3 * v.back());
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int trials = argc > 2 ? std::atoi(argv[2]) : 40;
  const int N = argc > 3 ? std::atoi(argv[3]) : 1000;
  const int D = 7, W0 = 6, kSets = 4, max_windows = 2;
  const double delta = 1.0 / N, rounding = 0.2;
  const int64_t kMs = 1000000, t0 = 1000 * kMs, step = 20 * kMs, horizon_ns = 400 * kMs;
  using SetChecking = int (*)(tpamd_planner_set *, int);
  using CheckResults = int (*)(tpamd_planner_set *, int, const int32_t *, tpamd_planner_check *);
  const SetChecking set_checking = (SetChecking)dlsym(RTLD_DEFAULT, "tpamd_planner_set_set_checking");
  const CheckResults check_results = (CheckResults)dlsym(RTLD_DEFAULT, "tpamd_planner_set_check_results");
  const bool can_check = set_checking && check_results;
  tpamd_engine *e = nullptr;
  if (tpamd_engine_create(0, &e) != 0) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 16;
  cfg.history_capacity = 10 * N; cfg.trajectory_capacity = 1024;
  cfg.sampling_method = 0; cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = 4 * kMs;
  // sets: 0 / 1 plan with checking off / on, 2 / 3 plan_device with checking off / on
  tpamd_planner_set *set[kSets] = {};
  std::vector<int32_t> offsets(B + 1, 0), np(B), st(B);
  std::vector<double> wps, vmax, amax, dl(B, delta);
  for (int b = 0; b < B; b++) {
    offsets[b + 1] = offsets[b] + W0;
    for (int j = 0; j < W0 * D; j++) wps.push_back(3.0 * rnd() - 1.5);
    for (int d = 0; d < D; d++) { vmax.push_back(1.0 + rnd()); amax.push_back(2.0 + 3.0 * rnd()); }
  }
  std::vector<int64_t> start(B, t0), horizon(B, horizon_ns);
  std::vector<tpamd_planner_summary> summary(B);
  for (int k = 0; k < kSets; k++) {
    if (tpamd_planner_set_create(e, &cfg, &set[k]) != 0) { std::printf("{\"error\": \"no set\"}\n"); return 1; }
    if ((k & 1) && can_check && set_checking(set[k], 1) != 0) { std::printf("{\"error\": \"set_checking\"}\n"); return 1; }
    tpamd_planner_set_set_waypoints(set[k], B, nullptr, offsets.data(), wps.data(), rounding, vmax.data(), amax.data(),
                                    dl.data(), nullptr, np.data(), st.data());
    tpamd_planner_set_plan(set[k], start.data(), horizon.data(), summary.data());
    tpamd_planner_set_reserve(set[k], 0, 0);
  }
  int64_t *d_start = upload(start), *d_horizon = upload(horizon);
  tpamd_planner_summary *d_summary = nullptr;
  tpamd_plan_device_info *d_info = nullptr;
  hipMalloc((void **)&d_summary, B * sizeof(tpamd_planner_summary));
  hipMalloc((void **)&d_info, sizeof(tpamd_plan_device_info));
  hipStream_t stream;
  hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  std::vector<double> t[kSets];
  for (int trial = 0; trial < trials + 2; trial++) {     // two warm-up rounds are dropped
    const bool keep = trial >= 2;
    for (auto &s : start) s = t0 + (int64_t)(trial + 1) * step;
    hipMemcpy(d_start, start.data(), B * 8, hipMemcpyHostToDevice);
    hipDeviceSynchronize();
    for (int k = 0; k < kSets; k++) {
      if ((k & 1) && !can_check) continue;
      const double a = now();
      if (k < 2) {
        tpamd_planner_set_plan(set[k], start.data(), horizon.data(), summary.data());
      } else {
        tpamd_planner_set_plan_device(set[k], d_start, d_horizon, max_windows, d_summary, d_info, stream);
        hipStreamSynchronize(stream);
      }
      if (keep) t[k].push_back(now() - a);
    }
  }
  int ok = 0, checked = 0, violating = 0, windows = 0;
  for (const auto &r : summary) ok += r.status == TPAMD_PLAN_OK;
  if (can_check) {
    std::vector<tpamd_planner_check> rec(B);
    check_results(set[1], B, nullptr, rec.data());
    for (const auto &r : rec) { checked += r.windows > 0; violating += r.violations > 0; windows += r.windows; }
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"trials\": %d, \"library_checks\": %s, ", B, D, N, trials,
              can_check ? "true" : "false");
  report("plan_off", t[0]);
  report("plan_on", t[1]);
  report("plan_device_w2_off", t[2]);
  report("plan_device_w2_on", t[3]);
  std::printf("\"last_plan_ok\": %d, \"planners_checked\": %d, \"windows_checked\": %d, \"planners_with_violations\": %d}\n", ok,
              checked, windows, violating);
  hipStreamDestroy(stream);
  for (int k = 0; k < kSets; k++) tpamd_planner_set_destroy(set[k]);
  tpamd_engine_destroy(e);
  return 0;
}

// Moving planners between sets, run on the GPU machine (argv: planners, trials). 1024 planners x 7
// joints, N = 1000 path samples, 6 waypoints each, in a steady replan (three Plans 100 ms apart, 750 ms
// ahead). Then, medians over the trials:
//   export   tpamd_planner_set_export_state_device of every planner into one blob (exact sizes
//            from tpamd_planner_set_state_info), HIP events around the call on a non-blocking stream
//   import   tpamd_planner_set_import_state_device of that blob into a second set, likewise
//   copy     tpamd_planner_set_copy_planners into that set (host clock; it synchronises and
//            includes the size query and its download)
//   d2d      hipMemcpyDtoDAsync of the same byte count, the yardstick, in the same run
// The import is checked once: the second set's export equals the first set's. One JSON line.
//
// g++ -O2 -std=c++17 -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/set_state_bench.cc
//     -L<csrc> -ltpamd -L/opt/rocm/lib -lamdhip64 -Wl,-rpath,<csrc> -o tools/set_state_bench
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../include/tpamd.h"

#define BENCH_SUPPORT_SEED 20261020
#include "bench_support.h"

static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}
#define CHECK(expr)                                                      \
  do {                                                                   \
    const int rc_ = (int)(expr);                                         \
    if (rc_ != 0) {                                                      \
      std::printf("{\"error\": \"%s = %d\"}\n", #expr, rc_);             \
      return 1;                                                          \
    }                                                                    \
  } while (0)

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int trials = argc > 2 ? std::atoi(argv[2]) : 21;
  const int D = 7, N = 1000, W = 6;
  const int64_t kMs = 1000000;
  tpamd_engine *engine = nullptr;
  CHECK(tpamd_engine_create(0, &engine));
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 3 * W - 2;
  cfg.sampling_method = 0; cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *a = nullptr, *b = nullptr;
  CHECK(tpamd_planner_set_create(engine, &cfg, &a));
  CHECK(tpamd_planner_set_create(engine, &cfg, &b));
  std::vector<int32_t> offsets(B + 1), status(B), points(B);
  std::vector<double> wps((size_t)B * W * D), vmax((size_t)B * D), amax((size_t)B * D), delta(B, 0.004);
  for (int k = 0; k <= B; k++) offsets[k] = k * W;
  for (double &x : wps) x = 4.0 * rnd() - 2.0;
  for (double &x : vmax) x = 1.0 + rnd();
  for (double &x : amax) x = 2.0 + 2.0 * rnd();
  CHECK(tpamd_planner_set_set_waypoints(a, B, nullptr, offsets.data(), wps.data(), 0.2, vmax.data(), amax.data(),
                                        delta.data(), nullptr, points.data(), status.data()));
  std::vector<int64_t> start(B), horizon(B, 750 * kMs);
  std::vector<tpamd_planner_summary> summary(B);
  int planned = 0;
  for (int step = 0; step < 3; step++) {
    std::fill(start.begin(), start.end(), (1000 + 100 * step) * kMs);
    CHECK(tpamd_planner_set_plan(a, start.data(), horizon.data(), summary.data()));
  }
  for (int k = 0; k < B; k++) planned += summary[k].status == TPAMD_PLAN_OK;

  std::vector<tpamd_planner_state_info> info(B);
  CHECK(tpamd_planner_set_state_info(a, B, nullptr, info.data()));
  std::vector<int64_t> off(B + 1, 0);
  int history = 0, trajectory = 0;
  for (int k = 0; k < B; k++) {
    off[k + 1] = off[k] + info[k].bytes;
    history = std::max(history, info[k].history_count);
    trajectory = std::max(trajectory, info[k].trajectory_count);
  }
  const size_t total = (size_t)off[B];
  CHECK(tpamd_planner_set_reserve(b, history, trajectory));      // the device import allocates nothing

  void *blob = nullptr, *blob_b = nullptr, *other = nullptr;
  int64_t *d_off = nullptr;
  int32_t *d_status = nullptr;
  tpamd_planner_summary *d_summary = nullptr;
  CHECK(hipMalloc(&blob, total));
  CHECK(hipMalloc(&blob_b, total));
  CHECK(hipMalloc(&other, total));
  CHECK(hipMalloc((void **)&d_off, (B + 1) * 8));
  CHECK(hipMalloc((void **)&d_status, B * 4));
  CHECK(hipMalloc((void **)&d_summary, B * sizeof(tpamd_planner_summary)));
  CHECK(hipMemcpy(d_off, off.data(), (B + 1) * 8, hipMemcpyHostToDevice));
  hipStream_t st;
  CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0));
  CHECK(hipEventCreate(&e1));
  std::vector<double> t_export, t_import, t_copy, t_d2d;
  int ok_export = 0, ok_import = 0, ok_copy = 0;
  for (int trial = -2; trial < trials; trial++) {       // two warm-up rounds
    float ms = 0.f;
    CHECK(hipEventRecord(e0, st));
    CHECK(tpamd_planner_set_export_state_device(a, B, nullptr, blob, d_off, d_status, st));
    CHECK(hipEventRecord(e1, st));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (trial >= 0) t_export.push_back(ms);
    CHECK(hipMemcpy(status.data(), d_status, B * 4, hipMemcpyDeviceToHost));
    ok_export = (int)std::count(status.begin(), status.end(), TPAMD_PLAN_OK);

    CHECK(hipEventRecord(e0, st));
    CHECK(tpamd_planner_set_import_state_device(b, B, nullptr, blob, d_off, d_summary, d_status, st));
    CHECK(hipEventRecord(e1, st));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (trial >= 0) t_import.push_back(ms);
    CHECK(hipMemcpy(status.data(), d_status, B * 4, hipMemcpyDeviceToHost));
    ok_import = (int)std::count(status.begin(), status.end(), TPAMD_PLAN_OK);

    const double c0 = now();
    CHECK(tpamd_planner_set_copy_planners(b, nullptr, a, nullptr, B, summary.data(), status.data()));
    if (trial >= 0) t_copy.push_back(1e3 * (now() - c0));
    ok_copy = (int)std::count(status.begin(), status.end(), TPAMD_PLAN_OK);

    CHECK(hipEventRecord(e0, st));
    CHECK(hipMemcpyDtoDAsync(other, blob, total, st));
    CHECK(hipEventRecord(e1, st));
    CHECK(hipEventSynchronize(e1));
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    if (trial >= 0) t_d2d.push_back(ms);
  }
  // the second set holds what the first holds
  CHECK(tpamd_planner_set_export_state_device(b, B, nullptr, blob_b, d_off, d_status, st));
  CHECK(hipStreamSynchronize(st));
  std::vector<unsigned char> ha(total), hb(total);
  CHECK(hipMemcpy(ha.data(), blob, total, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hb.data(), blob_b, total, hipMemcpyDeviceToHost));
  const int equal = std::memcmp(ha.data(), hb.data(), total) == 0;
  const double ex = median(t_export), im = median(t_import), cp = median(t_copy), dd = median(t_d2d);
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"trials\": %d, \"planned\": %d, "
              "\"blob_bytes\": %zu, \"largest_history\": %d, \"largest_trajectory\": %d, "
              "\"export_ms\": %.4f, \"import_ms\": %.4f, \"copy_planners_ms\": %.4f, \"d2d_ms\": %.4f, "
              "\"export_over_d2d\": %.2f, \"import_over_d2d\": %.2f, \"copy_over_d2d\": %.2f, "
              "\"export_gb_s\": %.1f, \"import_gb_s\": %.1f, \"d2d_gb_s\": %.1f, "
              "\"ok_export\": %d, \"ok_import\": %d, \"ok_copy\": %d, \"records_equal\": %d}\n",
              B, D, N, trials, planned, total, history, trajectory, ex, im, cp, dd, ex / dd, im / dd, cp / dd,
              total / ex * 1e-6, total / im * 1e-6, total / dd * 1e-6, ok_export, ok_import, ok_copy, equal);
  tpamd_planner_set_destroy(a);
  tpamd_planner_set_destroy(b);
  tpamd_engine_destroy(engine);
  return equal && ok_export == B && ok_import == B && ok_copy == B ? 0 : 1;
}

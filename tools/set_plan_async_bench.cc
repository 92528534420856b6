// The enqueued-only Plan of a planner set against the synchronous one, run on the GPU machine
// (tools/gpu_set_plan_async_bench.py builds and runs it; argv: planners, trials, path samples).
// 1024 planners x 7 joints, N = 1000 path samples, planned 400 ms ahead and replanned every 20 ms
// (a steady receding-horizon replan: most planners solve one window per call). In the same build
// and the same run, three ways:
//   (a) tpamd_planner_set_plan (host arrays, synchronises)
//   (b) tpamd_planner_set_plan_device + hipStreamSynchronize with max_windows 1, 2 and 4
//   (c) the control cycle retarget -> plan -> insert into a buffer set -> one tick of setpoints,
//       once through the synchronous entries and once through the _device entries on one stream
//       with one synchronisation at the end
// Each way has sets of its own with the same paths and the same first plan. Reported per call or
// cycle: wall time (host clock from before the first call until the results are there) and the
// host time spent inside the library calls (for (b) and the device cycle: until the last call
// returned, before the synchronisation). One JSON line; times are medians over the trials.
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
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[v.size() / 2];
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int trials = argc > 2 ? std::atoi(argv[2]) : 40;
  const int N = argc > 3 ? std::atoi(argv[3]) : 1000;
  const int D = 7, W0 = 6, W = 3, kSets = 6;
  const int kCycleWindows = 8;      // a path that starts in mid-motion takes more windows than a steady replan
  const double delta = 1.0 / N, rounding = 0.2;
  const int64_t kMs = 1000000, t0 = 1000 * kMs, step = 20 * kMs, horizon_ns = 400 * kMs;
  tpamd_engine *e = nullptr;
  if (tpamd_engine_create(0, &e) != 0) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 16;
  cfg.history_capacity = 10 * N; cfg.trajectory_capacity = 1024;   // room for kCycleWindows windows: plan_device cannot grow
  cfg.sampling_method = 0; cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = 4 * kMs;
  // sets: 0 (a), 1..3 (b) with max_windows 1, 2, 4, 4 / 5 the synchronous / device cycle
  tpamd_planner_set *set[kSets] = {};
  std::vector<int32_t> offsets(B + 1, 0), roff(B + 1, 0), ids(B), np(B), st(B);
  std::vector<double> wps, vmax, amax, dl(B, delta), rw;
  for (int b = 0; b < B; b++) {
    ids[b] = b;
    offsets[b + 1] = offsets[b] + W0;
    roff[b + 1] = roff[b] + W;
    for (int j = 0; j < W0 * D; j++) wps.push_back(3.0 * rnd() - 1.5);
    for (int j = 0; j < W * D; j++) rw.push_back(3.0 * rnd() - 1.5);
    for (int d = 0; d < D; d++) { vmax.push_back(1.0 + rnd()); amax.push_back(2.0 + 3.0 * rnd()); }
  }
  std::vector<int64_t> start(B, t0), horizon(B, horizon_ns);
  std::vector<tpamd_planner_summary> summary(B);
  int planned = 0;
  for (int k = 0; k < kSets; k++) {
    if (tpamd_planner_set_create(e, &cfg, &set[k]) != 0) { std::printf("{\"error\": \"no set\"}\n"); return 1; }
    tpamd_planner_set_set_waypoints(set[k], B, nullptr, offsets.data(), wps.data(), rounding, vmax.data(), amax.data(),
                                    dl.data(), nullptr, np.data(), st.data());
    tpamd_planner_set_plan(set[k], start.data(), horizon.data(), summary.data());
    tpamd_planner_set_reserve(set[k], 0, 0);
  }
  for (const auto &r : summary) planned += r.status == TPAMD_PLAN_OK;
  tpamd_buffer_set *buf[2] = {};
  for (int k = 0; k < 2; k++) tpamd_buffer_set_create(e, B, D, 1024, 1e-6, &buf[k]);
  int64_t *d_start = upload(start), *d_horizon = upload(horizon), *d_tick = upload(start);
  double *d_w = upload(rw), *d_v = upload(vmax), *d_a = upload(amax), *d_dl = upload(dl);
  int32_t *d_np = upload(np), *d_st = upload(st), *d_is = upload(st), *d_ts = upload(st);
  double *d_q = nullptr;
  tpamd_planner_summary *d_summary = nullptr;
  tpamd_plan_device_info *d_info = nullptr;
  hipMalloc((void **)&d_q, (size_t)3 * B * D * 8);
  hipMalloc((void **)&d_summary, B * sizeof(tpamd_planner_summary));
  hipMalloc((void **)&d_info, sizeof(tpamd_plan_device_info));
  hipStream_t stream;
  hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  const int mw[3] = {1, 2, 4};
  std::vector<double> t_sync, t_dev[3], t_dev_call[3], t_cyc_sync, t_cyc_sync_host, t_cyc_dev, t_cyc_dev_call;
  std::vector<double> q((size_t)3 * B * D);
  std::vector<int32_t> tick_status(B);
  tpamd_plan_device_info info[3] = {}, cycle_info = {};
  int windows_cyc_sync = 0, ok_sync = 0, ok_dev[3] = {}, ok_cyc_sync = 0, ok_cyc_dev = 0, windows_sync = 0, equal_mw4 = 0;
  std::vector<tpamd_planner_summary> sum_sync(B), sum_dev(B);
  for (int trial = 0; trial < trials + 2; trial++) {     // two warm-up rounds are dropped
    const bool keep = trial >= 2;
    for (auto &s : start) s = t0 + (int64_t)(trial + 1) * step;
    hipMemcpy(d_start, start.data(), B * 8, hipMemcpyHostToDevice);
    hipMemcpy(d_tick, start.data(), B * 8, hipMemcpyHostToDevice);
    hipDeviceSynchronize();
    // (a)
    double a = now();
    tpamd_planner_set_plan(set[0], start.data(), horizon.data(), sum_sync.data());
    if (keep) t_sync.push_back(now() - a);
    // (b)
    for (int v = 0; v < 3; v++) {
      a = now();
      tpamd_planner_set_plan_device(set[1 + v], d_start, d_horizon, mw[v], d_summary, d_info, stream);
      const double called = now() - a;
      hipStreamSynchronize(stream);
      if (keep) { t_dev[v].push_back(now() - a); t_dev_call[v].push_back(called); }
      hipMemcpy(&info[v], d_info, sizeof(info[v]), hipMemcpyDeviceToHost);
      if (v == 2) hipMemcpy(sum_dev.data(), d_summary, B * sizeof(tpamd_planner_summary), hipMemcpyDeviceToHost);
    }
    // (c) synchronous entries
    a = now();
    tpamd_planner_set_retarget(set[4], B, ids.data(), start.data(), roff.data(), rw.data(), rounding, vmax.data(), amax.data(),
                               dl.data(), amax.data(), np.data(), st.data(), nullptr, nullptr, nullptr);
    tpamd_planner_set_plan(set[4], start.data(), horizon.data(), summary.data());
    tpamd_buffer_set_insert_from_planner_set(buf[0], set[4], B, nullptr, nullptr, st.data());
    tpamd_buffer_set_sample_at_ticks(buf[0], B, nullptr, start.data(), 4 * kMs, 1, q.data(), q.data() + B * D,
                                     q.data() + 2 * B * D, tick_status.data());
    if (keep) { t_cyc_sync.push_back(now() - a); t_cyc_sync_host.push_back(now() - a); }
    ok_cyc_sync = windows_cyc_sync = 0;
    for (int32_t s : tick_status) ok_cyc_sync += s == TPAMD_PLAN_OK;
    for (const auto &r : summary) windows_cyc_sync = std::max(windows_cyc_sync, (int)r.windows);
    // (c) device entries, one stream, one synchronisation
    a = now();
    tpamd_planner_set_retarget_device(set[5], B, ids.data(), d_start, roff.data(), d_w, rounding, d_v, d_a, d_dl, d_a, d_np,
                                      d_st, nullptr, nullptr, nullptr, stream);
    tpamd_planner_set_plan_device(set[5], d_start, d_horizon, kCycleWindows, d_summary, d_info, stream);
    tpamd_buffer_set_insert_from_planner_set_device(buf[1], set[5], B, nullptr, nullptr, d_is, stream);
    tpamd_buffer_set_sample_at_ticks_device(buf[1], B, nullptr, d_tick, 4 * kMs, 1, d_q, d_q + B * D, d_q + 2 * B * D, d_ts,
                                            stream);
    const double called = now() - a;
    hipStreamSynchronize(stream);
    if (keep) { t_cyc_dev.push_back(now() - a); t_cyc_dev_call.push_back(called); }
    hipMemcpy(tick_status.data(), d_ts, B * 4, hipMemcpyDeviceToHost);
    hipMemcpy(&cycle_info, d_info, sizeof(cycle_info), hipMemcpyDeviceToHost);
    ok_cyc_dev = 0;
    for (int32_t s : tick_status) ok_cyc_dev += s == TPAMD_PLAN_OK;
    ok_sync = windows_sync = equal_mw4 = 0;
    for (int b = 0; b < B; b++) {
      ok_sync += sum_sync[b].status == TPAMD_PLAN_OK;
      windows_sync = std::max(windows_sync, (int)sum_sync[b].windows);
      equal_mw4 += sum_sync[b].status == sum_dev[b].status && sum_sync[b].end_time_ns == sum_dev[b].end_time_ns &&
                   sum_sync[b].num_samples == sum_dev[b].num_samples;
    }
    for (int v = 0; v < 3; v++) ok_dev[v] = info[v].num_ok;
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"trials\": %d, \"replan_every_ms\": %lld, "
              "\"horizon_ms\": %lld, \"planned_first\": %d, "
              "\"plan_sync_ms\": %.3f, \"plan_sync_ok\": %d, \"plan_sync_max_windows\": %d, "
              "\"plan_device_w1_ms\": %.3f, \"plan_device_w1_host_ms\": %.3f, \"plan_device_w1_ok\": %d, "
              "\"plan_device_w2_ms\": %.3f, \"plan_device_w2_host_ms\": %.3f, \"plan_device_w2_ok\": %d, "
              "\"plan_device_w4_ms\": %.3f, \"plan_device_w4_host_ms\": %.3f, \"plan_device_w4_ok\": %d, "
              "\"w4_summaries_equal_sync\": %d, "
              "\"cycle_sync_ms\": %.3f, \"cycle_sync_host_ms\": %.3f, \"cycle_sync_ticks_ok\": %d, "
              "\"cycle_sync_max_windows\": %d, \"cycle_device_max_windows\": %d, \"cycle_device_ms\": %.3f, \"cycle_device_host_ms\": %.3f, \"cycle_device_ticks_ok\": %d, "
              "\"cycle_device_exhausted\": %d, \"cycle_device_windows_solved\": %d}\n",
              B, D, N, trials, (long long)(step / kMs), (long long)(horizon_ns / kMs), planned, 1e3 * median(t_sync), ok_sync,
              windows_sync, 1e3 * median(t_dev[0]), 1e3 * median(t_dev_call[0]), ok_dev[0], 1e3 * median(t_dev[1]),
              1e3 * median(t_dev_call[1]), ok_dev[1], 1e3 * median(t_dev[2]), 1e3 * median(t_dev_call[2]), ok_dev[2],
              equal_mw4, 1e3 * median(t_cyc_sync), 1e3 * median(t_cyc_sync_host), ok_cyc_sync, windows_cyc_sync, kCycleWindows, 1e3 * median(t_cyc_dev),
              1e3 * median(t_cyc_dev_call), ok_cyc_dev, cycle_info.num_exhausted, cycle_info.max_windows_solved);
  hipStreamDestroy(stream);
  for (int k = 0; k < 2; k++) tpamd_buffer_set_destroy(buf[k]);
  for (int k = 0; k < kSets; k++) tpamd_planner_set_destroy(set[k]);
  tpamd_engine_destroy(e);
  return 0;
}

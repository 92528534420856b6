// Retargeting the moving planners of a set, run on the GPU machine (tools/gpu_set_retarget_bench.py
// builds and runs it; argv: planners, trials). 1024 planners x 7 joints, N = 300 path samples,
// planned 750 ms ahead; 200 ms into the motion every planner is redirected onto 4 new waypoints.
// Three routes to the same resident state:
//   baseline  the best route without the retarget entry: GetSetpoints with one tick (position and
//             velocity come down), ComputeStoppingPoint per planner on the host, SetWaypointPaths
//             with [position, stopping point, waypoints...] and the velocity as initial velocity
//   host      PathTimingTrajectorySet::RetargetWaypointPaths (tpamd_planner_set_retarget; synchronises)
//   device    tpamd_planner_set_retarget_device on a non-blocking stream with the inputs in device
//             memory, timed with HIP events around the call (enqueue to completion)
// All three must leave the same resident splines. One JSON line; times are medians over the trials
// (host clock around the calls, or the events); the PCIe bytes are those of the calls' arrays.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../include/tpamd.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../x-edr-trajectory-planning_amd/host/path_tools.h"

#define BENCH_SUPPORT_SEED 20261019
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

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int trials = argc > 2 ? std::atoi(argv[2]) : 7;
  const int D = 7, N = 300, W0 = 5, W = 4;
  const double delta = 0.01, rounding = 0.2;
  const int64_t kMs = 1000000, t0 = 1000 * kMs, t_retarget = t0 + 200 * kMs;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  auto waypoints = [&](int count) {
    std::vector<VectorXd> w;
    for (int i = 0; i < count; i++) {
      VectorXd v(D);
      for (int d = 0; d < D; d++) v[d] = 3.0 * rnd() - 1.5;
      w.push_back(v);
    }
    return w;
  };
  std::vector<size_t> all(B);
  std::vector<std::vector<VectorXd>> first(B), next(B);
  std::vector<VectorXd> vmax(B, VectorXd(D)), amax(B, VectorXd(D));
  std::vector<Time> when(B, FromUnixNanos(t_retarget));
  for (int b = 0; b < B; b++) {
    all[b] = b;
    first[b] = waypoints(W0);
    next[b] = waypoints(W);
    for (int d = 0; d < D; d++) { vmax[b][d] = 1.0 + rnd(); amax[b][d] = 2.0 + 3.0 * rnd(); }
  }
  // three sets with the same paths and the same plan
  PathTimingTrajectorySet base(opt, B, 16), host(opt, B, 16), dev(opt, B, 16);
  if (!base.status().ok() || !host.status().ok() || !dev.status().ok()) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  int planned = 0;
  for (PathTimingTrajectorySet *s : {&base, &host, &dev}) {
    s->SetWaypointPaths(all, first, vmax, amax, {}, rounding, delta);
    planned = 0;
    for (const auto &st : s->Plan(FromUnixNanos(t0), Milliseconds(750))) planned += st.ok();
  }
  // device-resident inputs of the device route
  std::vector<int32_t> ids(B), offsets(B + 1, 0);
  std::vector<int64_t> t(B, t_retarget);
  std::vector<double> flat, fv, fa, dl(B, delta);
  for (int b = 0; b < B; b++) {
    ids[b] = b;
    offsets[b + 1] = offsets[b] + W;
    for (const auto &w : next[b]) flat.insert(flat.end(), w.begin(), w.end());
    fv.insert(fv.end(), vmax[b].begin(), vmax[b].end());
    fa.insert(fa.end(), amax[b].begin(), amax[b].end());
  }
  int64_t *d_t;
  double *d_wps, *d_vmax, *d_amax, *d_dl;
  int32_t *d_np, *d_st;
  hipMalloc(&d_t, B * 8); hipMalloc(&d_wps, flat.size() * 8); hipMalloc(&d_vmax, fv.size() * 8);
  hipMalloc(&d_amax, fa.size() * 8); hipMalloc(&d_dl, B * 8); hipMalloc(&d_np, B * 4); hipMalloc(&d_st, B * 4);
  hipMemcpy(d_t, t.data(), B * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_wps, flat.data(), flat.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_vmax, fv.data(), fv.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_amax, fa.data(), fa.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_dl, dl.data(), B * 8, hipMemcpyHostToDevice);
  hipStream_t stream;
  hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  std::vector<double> t_base, t_host, t_device, t_device_call;
  int ok_base = 0, ok_host = 0;
  for (int trial = 0; trial < trials; trial++) {
    // the trajectories stay resident through a retarget: every trial starts from the same state
    double a = now();
    TrajectorySetpoints sp;
    base.GetSetpoints(all, when, Milliseconds(4), 1, &sp);
    std::vector<std::vector<VectorXd>> lists(B);
    std::vector<VectorXd> iv(B, VectorXd(D));
    for (int b = 0; b < B; b++) {
      const double *q = &sp.positions[(size_t)b * D], *qd = &sp.velocities[(size_t)b * D];
      const auto stop = ComputeStoppingPoint({q, (size_t)D}, {qd, (size_t)D}, {amax[b].data(), (size_t)D}, rounding);
      lists[b].push_back(VectorXd(q, D));
      iv[b] = VectorXd(qd, D);
      if (stop.ok() && !(iv[b].maxAbs() < 100 * 2.220446049250313e-16)) lists[b].push_back(stop.value());
      lists[b].insert(lists[b].end(), next[b].begin(), next[b].end());
    }
    ok_base = 0;
    for (const auto &st : base.SetWaypointPaths(all, lists, vmax, amax, iv, rounding, delta)) ok_base += st.ok();
    t_base.push_back(now() - a);
    a = now();
    ok_host = 0;
    for (const auto &st : host.RetargetWaypointPaths(all, when, next, vmax, amax, rounding, delta)) ok_host += st.ok();
    t_host.push_back(now() - a);
    hipEventRecord(e0, stream);
    a = now();
    tpamd_planner_set_retarget_device(dev.native_handle(), B, ids.data(), d_t, offsets.data(), d_wps, rounding, d_vmax,
                                      d_amax, d_dl, nullptr, d_np, d_st, nullptr, nullptr, nullptr, stream);
    t_device_call.push_back(now() - a);
    hipEventRecord(e1, stream);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    t_device.push_back(ms * 1e-3);
  }
  int equal = 0;
  for (int b = 0; b < B; b++) {
    std::vector<double> k1, c1, k2, c2, k3, c3;
    base.GetPath(b, &k1, &c1);
    host.GetPath(b, &k2, &c2);
    dev.GetPath(b, &k3, &c3);
    equal += !k1.empty() && k1 == k2 && c1 == c2 && k1 == k3 && c1 == c3;
  }
  double a = now();
  int replanned = 0;
  for (const auto &st : host.Plan(FromUnixNanos(t_retarget), Milliseconds(750))) replanned += st.ok();
  const double t_plan = now() - a;
  // the arrays that cross PCIe, per planner: baseline = one tick of setpoints (ids + time up; q, qd,
  // qdd, status down) plus set_waypoints (ids, offsets, W + 2 waypoints, limits, delta, initial
  // velocity up; count and status down); host retarget = ids, time, offsets, W waypoints, limits,
  // delta, stopping acceleration up; count, status, position, velocity, stopping point down;
  // device retarget = ids and offsets up
  const int base_up = (4 + 8) + (4 + 4 + (W + 2) * D * 8 + 3 * D * 8 + 8), base_down = (3 * D * 8 + 4) + (4 + 4);
  const int host_up = 4 + 8 + 4 + W * D * 8 + 3 * D * 8 + 8, host_down = 4 + 4 + 3 * D * 8;
  std::printf("{\"planners\": %d, \"dofs\": %d, \"new_waypoints\": %d, \"path_samples\": %d, \"trials\": %d, "
              "\"planned_before\": %d, \"baseline_setpoints_host_stop_set_waypoints_ms\": %.3f, \"retarget_host_ms\": %.3f, "
              "\"retarget_device_events_ms\": %.3f, \"retarget_device_call_ms\": %.3f, \"speedup_host_vs_baseline\": %.1f, "
              "\"speedup_device_vs_baseline\": %.1f, \"baseline_ok\": %d, \"retarget_ok\": %d, \"splines_equal\": %d, "
              "\"replanned_ok\": %d, \"replan_ms\": %.3f, \"baseline_bytes_up\": %lld, \"baseline_bytes_down\": %lld, "
              "\"retarget_host_bytes_up\": %lld, \"retarget_host_bytes_down\": %lld, \"retarget_device_bytes_up\": %lld, "
              "\"retarget_device_bytes_down\": 0}\n",
              B, D, W, N, trials, planned, 1e3 * median(t_base), 1e3 * median(t_host), 1e3 * median(t_device),
              1e3 * median(t_device_call), median(t_base) / median(t_host), median(t_base) / median(t_device), ok_base,
              ok_host, equal, replanned, 1e3 * t_plan, (long long)base_up * B, (long long)base_down * B,
              (long long)host_up * B, (long long)host_down * B, (long long)8 * B + 4);
  hipStreamDestroy(stream);
  return 0;
}

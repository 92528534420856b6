// New waypoint paths for a planner set, run on the GPU machine (g++ -O2 -std=c++17 -ffp-contract=off
// -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include tools/set_waypoints_bench.cc -L<host> -ltp_host -L<csrc>
// -ltpamd -L/opt/rocm/lib -lamdhip64; argv: planners, trials). 1024 planners x 7 joints x 6 waypoints,
// N = 1000 path samples. Three ways of giving every planner a new path:
//   mirror  TimeableJointSplinePath::SetWaypoints + limits per planner on the host, then SetPaths
//           (one ragged upload)
//   host    tpamd_planner_set_set_waypoints (host arrays; synchronises)
//   device  tpamd_planner_set_set_waypoints_device on a non-blocking stream with the inputs in
//           device memory, timed with HIP events around the call (enqueue to completion)
// All three must leave the same resident splines. Then a Plan(t0, 750 ms) of the fitted set. One
// JSON line; times are medians over the trials (host clock around the call, or the events).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../include/tpamd.h"
#include "../x-edr-trajectory-planning_amd/host/engine_handle.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"

#define BENCH_SUPPORT_SEED 20261016
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
  const int D = 7, N = 1000, W = 6, P = 3 * W - 2;
  const double delta = 0.01, rounding = 0.2;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  // inputs: packed for the C-ABI, per planner for the mirror
  std::vector<std::vector<VectorXd>> wps(B);
  std::vector<VectorXd> vmax(B, VectorXd(D)), amax(B, VectorXd(D));
  std::vector<double> flat, fv, fa, dl(B, delta), iv((size_t)B * D, 0.0);
  std::vector<int32_t> ids(B), offsets(B + 1, 0), st(B), np(B);
  std::vector<size_t> all(B);
  for (int b = 0; b < B; b++) {
    for (int i = 0; i < W; i++) {
      VectorXd v(D);
      for (int d = 0; d < D; d++) v[d] = 4.0 * rnd() - 2.0;
      wps[b].push_back(v);
      flat.insert(flat.end(), v.begin(), v.end());
    }
    for (int d = 0; d < D; d++) {
      vmax[b][d] = 1.0 + rnd();
      amax[b][d] = 2.0 + 2.0 * rnd();
      fv.push_back(vmax[b][d]);
      fa.push_back(amax[b][d]);
    }
    ids[b] = b;
    all[b] = b;
    offsets[b + 1] = offsets[b] + W;
  }
  PathTimingTrajectorySet mirror_set(opt, B, P), fit_set(opt, B, P);
  if (!mirror_set.status().ok() || !fit_set.status().ok()) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  // the C-ABI on a set of its own
  tpamd::EngineLease lease = tpamd::acquire_engine();
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = P;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = 4000000;
  tpamd_planner_set *ps = nullptr;
  if (tpamd_planner_set_create(lease.get(), &cfg, &ps) != 0) { std::printf("{\"error\": \"set\"}\n"); return 1; }
  double *d_wps, *d_vmax, *d_amax, *d_dl;
  int32_t *d_np, *d_st;
  hipMalloc(&d_wps, flat.size() * 8); hipMalloc(&d_vmax, fv.size() * 8); hipMalloc(&d_amax, fa.size() * 8);
  hipMalloc(&d_dl, B * 8); hipMalloc(&d_np, B * 4); hipMalloc(&d_st, B * 4);
  hipMemcpy(d_wps, flat.data(), flat.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_vmax, fv.data(), fv.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_amax, fa.data(), fa.size() * 8, hipMemcpyHostToDevice);
  hipMemcpy(d_dl, dl.data(), B * 8, hipMemcpyHostToDevice);
  hipStream_t stream;
  hipStreamCreateWithFlags(&stream, hipStreamNonBlocking);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  std::vector<double> t_mirror, t_host, t_device, t_device_call;
  int ok_host = 0;
  for (int trial = 0; trial < trials; trial++) {
    double a = now();
    std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
    for (int b = 0; b < B; b++) {
      paths[b] = std::make_shared<TimeableJointSplinePath>(
          JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta).set_rounding(rounding));
      paths[b]->SetWaypoints({wps[b].data(), wps[b].size()});
      paths[b]->SetMaxJointVelocity({vmax[b].data(), vmax[b].size()});
      paths[b]->SetMaxJointAcceleration({amax[b].data(), amax[b].size()});
    }
    mirror_set.SetPaths(paths);
    t_mirror.push_back(now() - a);
    a = now();
    tpamd_planner_set_set_waypoints(ps, B, ids.data(), offsets.data(), flat.data(), rounding, fv.data(), fa.data(),
                                    dl.data(), iv.data(), np.data(), st.data());
    t_host.push_back(now() - a);
    ok_host = 0;
    for (int b = 0; b < B; b++) ok_host += st[b] == TPAMD_PLAN_OK;
    hipEventRecord(e0, stream);
    a = now();
    tpamd_planner_set_set_waypoints_device(ps, B, ids.data(), offsets.data(), d_wps, rounding, d_vmax, d_amax, d_dl,
                                           nullptr, d_np, d_st, stream);
    t_device_call.push_back(now() - a);
    hipEventRecord(e1, stream);
    hipEventSynchronize(e1);
    float ms = 0;
    hipEventElapsedTime(&ms, e0, e1);
    t_device.push_back(ms * 1e-3);
  }
  // the same splines on every side
  fit_set.SetWaypointPaths(all, wps, vmax, amax, {}, rounding, delta);
  int equal = 0;
  for (int b = 0; b < B; b++) {
    std::vector<double> k1, c1, k2, c2, k3(P + 3), c3((size_t)P * D);
    int32_t got = 0;
    mirror_set.GetPath(b, &k1, &c1);
    fit_set.GetPath(b, &k2, &c2);
    tpamd_planner_set_download_path(ps, b, &got, k3.data(), c3.data(), P);
    equal += k1 == k2 && c1 == c2 && k1 == k3 && c1 == c3;
  }
  const int64_t t0 = 1000 * 1000000LL;
  double a = now();
  fit_set.Plan(FromUnixNanos(t0), Milliseconds(750));
  const double t_plan = now() - a;
  std::printf("{\"planners\": %d, \"dofs\": %d, \"waypoints\": %d, \"control_points\": %d, \"path_samples\": %d, "
              "\"trials\": %d, \"mirror_host_loop_ms\": %.3f, \"set_waypoints_host_ms\": %.3f, "
              "\"set_waypoints_device_events_ms\": %.3f, \"set_waypoints_device_call_ms\": %.3f, "
              "\"speedup_host_vs_mirror\": %.1f, \"speedup_device_vs_mirror\": %.1f, \"fitted_ok\": %d, "
              "\"splines_equal\": %d, \"first_plan_ms\": %.3f, \"bytes_up_per_planner_host\": %d}\n",
              B, D, W, P, N, trials, 1e3 * median(t_mirror), 1e3 * median(t_host), 1e3 * median(t_device),
              1e3 * median(t_device_call), median(t_mirror) / median(t_host), median(t_mirror) / median(t_device),
              ok_host, equal, 1e3 * t_plan, 4 + 4 + W * D * 8 + 3 * D * 8 + 8);
  hipStreamDestroy(stream);
  tpamd_planner_set_destroy(ps);
  return 0;
}

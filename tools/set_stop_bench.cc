// Stopping the trajectories of a planner set, run on the GPU machine (g++ -O2 -std=c++17
// -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/set_stop_bench.cc -L<host>
// -ltp_host -L<csrc> -ltpamd -L<rocm>/lib -lamdhip64; argv: planners, trials). The
// tools/readout_bench.cc workload: 1024 planners x 7 joints, 10 waypoints, N = 1000 path samples,
// 4 ms time step, one Plan(t0, 750 ms). Every planner is stopped 300 ms after its start time with
// max_acceleration = 2x its path limit:
//   (a) host_loop       GetTrajectory + the mirror TrajectoryBuffer::StopBeforeTime per planner
//   (b) set_host        PathTimingTrajectorySet::StopTrajectoriesBeforeTime (one call)
//   (c) set_device      tpamd_planner_set_stop_trajectories_device on a non-blocking stream into
//                       device memory, timed with HIP events around the call (a raw C-ABI set with
//                       the same paths and Plan)
// Times are medians over the trials. (b) must equal (a) byte for byte. One JSON line.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"

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
  const int D = 7, N = 1000, W = 10;
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
  std::vector<Time> times(B);
  std::vector<VectorXd> amax(B);
  std::vector<double> am_flat((size_t)B * D);
  std::vector<int64_t> tns(B);
  for (int b = 0; b < B; b++) {
    ids[b] = b;
    tns[b] = tpamd::compat::ToUnixNanos(set.GetStartTime(b)) + 300 * kMs;
    times[b] = FromUnixNanos(tns[b]);
    amax[b] = VectorXd(D);
    for (int d = 0; d < D; d++) am_flat[(size_t)b * D + d] = amax[b][d] = 2.0 * paths[b]->GetMaxJointAcceleration()[d];
  }
  std::vector<double> ta, tb;
  int equal = 0, ok = 0;
  size_t seg_rows = 0;
  for (int trial = 0; trial < trials; trial++) {
    // (a) the host loop
    std::vector<std::shared_ptr<TrajectoryBuffer>> bufs(B);
    std::vector<Status> st(B);
    double a = now();
    for (int b = 0; b < B; b++) {
      PlannedTrajectory p;
      set.GetTrajectory(b, &p);
      const size_t n = p.time.size();
      std::vector<VectorXd> q(n), v(n), c(n);
      for (size_t i = 0; i < n; i++) {
        q[i] = VectorXd(&p.positions[i * D], D);
        v[i] = VectorXd(&p.velocities[i * D], D);
        c[i] = VectorXd(&p.accelerations[i * D], D);
      }
      bufs[b] = *TrajectoryBuffer::Create();
      bufs[b]->InsertSegment(p.time, q, v, c);
      st[b] = bufs[b]->StopBeforeTime(times[b], amax[b], 4e-3);
    }
    ta.push_back(now() - a);
    // (b) one set call
    std::vector<StoppingSegment> segs;
    a = now();
    set.StopTrajectoriesBeforeTime(ids, times, amax, 4e-3, &segs);
    tb.push_back(now() - a);
    if (trial == 0 && segs.size() == (size_t)B) {
      for (int b = 0; b < B; b++) {
        ok += st[b].ok();
        seg_rows += segs[b].time.size();
        const TrajectoryBuffer &buf = *bufs[b];
        bool same = segs[b].status.code() == st[b].code() && segs[b].keep + segs[b].time.size() == buf.GetNumSamples();
        PlannedTrajectory p;
        set.GetTrajectory(b, &p);
        for (size_t i = 0; same && i < buf.GetNumSamples(); i++) {
          const bool kept = i < segs[b].keep;
          const size_t j = i - segs[b].keep;
          same = std::memcmp(&buf.GetTimes()[i], kept ? &p.time[i] : &segs[b].time[j], 8) == 0 &&
                 std::memcmp(buf.GetVelocities()[i].data(), kept ? &p.velocities[i * D] : &segs[b].velocities[j * D],
                             D * 8) == 0 &&
                 std::memcmp(buf.GetAccelerations()[i].data(),
                             kept ? &p.accelerations[i * D] : &segs[b].accelerations[j * D], D * 8) == 0;
        }
        equal += same;
      }
    }
  }

  // (c) the _device variant on a raw set with the same paths and Plan
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
    std::vector<double> knots, cps, vmax, am, delta, iv((size_t)B * D, 0.0);
    for (int b = 0; b < B; b++) {
      np[b] = paths[b]->num_control_points();
      knots.insert(knots.end(), paths[b]->knots().begin(), paths[b]->knots().end());
      cps.insert(cps.end(), paths[b]->packed_control_points().begin(), paths[b]->packed_control_points().end());
      vmax.insert(vmax.end(), paths[b]->GetMaxJointVelocity().begin(), paths[b]->GetMaxJointVelocity().end());
      am.insert(am.end(), paths[b]->GetMaxJointAcceleration().begin(), paths[b]->GetMaxJointAcceleration().end());
      delta.push_back(paths[b]->GetPathSamplingDistance());
    }
    // the paths were uploaded as kNewPath by the set above; upload the same here
    if (tpamd_planner_set_upload_paths_ragged(ps, B, nullptr, np.data(), knots.data(), cps.data(), vmax.data(), am.data(),
                                              delta.data(), iv.data(), st.data()) != 0) {
      std::printf("{\"error\": \"upload\"}\n");
      return 1;
    }
    std::vector<int64_t> s(B, t0), h(B, 750 * kMs);
    if (tpamd_planner_set_plan(ps, s.data(), h.data(), nullptr) != 0) { std::printf("{\"error\": \"plan\"}\n"); return 1; }
  }
  hipStream_t stream = nullptr;
  HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  const int64_t cap = (int64_t)std::max<size_t>(seg_rows, 1) * 2;
  int32_t *d_st = nullptr, *d_keep = nullptr;
  int64_t *d_t = nullptr, *d_off = nullptr;
  double *d_am = nullptr, *d_rows = nullptr;
  HIPCHECK(hipMalloc(&d_st, B * 4)); HIPCHECK(hipMalloc(&d_keep, B * 4)); HIPCHECK(hipMalloc(&d_t, B * 8));
  HIPCHECK(hipMalloc(&d_off, (B + 1) * 8)); HIPCHECK(hipMalloc(&d_am, (size_t)B * D * 8));
  HIPCHECK(hipMalloc(&d_rows, (size_t)cap * (1 + 3 * D) * 8));
  HIPCHECK(hipMemcpy(d_t, tns.data(), B * 8, hipMemcpyHostToDevice));
  HIPCHECK(hipMemcpy(d_am, am_flat.data(), (size_t)B * D * 8, hipMemcpyHostToDevice));
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  std::vector<double> tc, tcall;
  double *rt = d_rows, *rq = rt + cap, *rqd = rq + cap * D, *rqdd = rqd + cap * D;
  for (int trial = 0; trial < trials + 1; trial++) {
    HIPCHECK(hipEventRecord(ev0, stream));
    const double a = now();
    if (tpamd_planner_set_stop_trajectories_device(ps, B, nullptr, d_t, d_am, 4e-3, d_st, d_keep, d_off, cap, rt, rq, rqd,
                                                   rqdd, stream) != 0) {
      std::printf("{\"error\": \"device stop\"}\n");
      return 1;
    }
    const double enq = now() - a;
    HIPCHECK(hipEventRecord(ev1, stream));
    HIPCHECK(hipEventSynchronize(ev1));
    float ms = 0;
    HIPCHECK(hipEventElapsedTime(&ms, ev0, ev1));
    if (trial > 0) { tc.push_back(ms * 1e-3); tcall.push_back(enq); }
  }
  int64_t total = -1;
  HIPCHECK(hipMemcpy(&total, d_off + B, 8, hipMemcpyDeviceToHost));
  for (void *p : {(void *)d_st, (void *)d_keep, (void *)d_t, (void *)d_off, (void *)d_am, (void *)d_rows})
    HIPCHECK(hipFree(p));
  HIPCHECK(hipStreamDestroy(stream));
  tpamd_planner_set_destroy(ps);
  tpamd_engine_destroy(e);
  std::printf("{\"planners\": %d, \"dofs\": %d, \"trials\": %d, \"stopped_ok\": %d, \"segment_rows\": %zu, "
              "\"device_segment_rows\": %lld, \"set_equals_host_loop\": %d, \"host_loop_ms\": %.3f, "
              "\"set_host_ms\": %.3f, \"set_device_ms\": %.3f, \"set_device_enqueue_ms\": %.3f, "
              "\"speedup_host_call\": %.1f, \"speedup_device\": %.1f}\n",
              B, D, trials, ok, seg_rows, (long long)total, equal, median(ta) * 1e3, median(tb) * 1e3,
              median(tc) * 1e3, median(tcall) * 1e3, median(ta) / median(tb), median(ta) / median(tc));
  return 0;
}

// One control cycle of a planner set's commanded trajectories, run on the GPU machine (g++ -O2
// -std=c++17 -ffp-contract=off -D__HIP_PLATFORM_AMD__ -I<rocm>/include tools/buffer_set_bench.cc
// -L<host> -ltp_host -L<csrc> -ltpamd -L<rocm>/lib -lamdhip64; argv: planners, trials). The
// tools/set_stop_bench.cc workload: 1024 planners x 7 joints, 10 waypoints, N = 1000 path samples,
// 4 ms time step, one Plan(t0, 750 ms). A cycle splices every planner's new trajectory into its
// trajectory buffer, discards the samples before now = start + 100 ms and reads one tick of
// setpoints at now:
//   (a) host_loop     what a caller does without a buffer set: GetTrajectories (one packed
//                     download), then per planner the mirror's InsertSegment /
//                     DiscardSegmentBefore / Get{Position,Velocity,Acceleration}AtTime, one thread
//   (b) set_device    tpamd_buffer_set_insert_from_planner_set_device + discard_before_device +
//                     sample_at_ticks_device on a non-blocking stream into device memory, timed
//                     with HIP events around the three calls, and again with the setpoints
//                     copied to the host
//   (c) set_host      the same three calls through the host-pointer entries
// Times are medians over the trials; bytes are what crosses PCIe per cycle. (b) and (c) must
// equal (a) byte for byte. One JSON line.
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
  const int64_t kMs = 1000000, t0 = 1000 * kMs;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  for (int b = 0; b < B; b++) paths[b] = make_path(D, N, W);
  PathTimingTrajectorySet set(opt, B, 3 * W - 2);
  if (!set.status().ok()) { std::printf("{\"error\": \"no engine\"}\n"); return 1; }
  set.SetPaths(paths);
  set.Plan(FromUnixNanos(t0), Milliseconds(750));
  std::vector<size_t> ids(B);
  std::vector<int64_t> tick(B);
  size_t max_rows = 0, rows = 0;
  for (int b = 0; b < B; b++) {
    ids[b] = b;
    tick[b] = tpamd::compat::ToUnixNanos(set.GetStartTime(b)) + 100 * kMs;
    max_rows = std::max(max_rows, set.GetNumTimeSamples(b));
    rows += set.GetNumTimeSamples(b);
  }

  // (a) the host loop
  std::vector<std::shared_ptr<TrajectoryBuffer>> bufs(B);
  for (auto &m : bufs) m = *TrajectoryBuffer::Create();
  std::vector<double> ta, ref((size_t)B * 3 * D, -1.0);
  for (int trial = 0; trial < trials; trial++) {
    const double a = now();
    std::vector<PlannedTrajectory> traj;
    set.GetTrajectories(ids, &traj);
    for (int b = 0; b < B; b++) {
      const PlannedTrajectory &p = traj[b];
      const size_t n = p.time.size();
      std::vector<VectorXd> q(n), v(n), c(n);
      for (size_t i = 0; i < n; i++) {
        q[i] = VectorXd(&p.positions[i * D], D);
        v[i] = VectorXd(&p.velocities[i * D], D);
        c[i] = VectorXd(&p.accelerations[i * D], D);
      }
      bufs[b]->InsertSegment(p.time, q, v, c);
      const Time at = FromUnixNanos(tick[b]);
      bufs[b]->DiscardSegmentBefore(at);
      const auto sq = bufs[b]->GetPositionAtTime(at), sv = bufs[b]->GetVelocityAtTime(at), sa = bufs[b]->GetAccelerationAtTime(at);
      if (sq.ok() && sv.ok() && sa.ok()) {
        std::memcpy(&ref[((size_t)b * 3 + 0) * D], (*sq).data(), D * 8);
        std::memcpy(&ref[((size_t)b * 3 + 1) * D], (*sv).data(), D * 8);
        std::memcpy(&ref[((size_t)b * 3 + 2) * D], (*sa).data(), D * 8);
      }
    }
    ta.push_back(now() - a);
  }
  // GetTrajectories brings time, s, sd, sdd and q, qd, qdd of every sample down; ids go up
  const size_t host_loop_bytes = rows * (4 + 3 * D) * 8 + (size_t)(B + 1) * 8 + (size_t)B * 4;

  // (b), (c) buffer sets on the planner set's engine
  tpamd_buffer_set *bd = nullptr, *bh = nullptr;
  const int cap = (int)max_rows + 64;
  if (tpamd_buffer_set_create(set.engine(), B, D, cap, 1e-6, &bd) != 0 ||
      tpamd_buffer_set_create(set.engine(), B, D, cap, 1e-6, &bh) != 0) {
    std::printf("{\"error\": \"buffer set\"}\n");
    return 1;
  }
  hipStream_t stream = nullptr;
  HIPCHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  int64_t *d_tick = nullptr;
  int32_t *d_st = nullptr, *d_ts = nullptr;
  double *d_q = nullptr;
  HIPCHECK(hipMalloc(&d_tick, B * 8)); HIPCHECK(hipMalloc(&d_st, B * 4)); HIPCHECK(hipMalloc(&d_ts, B * 4));
  HIPCHECK(hipMalloc(&d_q, (size_t)B * 3 * D * 8));
  HIPCHECK(hipMemcpy(d_tick, tick.data(), B * 8, hipMemcpyHostToDevice));
  double *dq = d_q, *dv = d_q + (size_t)B * D, *da = dv + (size_t)B * D;
  hipEvent_t ev0, ev1;
  HIPCHECK(hipEventCreate(&ev0));
  HIPCHECK(hipEventCreate(&ev1));
  std::vector<double> tb, tb_down, tenq, got((size_t)B * 3 * D);
  std::vector<int32_t> ts(B);
  for (int down = 0; down < 2; down++)
    for (int trial = 0; trial < trials + 1; trial++) {
      HIPCHECK(hipEventRecord(ev0, stream));
      const double a = now();
      int rc = tpamd_buffer_set_insert_from_planner_set_device(bd, set.native_handle(), B, nullptr, nullptr, d_st, stream);
      rc |= tpamd_buffer_set_discard_before_device(bd, B, nullptr, d_tick, nullptr, nullptr, stream);
      rc |= tpamd_buffer_set_sample_at_ticks_device(bd, B, nullptr, d_tick, 4 * kMs, 1, dq, dv, da, d_ts, stream);
      if (rc != 0) { std::printf("{\"error\": \"device cycle\"}\n"); return 1; }
      const double enq = now() - a;
      if (down) {
        HIPCHECK(hipMemcpyAsync(got.data(), d_q, got.size() * 8, hipMemcpyDeviceToHost, stream));
        HIPCHECK(hipMemcpyAsync(ts.data(), d_ts, B * 4, hipMemcpyDeviceToHost, stream));
      }
      HIPCHECK(hipEventRecord(ev1, stream));
      HIPCHECK(hipEventSynchronize(ev1));
      float ms = 0;
      HIPCHECK(hipEventElapsedTime(&ms, ev0, ev1));
      if (trial > 0) { (down ? tb_down : tb).push_back(ms * 1e-3); tenq.push_back(enq); }
    }
  int equal_device = 0, equal_host = 0, ticks_ok = 0;
  for (int b = 0; b < B; b++) {
    ticks_ok += ts[b] == TPAMD_PLAN_OK;
    equal_device += !std::memcmp(&got[(size_t)b * D], &ref[((size_t)b * 3 + 0) * D], D * 8) &&
                    !std::memcmp(&got[((size_t)B + b) * D], &ref[((size_t)b * 3 + 1) * D], D * 8) &&
                    !std::memcmp(&got[((size_t)2 * B + b) * D], &ref[((size_t)b * 3 + 2) * D], D * 8);
  }
  const size_t device_bytes_down = got.size() * 8 + (size_t)B * 4;

  std::vector<double> tc, hq((size_t)B * D, -1.0), hv = hq, ha = hq;
  std::vector<int32_t> st(B), hts(B);
  for (int trial = 0; trial < trials; trial++) {
    const double a = now();
    int rc = tpamd_buffer_set_insert_from_planner_set(bh, set.native_handle(), B, nullptr, nullptr, st.data());
    rc |= tpamd_buffer_set_discard_before(bh, B, nullptr, tick.data(), nullptr);
    rc |= tpamd_buffer_set_sample_at_ticks(bh, B, nullptr, tick.data(), 4 * kMs, 1, hq.data(), hv.data(), ha.data(), hts.data());
    if (rc != 0) { std::printf("{\"error\": \"host cycle\"}\n"); return 1; }
    tc.push_back(now() - a);
  }
  for (int b = 0; b < B; b++)
    equal_host += !std::memcmp(&hq[(size_t)b * D], &ref[((size_t)b * 3 + 0) * D], D * 8) &&
                  !std::memcmp(&hv[(size_t)b * D], &ref[((size_t)b * 3 + 1) * D], D * 8) &&
                  !std::memcmp(&ha[(size_t)b * D], &ref[((size_t)b * 3 + 2) * D], D * 8);
  // host entries: statuses and sample counts down, ticks up, setpoints and tick statuses down
  const size_t host_entry_bytes = (size_t)B * 4 * 3 + (size_t)B * 8 * 2 + device_bytes_down;

  for (void *p : {(void *)d_tick, (void *)d_st, (void *)d_ts, (void *)d_q}) HIPCHECK(hipFree(p));
  HIPCHECK(hipStreamDestroy(stream));
  tpamd_buffer_set_destroy(bd);
  tpamd_buffer_set_destroy(bh);
  std::printf("{\"planners\": %d, \"dofs\": %d, \"trials\": %d, \"trajectory_rows\": %zu, \"ticks_ok\": %d, "
              "\"device_equals_host_loop\": %d, \"host_entries_equal_host_loop\": %d, \"host_loop_ms\": %.3f, "
              "\"set_device_ms\": %.3f, \"set_device_with_setpoints_down_ms\": %.3f, \"set_device_enqueue_ms\": %.3f, "
              "\"set_host_ms\": %.3f, \"host_loop_pcie_bytes\": %zu, \"set_device_pcie_bytes\": 0, "
              "\"set_device_with_setpoints_down_pcie_bytes\": %zu, \"set_host_pcie_bytes\": %zu, "
              "\"speedup_device\": %.1f, \"speedup_host_entries\": %.1f}\n",
              B, D, trials, rows, ticks_ok, equal_device, equal_host, median(ta) * 1e3, median(tb) * 1e3,
              median(tb_down) * 1e3, median(tenq) * 1e3, median(tc) * 1e3, host_loop_bytes, device_bytes_down,
              host_entry_bytes, median(ta) / median(tb), median(ta) / median(tc));
  return 0;
}

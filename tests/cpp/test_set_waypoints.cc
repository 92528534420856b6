// GPU test of the planner-set waypoint fit (run by tests/test_gpu_set_waypoints.py):
// PathTimingTrajectorySet::SetWaypointPaths / tpamd_planner_set_set_waypoints(_device) fit the
// waypoints on the device. For 260-planner sets at D = 3 and 7 with both sampling methods:
//   1. a set fitted on the device against a set loaded by SetPaths from host-fitted paths
//      (TimeableJointSplinePath::SetWaypoints): GetPath bytes, every Plan summary and the
//      GetTrajectories bytes of a whole receding-horizon run;
//   2. mid-motion, a subset gets new waypoints with an initial velocity (the trajectory's velocity
//      at the next start, or zero); every Plan of the set equals one mirror planner per planner
//      given the same calls;
//   4. the per-planner capacity starts below the first paths and grows again for long lists.
// Then through the C-ABI: 3. the _device variant on a non-blocking stream, with a Plan enqueued
// right after it, equals the host variant (per-planner delta, rounding, initial velocity), and
// 5. call-level errors leave GetPath and the next Plan unchanged; a planner without waypoints keeps
// its state.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static std::vector<VectorXd> RandomWaypoints(int W, int D) {
  std::vector<VectorXd> w;
  for (int i = 0; i < W; i++) {
    VectorXd v(D);
    for (int d = 0; d < D; d++) v[d] = 5.0 * Rnd() - 2.5;
    if (i > 0 && Rnd() < 0.1) v = w.back();          // a repeated waypoint now and then
    w.push_back(v);
  }
  return w;
}
static VectorXd RandomVec(int D, double lo, double hi) {
  VectorXd v(D);
  for (int d = 0; d < D; d++) v[d] = lo + (hi - lo) * Rnd();
  return v;
}

// The host flow the device fit replaces: SetWaypoints + limits + SetInitialVelocity on a path
static std::shared_ptr<TimeableJointSplinePath> HostPath(int D, int N, double delta, double rounding,
                                                         const std::vector<VectorXd> &wps, const VectorXd &vmax,
                                                         const VectorXd &amax, const VectorXd *iv) {
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta).set_rounding(rounding));
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  if (iv) CHECK(path->SetInitialVelocity({iv->data(), iv->size()}).ok());
  return path;
}

static bool SameTrajectories(const std::vector<PlannedTrajectory> &a, const std::vector<PlannedTrajectory> &b) {
  if (a.size() != b.size()) return false;
  for (size_t i = 0; i < a.size(); i++)
    if (!SameBits(a[i].time, b[i].time) || !SameBits(a[i].path_parameter, b[i].path_parameter) ||
        !SameBits(a[i].path_parameter_derivative, b[i].path_parameter_derivative) ||
        !SameBits(a[i].second_path_parameter_derivative, b[i].second_path_parameter_derivative) ||
        !SameBits(a[i].positions, b[i].positions) || !SameBits(a[i].velocities, b[i].velocities) ||
        !SameBits(a[i].accelerations, b[i].accelerations))
      return false;
  return true;
}

static void TestAgainstHostFit(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, P0 = 7;               // capacity to start with: below most fits
  const double delta = 0.02, rounding = 0.2;
  g_seed = 3000 + D * 11 + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet dev(opt, B, P0), host(opt, B, P0);
  CHECK(dev.status().ok() && host.status().ok());
  if (!dev.status().ok() || !host.status().ok()) return;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  std::vector<size_t> all(B);
  std::vector<std::vector<VectorXd>> wps(B);
  std::vector<VectorXd> vmax(B), amax(B);
  for (int b = 0; b < B; b++) {
    all[b] = b;
    wps[b] = RandomWaypoints(RndInt(1, 7), D);
    vmax[b] = RandomVec(D, 1.0, 2.0);
    amax[b] = RandomVec(D, 2.0, 4.0);
    paths[b] = HostPath(D, N, delta, rounding, wps[b], vmax[b], amax[b], nullptr);
  }
  // 1. the device fit against SetPaths of the host fits: the resident paths, byte for byte
  const auto st = dev.SetWaypointPaths(all, wps, vmax, amax, {}, rounding, delta);
  int ok = 0;
  for (const auto &s : st) ok += s.ok();
  CHECK(ok == B);
  CHECK(host.SetPaths(paths).ok());
  int same_paths = 0, max_points = 0;
  for (int b = 0; b < B; b++) {
    std::vector<double> k1, c1, k2, c2;
    CHECK(dev.GetPath(b, &k1, &c1).ok() && host.GetPath(b, &k2, &c2).ok());
    same_paths += SameBits(k1, k2) && SameBits(c1, c2) && SameBits(k1, paths[b]->knots());
    max_points = std::max(max_points, (int)dev.NumControlPoints(b));
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  CHECK(same_paths == B);
  CHECK(max_points > P0);
  std::vector<bool> diverged(B, false);
  int64_t start = 2000 * kMs;
  int plans = 0, compared = 0, refits = 0, reported = 0, left_out = 0, long_lists = 0;
  for (int round = 0; round < 14; round++) {
    const bool to_end = round >= 9;
    const int64_t horizon = to_end ? (int64_t)100000 * kMs : 500 * kMs;
    const auto sd = dev.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    const auto sh = host.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    std::vector<PathTimingTrajectory *> batch;
    for (int b = 0; b < B; b++) batch.push_back(mirrors[b].get());
    const auto ms = PathTimingTrajectory::PlanBatch(batch, FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    plans++;
    // the two sets: statuses, summaries, trajectories
    std::vector<PlannedTrajectory> td, th;
    CHECK(dev.GetTrajectories(all, &td).ok() && host.GetTrajectories(all, &th).ok());
    CHECK(SameTrajectories(td, th));
    for (int b = 0; b < B; b++) {
      CHECK(sd[b].code() == sh[b].code());
      CHECK(dev.GetNumTimeSamples(b) == host.GetNumTimeSamples(b) &&
            ToUnixNanos(dev.GetEndTime(b)) == ToUnixNanos(host.GetEndTime(b)) &&
            ToUnixNanos(dev.GetFinalDecelStart(b)) == ToUnixNanos(host.GetFinalDecelStart(b)) &&
            dev.IsTrajectoryAtEnd(b) == host.IsTrajectoryAtEnd(b) && dev.WindowsOfLastPlan(b) == host.WindowsOfLastPlan(b));
      // the set against its mirror planners
      if (diverged[b]) continue;
      CHECK(sd[b].code() == ms[b].code());
      const int bad = CompareOne(dev, b, *mirrors[b], paths[b].get());
      CHECK(bad == 0);
      if (bad && ++reported <= 12)
        std::printf("  D %d %s round %d planner %d: differences 0x%x (status %d / mirror %d)\n", D,
                    skip ? "skip" : "uniform", round, b, bad, (int)sd[b].code(), (int)ms[b].code());
      compared++;
      // a failed first window of a new path leaves it sampled in the set, not in the mirror
      // (DESIGN.md): such planners are compared with the mirror no further
      if (ms[b].code() == StatusCode::kInvalidArgument && sd[b].code() == StatusCode::kInvalidArgument) {
        diverged[b] = true;
        left_out++;
      }
    }
    const int64_t next = start + 150 * kMs;
    if (!to_end && round % 3 == 1) {
      // 2. a seeded subset, mid-motion, gets new waypoints; half of it with the trajectory's
      //    velocity at the next start as initial velocity. Round 7's lists are long (4: growth).
      std::vector<size_t> ids;
      std::vector<std::vector<VectorXd>> nw;
      std::vector<VectorXd> nv, na, niv;
      for (int b = 0; b < B; b++) {
        if (diverged[b] || Rnd() > 0.35) continue;
        VectorXd v(D);
        v.setZero();
        if (b % 2 == 0) {
          const auto at = mirrors[b]->GetVelocityAtTime(FromUnixNanos(next));
          if (at.ok()) v = *at;
        }
        ids.push_back(b);
        const int W = round == 7 ? RndInt(20, 30) : RndInt(1, 6);
        long_lists += round == 7;
        nw.push_back(RandomWaypoints(W, D));
        nv.push_back(RandomVec(D, 1.0, 2.0));
        na.push_back(RandomVec(D, 2.0, 4.0));
        niv.push_back(v);
      }
      const auto got = dev.SetWaypointPaths(ids, nw, nv, na, niv, rounding, delta);
      for (size_t k = 0; k < ids.size(); k++) {
        const int b = (int)ids[k];
        CHECK(got[k].ok());
        paths[b] = HostPath(D, N, delta, rounding, nw[k], nv[k], na[k], &niv[k]);
        CHECK(host.SetPath(b, *paths[b]).ok());
        CHECK(mirrors[b]->SetPath(paths[b]).ok());
        std::vector<double> k1, c1;
        CHECK(dev.GetPath(b, &k1, &c1).ok());
        CHECK(SameBits(k1, paths[b]->knots()) && SameBits(c1, paths[b]->packed_control_points()));
        max_points = std::max(max_points, (int)dev.NumControlPoints(b));
        refits++;
      }
    }
    start = to_end ? start + 3000 * kMs : next;
  }
  int at_end = 0;
  for (int b = 0; b < B; b++) at_end += dev.IsTrajectoryAtEnd(b);
  CHECK(refits > B / 2);
  CHECK(long_lists > 10 && max_points >= 3 * 20 - 2);
  CHECK(at_end > B / 2);
  // a non-zero initial velocity that does not fit the new path's tangent fails the first window
  // (:387-392) alike in the set and the mirror; such planners stay compared between the two sets
  CHECK(left_out < B / 2);
  std::printf("device fit vs host fit and mirrors (D %d, %s): %d plans, resident paths bit-equal, %d planner states "
              "bit-equal to the mirrors, %d refits mid-motion, largest P %d (capacity started at %d), %d at the end, "
              "%d left out after a failed first window\n",
              D, skip ? "skip" : "uniform", plans, compared, refits, max_points, P0, at_end, left_out);
}

// 3. and 5. through the C-ABI
static void TestCAbi(int D, int method) {
  const int B = 260, N = 200;
  g_seed = 555 + D + method;
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) return;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 4;
  cfg.sampling_method = method; cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = method ? 4 * kMs : kMs;
  tpamd_planner_set *h = nullptr, *d = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &h) == 0 && tpamd_planner_set_create(e, &cfg, &d) == 0);
  if (!h || !d) return;
  // every other planner, in a shuffled order; one without waypoints
  std::vector<int32_t> ids, offsets = {0};
  std::vector<double> wps, vmax, amax, delta, iv;
  for (int b = 0; b < B; b += 2) ids.push_back(b);
  for (size_t i = ids.size() - 1; i > 0; i--) std::swap(ids[i], ids[RndInt(0, (int)i)]);
  const int n = (int)ids.size(), empty_k = 5;
  for (int k = 0; k < n; k++) {
    const int W = k == empty_k ? 0 : RndInt(1, 9);
    for (const auto &w : RandomWaypoints(W, D)) wps.insert(wps.end(), w.begin(), w.end());
    offsets.push_back(offsets.back() + W);
    for (int j = 0; j < D; j++) {
      vmax.push_back(1.0 + Rnd()); amax.push_back(2.0 + 2.0 * Rnd()); iv.push_back(0.0);
    }
    delta.push_back(0.01 + 0.02 * Rnd());
  }
  const double rounding = 0.35;
  std::vector<int32_t> np_h(n, -1), st_h(n, -1), np_d(n, -1), st_d(n, -1);
  CHECK(tpamd_planner_set_set_waypoints(h, n, ids.data(), offsets.data(), wps.data(), rounding, vmax.data(), amax.data(),
                                        delta.data(), iv.data(), np_h.data(), st_h.data()) == 0);
  for (int k = 0; k < n; k++) {
    const int W = offsets[k + 1] - offsets[k];
    CHECK(st_h[k] == (W ? TPAMD_PLAN_OK : TPAMD_PLAN_INVALID_ARGUMENT));
    CHECK(np_h[k] == (W ? (W == 1 ? 4 : 3 * W - 2) : 0));
  }
  // the device variant: inputs in device memory, a non-blocking stream, a Plan enqueued right after
  double *d_wps = nullptr, *d_vmax = nullptr, *d_amax = nullptr, *d_delta = nullptr, *d_iv = nullptr;
  int32_t *d_np = nullptr, *d_st = nullptr;
  HIP_OK(hipMalloc(&d_wps, wps.size() * 8)); HIP_OK(hipMalloc(&d_vmax, vmax.size() * 8));
  HIP_OK(hipMalloc(&d_amax, amax.size() * 8)); HIP_OK(hipMalloc(&d_delta, delta.size() * 8));
  HIP_OK(hipMalloc(&d_iv, iv.size() * 8)); HIP_OK(hipMalloc(&d_np, n * 4)); HIP_OK(hipMalloc(&d_st, n * 4));
  HIP_OK(hipMemcpy(d_wps, wps.data(), wps.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_vmax, vmax.data(), vmax.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_amax, amax.data(), amax.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_delta, delta.data(), delta.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_iv, iv.data(), iv.size() * 8, hipMemcpyHostToDevice));
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  // the initial velocity NULL on the device side: zero, as the host's zeros
  CHECK(tpamd_planner_set_set_waypoints_device(d, n, ids.data(), offsets.data(), d_wps, rounding, d_vmax, d_amax,
                                               d_delta, nullptr, d_np, d_st, stream) == 0);
  std::vector<int64_t> s(B, 1000 * kMs), hz(B, 400 * kMs);
  std::vector<tpamd_planner_summary> sum_h(B), sum_d(B);
  CHECK(tpamd_planner_set_plan(d, s.data(), hz.data(), sum_d.data()) == 0);
  CHECK(tpamd_planner_set_plan(h, s.data(), hz.data(), sum_h.data()) == 0);
  CHECK(std::memcmp(sum_h.data(), sum_d.data(), B * sizeof(tpamd_planner_summary)) == 0);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipMemcpy(np_d.data(), d_np, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(st_d.data(), d_st, n * 4, hipMemcpyDeviceToHost));
  CHECK(np_d == np_h && st_d == st_h);
  int planned = 0;
  for (int b = 0; b < B; b++) planned += sum_h[b].status == TPAMD_PLAN_OK;
  CHECK(planned > B / 4);
  auto path_of = [&](tpamd_planner_set *ps, int b, std::vector<double> *k, std::vector<double> *c) {
    int32_t P = 0;
    CHECK(tpamd_planner_set_download_path(ps, b, &P, nullptr, nullptr, 0) == 0);
    k->assign(P ? P + 3 : 0, 0.0);
    c->assign((size_t)P * D, 0.0);
    if (P) CHECK(tpamd_planner_set_download_path(ps, b, &P, k->data(), c->data(), P) == 0);
    return P;
  };
  auto trajectories = [&](tpamd_planner_set *ps) {
    std::vector<int64_t> off(B + 1);
    CHECK(tpamd_planner_set_download_trajectories(ps, B, nullptr, off.data(), 0, nullptr, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, nullptr) == (off[B] > 0 ? TPAMD_E_INVALID_ARGUMENT : 0));
    const size_t rows = off[B];
    std::vector<double> all(rows * (4 + 3 * D));
    double *p = all.data();
    CHECK(tpamd_planner_set_download_trajectories(ps, B, nullptr, off.data(), rows, p, p + rows, p + 2 * rows,
                                                  p + 3 * rows, p + 4 * rows, p + (4 + D) * rows,
                                                  p + (4 + 2 * D) * rows) == 0);
    return all;
  };
  int same = 0;
  for (int b = 0; b < B; b++) {
    std::vector<double> k1, c1, k2, c2;
    const int P1 = path_of(h, b, &k1, &c1), P2 = path_of(d, b, &k2, &c2);
    same += P1 == P2 && SameBits(k1, k2) && SameBits(c1, c2);
  }
  CHECK(same == B);
  CHECK(trajectories(h) == trajectories(d));
  // 5. call-level errors: nothing changes, the next Plan is the twin's
  std::vector<int32_t> bad_ids = {0, 2, 0}, off3 = {0, 2, 4, 6};
  std::vector<double> w3(6 * D, 0.5), v3(3 * D, 1.5), a3(3 * D, 3.0), dl3(3, 0.01);
  std::vector<int32_t> np3(3), st3(3, -7);
  tpamd_planner_set *sets[2] = {h, d};
  for (tpamd_planner_set *ps : sets) {
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, bad_ids.data(), off3.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    std::vector<int32_t> out_ids = {1, 3, B};
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, out_ids.data(), off3.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    std::vector<int32_t> ok_ids = {1, 3, 5}, off_bad0 = {1, 2, 4, 6}, off_dec = {0, 4, 2, 6};
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, ok_ids.data(), off_bad0.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, ok_ids.data(), off_dec.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, ok_ids.data(), off3.data(), w3.data(), 0.2, nullptr, a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints(ps, 3, ok_ids.data(), off3.data(), nullptr, 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), nullptr) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints(ps, B + 1, nullptr, off3.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                          dl3.data(), nullptr, np3.data(), st3.data()) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints_device(ps, 3, bad_ids.data(), off3.data(), d_wps, 0.2, d_vmax, d_amax,
                                                 d_delta, nullptr, d_np, d_st, stream) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_set_waypoints_device(ps, 3, ok_ids.data(), off_dec.data(), d_wps, 0.2, d_vmax, d_amax,
                                                 d_delta, nullptr, d_np, d_st, stream) == TPAMD_E_INVALID_ARGUMENT);
  }
  CHECK(st3[0] == -7);
  // a set that saw only the errors against its twin that saw none
  tpamd_planner_set *twin = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &twin) == 0);
  CHECK(tpamd_planner_set_set_waypoints(twin, n, ids.data(), offsets.data(), wps.data(), rounding, vmax.data(),
                                        amax.data(), delta.data(), iv.data(), np_h.data(), st_h.data()) == 0);
  CHECK(tpamd_planner_set_plan(twin, s.data(), hz.data(), sum_h.data()) == 0);
  std::vector<int64_t> s2(B, 1150 * kMs), hz2(B, 400 * kMs);
  std::vector<tpamd_planner_summary> sum_t(B);
  CHECK(tpamd_planner_set_plan(h, s2.data(), hz2.data(), sum_h.data()) == 0);
  CHECK(tpamd_planner_set_plan(d, s2.data(), hz2.data(), sum_d.data()) == 0);
  CHECK(tpamd_planner_set_plan(twin, s2.data(), hz2.data(), sum_t.data()) == 0);
  CHECK(std::memcmp(sum_h.data(), sum_t.data(), B * sizeof(tpamd_planner_summary)) == 0);
  CHECK(std::memcmp(sum_d.data(), sum_t.data(), B * sizeof(tpamd_planner_summary)) == 0);
  for (int b = 0; b < B; b++) {
    std::vector<double> k1, c1, k2, c2;
    path_of(h, b, &k1, &c1);
    path_of(twin, b, &k2, &c2);
    CHECK(SameBits(k1, k2) && SameBits(c1, c2));
  }
  CHECK(trajectories(d) == trajectories(twin));
  // the planner without waypoints kept "no path": its Plan fails as before any path
  CHECK(sum_t[ids[empty_k]].status == TPAMD_PLAN_FAILED_PRECONDITION);
  // a later fit replaces a planner's path and state (a device fit on the default stream, then a
  // host readout of the path without a synchronisation in between)
  std::vector<int32_t> one = {ids[0]}, off1 = {0, 2};
  CHECK(tpamd_planner_set_set_waypoints_device(d, 1, one.data(), off1.data(), d_wps, 0.0, d_vmax, d_amax, d_delta,
                                               d_iv, nullptr, d_st, nullptr) == 0);
  std::vector<double> k1, c1;
  CHECK(path_of(d, ids[0], &k1, &c1) == 4);
  CHECK(SameBits(std::vector<double>(c1.begin(), c1.begin() + D), std::vector<double>(wps.begin(), wps.begin() + D)));
  HIP_OK(hipStreamDestroy(stream));
  for (void *p : {(void *)d_wps, (void *)d_vmax, (void *)d_amax, (void *)d_delta, (void *)d_iv, (void *)d_np, (void *)d_st})
    HIP_OK(hipFree(p));
  tpamd_planner_set_destroy(twin);
  tpamd_planner_set_destroy(h);
  tpamd_planner_set_destroy(d);
  tpamd_engine_destroy(e);
  std::printf("set_waypoints C-ABI (D %d, method %d): device variant on a non-blocking stream = host variant, "
              "%d planners planned, call-level errors changed nothing\n", D, method, planned);
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) TestAgainstHostFit(m, D);
  for (int D : {3, 7})
    for (int m : {0, 1}) TestCAbi(D, m);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

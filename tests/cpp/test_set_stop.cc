// GPU test of the stopping trajectories (run by tests/test_gpu_set_stop.py):
//   PathTimingTrajectorySet::StopTrajectoriesBeforeTime (tpamd_planner_set_stop_trajectories)
//   against the mirror: each planner's GetTrajectory loaded into a TrajectoryBuffer
//   (host/trajectory_buffer.h) and stopped with StopBeforeTime; keep + segment must equal the
//   buffer's contents byte for byte, with the same status. 260-planner sets at D = 3 and 7, both
//   sampling methods, several Plan rounds, stop times before the first sample, on a sample,
//   between samples, on the last sample and past the end, planners that never get a path,
//   feasible and infeasible max_acceleration. A twin set that never stops must plan the same.
//   The C-ABI: the _device variant on a non-blocking stream with a Plan enqueued right after it
//   equals the host variant; a too-small capacity, bad ids and the call-level errors.
//   The batch form (tpamd_stop_trajectories_*) on solver outputs (BatchPathTiming) and on their
//   resampled rows (tpamd_resample_uniform_host / _skip_host, ragged counts) at D = 3, 7, 14, by
//   time and by index, against the mirror; rows outside [first, last] stay untouched.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_path_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::StatusCode;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

// equal bytes; a NaN equals a NaN whatever its payload (host and device may make different ones)
static bool SameBitsOrNaN(const double *a, const double *b, size_t n) {
  if (n == 0 || std::memcmp(a, b, n * 8) == 0) return true;
  for (size_t i = 0; i < n; i++)
    if (std::memcmp(a + i, b + i, 8) != 0 && !(std::isnan(a[i]) && std::isnan(b[i]))) return false;
  return true;
}

static std::shared_ptr<TimeableJointSplinePath> RandomPath(int D, int N, int W, double fraction) {
  std::vector<VectorXd> wps;
  for (int i = 0; i < W; i++) {
    VectorXd v(D);
    for (int d = 0; d < D; d++) v[d] = 5.0 * Rnd() - 2.5;
    wps.push_back(v);
  }
  auto probe = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
  probe->SetWaypoints({wps.data(), wps.size()});
  const double delta = fraction * probe->knots().back() / (N - 1);
  auto path = std::make_shared<TimeableJointSplinePath>(
      JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta));
  std::vector<double> vmax(D), amax(D);
  for (int d = 0; d < D; d++) { vmax[d] = 1.0 + Rnd(); amax[d] = 2.0 + 2.0 * Rnd(); }
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  CHECK(path->SetWaypoints({wps.data(), wps.size()}).ok());
  return path;
}

static int Code(const Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return TPAMD_PLAN_OK;
    case StatusCode::kFailedPrecondition: return TPAMD_PLAN_FAILED_PRECONDITION;
    case StatusCode::kOutOfRange: return TPAMD_PLAN_OUT_OF_RANGE;
    case StatusCode::kInvalidArgument: return TPAMD_PLAN_INVALID_ARGUMENT;
    case StatusCode::kNotFound: return TPAMD_PLAN_NOT_FOUND;
    default: return TPAMD_PLAN_INTERNAL;
  }
}

// A trajectory given as rows: time [n], q / qd / qdd [n][D]
struct Rows {
  const double *t, *q, *qd, *qdd;
  int n, D;
};

// The mirror's stop on rows: the buffer after it (packed) and the status
struct MirrorStop {
  int status;
  std::vector<double> t, q, qd, qdd;
};
static MirrorStop Mirror(const Rows &r, bool by_index, int index, double time_sec, const double *amax, double time_step) {
  std::vector<VectorXd> Q(r.n), V(r.n), A(r.n);
  for (int i = 0; i < r.n; i++) {
    Q[i] = VectorXd(r.q + (size_t)i * r.D, r.D);
    V[i] = VectorXd(r.qd + (size_t)i * r.D, r.D);
    A[i] = VectorXd(r.qdd + (size_t)i * r.D, r.D);
  }
  auto buf = *TrajectoryBuffer::Create();
  CHECK(buf->InsertSegment(Span<const double>(r.t, r.n), Span<const VectorXd>(Q.data(), r.n),
                           Span<const VectorXd>(V.data(), r.n), Span<const VectorXd>(A.data(), r.n))
            .ok());
  const VectorXd am(amax, r.D);
  MirrorStop m;
  m.status = Code(by_index ? buf->StopAtIndex(index, am, time_step) : buf->StopBeforeTime(time_sec, am, time_step));
  for (size_t i = 0; i < buf->GetNumSamples(); i++) {
    m.t.push_back(buf->GetTimes()[i]);
    m.q.insert(m.q.end(), buf->GetPositions()[i].begin(), buf->GetPositions()[i].end());
    m.qd.insert(m.qd.end(), buf->GetVelocities()[i].begin(), buf->GetVelocities()[i].end());
    m.qdd.insert(m.qdd.end(), buf->GetAccelerations()[i].begin(), buf->GetAccelerations()[i].end());
  }
  return m;
}

// rows[0, keep) ++ segment against the mirror's buffer
static bool SameStop(const MirrorStop &m, const Rows &r, int keep, const double *st, const double *sq, const double *sqd,
                     const double *sqdd, int seg) {
  const int D = r.D;
  if (keep < 0 || keep > r.n || seg < 0 || (size_t)(keep + seg) != m.t.size()) return false;
  return SameBitsOrNaN(m.t.data(), r.t, keep) && SameBitsOrNaN(m.q.data(), r.q, (size_t)keep * D) &&
         SameBitsOrNaN(m.qd.data(), r.qd, (size_t)keep * D) && SameBitsOrNaN(m.qdd.data(), r.qdd, (size_t)keep * D) &&
         SameBitsOrNaN(m.t.data() + keep, st, seg) && SameBitsOrNaN(m.q.data() + (size_t)keep * D, sq, (size_t)seg * D) &&
         SameBitsOrNaN(m.qd.data() + (size_t)keep * D, sqd, (size_t)seg * D) &&
         SameBitsOrNaN(m.qdd.data() + (size_t)keep * D, sqdd, (size_t)seg * D);
}

// A stop time for a trajectory: before it, on a sample, between two, on the last, past the end
static int64_t StopTimeNs(const std::vector<double> &t, int kind, int64_t fallback) {
  if (t.empty()) return fallback;
  const int n = (int)t.size(), i = RndInt(0, n - 1);
  const double s = kind == 0 ? t[0] - 0.003 : kind == 1 ? t[i] : kind == 2 && i + 1 < n ? 0.5 * (t[i] + t[i + 1])
                   : kind == 3 ? t[n - 1] : t[n - 1] + 0.25;
  // a time stamp of the trajectory as nanoseconds: the nearest, so that ns / 1e9 lands on or near it
  return (int64_t)std::llround(s * 1e9);
}

static void TestSetAgainstMirror(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, with_path = 250;
  g_seed = 7000 + D * 7 + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet set(opt, B, 7), twin(opt, B, 7);
  CHECK(set.status().ok() && twin.status().ok());
  if (!set.status().ok() || !twin.status().ok()) return;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(with_path);
  for (int b = 0; b < with_path; b++) paths[b] = RandomPath(D, N, RndInt(3, 7), 0.3 + 0.4 * (b % 7) / 7.0);
  CHECK(set.SetPaths(paths).ok() && twin.SetPaths(paths).ok());
  std::vector<size_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  long long cat[8] = {0};     // ok, ok after rate 1, used all, not found, out of range, invalid, last at rest, empty
  int64_t start = 2000 * kMs;
  int rounds = 0;
  for (int round = 0; round < 6; round++, rounds++) {
    const bool to_end = round >= 4;
    const int64_t horizon = to_end ? (int64_t)100000 * kMs : 500 * kMs;
    const auto st = set.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    const auto tw = twin.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    CHECK(set.LastPlanBytesOverPcie() == twin.LastPlanBytesOverPcie());
    for (int b = 0; b < B; b++) {
      CHECK(st[b].code() == tw[b].code());
      CHECK(set.GetNumTimeSamples(b) == twin.GetNumTimeSamples(b));
      CHECK(set.GetEndTime(b) == twin.GetEndTime(b));
    }
    std::vector<PlannedTrajectory> tr(B);
    std::vector<Time> times(B);
    std::vector<VectorXd> amax(B);
    for (int b = 0; b < B; b++) {
      CHECK(set.GetTrajectory(b, &tr[b]).ok());
      times[b] = FromUnixNanos(StopTimeNs(tr[b].time, (b + round) % 5, start));
      amax[b] = VectorXd(D);
      const double scale = (b % 4 == 0) ? 0.05 : 1.0 + 3.0 * Rnd();       // infeasible / feasible
      for (int d = 0; d < D; d++) amax[b][d] = scale * (b < with_path ? paths[b]->GetMaxJointAcceleration()[d] : 1.0);
    }
    const double time_step = round == 2 ? -1e-3 : 1e-3;
    std::vector<StoppingSegment> segs;
    CHECK(set.StopTrajectoriesBeforeTime(all, times, amax, time_step, &segs).ok());
    if (segs.size() != (size_t)B) return;
    for (int b = 0; b < B; b++) {
      const PlannedTrajectory &p = tr[b];
      const Rows r{p.time.data(), p.positions.data(), p.velocities.data(), p.accelerations.data(), (int)p.time.size(), D};
      const MirrorStop m = Mirror(r, false, 0, (double)tpamd::compat::ToUnixNanos(times[b]) / 1e9, amax[b].data(), time_step);
      const StoppingSegment &s = segs[b];
      CHECK(Code(s.status) == m.status);
      const bool same = SameStop(m, r, (int)s.keep, s.time.data(), s.positions.data(), s.velocities.data(),
                                 s.accelerations.data(), (int)s.time.size());
      CHECK(same);
      if (!same && g_fail < 45)
        std::printf("  planner %d round %d: n %d status %d/%d keep %zu rows %zu, mirror %zu\n", b, round, r.n,
                    Code(s.status), m.status, s.keep, s.time.size(), m.t.size());
      if (r.n == 0) cat[7]++;
      else if (m.status == TPAMD_PLAN_OK && s.time.size() == 1 && s.keep + 1 == (size_t)r.n) cat[6]++;
      else if (m.status == TPAMD_PLAN_OK) cat[s.keep > 1 ? 1 : 2]++, cat[0]++;
      else if (m.status == TPAMD_PLAN_NOT_FOUND) cat[3]++;
      else if (m.status == TPAMD_PLAN_OUT_OF_RANGE) cat[4]++;
      else if (m.status == TPAMD_PLAN_INVALID_ARGUMENT) cat[5]++;
    }
    // the stop changes nothing: the next Plan equals the twin's
    start = to_end ? start + 3000 * kMs : start + 200 * kMs;
  }
  for (int b = 0; b < B; b++) {
    PlannedTrajectory a, c;
    CHECK(set.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok());
    CHECK(SameBitsOrNaN(a.time.data(), c.time.data(), a.time.size()) && a.time.size() == c.time.size() &&
          SameBitsOrNaN(a.positions.data(), c.positions.data(), a.positions.size()) &&
          SameBitsOrNaN(a.velocities.data(), c.velocities.data(), a.velocities.size()));
  }
  CHECK(cat[0] > 100 && cat[3] > 20 && cat[4] > 20 && cat[5] > 20 && cat[7] > 20);
  // errors of the call
  std::vector<StoppingSegment> segs;
  CHECK(!set.StopTrajectoriesBeforeTime({(size_t)B}, {FromUnixNanos(start)}, {VectorXd(D, 1.0)}, 1e-3, &segs).ok());
  CHECK(!set.StopTrajectoriesBeforeTime({0}, {FromUnixNanos(start)}, {VectorXd(D + 1, 1.0)}, 1e-3, &segs).ok());
  CHECK(!set.StopTrajectoriesBeforeTime({0}, {}, {VectorXd(D, 1.0)}, 1e-3, &segs).ok());
  std::printf("stop vs mirror (D %d, %s): %d rounds, ok %lld (keep > 1: %lld), not found %lld, out of range %lld, "
              "invalid %lld, last at rest %lld, no samples %lld\n",
              D, skip ? "skip" : "uniform", rounds, cat[0], cat[1], cat[3], cat[4], cat[5], cat[6], cat[7]);
}

// ------------------------------------------------------------------ the planner-set C-ABI
static void TestSetCabi(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, with_path = 250;
  g_seed = 9000 + D + (skip ? 1 : 0);
  const int64_t step_ts = skip ? 4 * kMs : kMs;
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) return;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 7;
  cfg.sampling_method = skip ? 1 : 0;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = step_ts;
  tpamd_planner_set *ps = nullptr, *twin = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &ps) == 0 && tpamd_planner_set_create(e, &cfg, &twin) == 0);
  if (!ps || !twin) return;
  std::vector<double> path_amax;
  {
    std::vector<int32_t> np(with_path), state(with_path, 1);
    std::vector<double> knots, cps, vmax, delta, iv(with_path * D, 0.0);
    for (int b = 0; b < with_path; b++) {
      auto p = RandomPath(D, N, RndInt(3, 7), 0.3 + 0.4 * (b % 7) / 7.0);
      np[b] = p->num_control_points();
      knots.insert(knots.end(), p->knots().begin(), p->knots().end());
      cps.insert(cps.end(), p->packed_control_points().begin(), p->packed_control_points().end());
      vmax.insert(vmax.end(), p->GetMaxJointVelocity().begin(), p->GetMaxJointVelocity().end());
      path_amax.insert(path_amax.end(), p->GetMaxJointAcceleration().begin(), p->GetMaxJointAcceleration().end());
      delta.push_back(p->GetPathSamplingDistance());
    }
    for (tpamd_planner_set *s : {ps, twin})
      CHECK(tpamd_planner_set_upload_paths_ragged(s, with_path, nullptr, np.data(), knots.data(), cps.data(), vmax.data(),
                                                  path_amax.data(), delta.data(), iv.data(), state.data()) == 0);
  }
  std::vector<tpamd_planner_summary> sum(B), sum_twin(B);
  int64_t start = 1000 * kMs;
  auto plan_both = [&](int64_t s0, int64_t h) {
    std::vector<int64_t> s(B, s0), hz(B, h);
    CHECK(tpamd_planner_set_plan(ps, s.data(), hz.data(), sum.data()) == 0);
    CHECK(tpamd_planner_set_plan(twin, s.data(), hz.data(), sum_twin.data()) == 0);
    CHECK(std::memcmp(sum.data(), sum_twin.data(), B * sizeof(tpamd_planner_summary)) == 0);
  };
  plan_both(start, 500 * kMs);
  const double kSentinel = -12345.0;
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  int rounds = 0, tot_ok = 0, tot_nf = 0;
  for (int round = 0; round < 3; round++, rounds++) {
    std::vector<int32_t> ids;
    for (int b = 0; b < B; b++) ids.push_back((b * 37 + round) % B);
    ids.push_back(3); ids.push_back(3); ids.push_back(259);
    const int n = (int)ids.size();
    std::vector<int64_t> tns(n);
    std::vector<double> am((size_t)n * D);
    for (int k = 0; k < n; k++) {
      const tpamd_planner_summary &s = sum[ids[k]];
      const int kind = k % 4;
      tns[k] = kind == 0 ? s.start_time_ns - 5 * step_ts : kind == 1 ? s.start_time_ns + 37 * step_ts
               : kind == 2 ? s.end_time_ns : s.start_time_ns + (s.end_time_ns - s.start_time_ns) / 2;
      for (int d = 0; d < D; d++)
        am[(size_t)k * D + d] = ids[k] < with_path ? path_amax[(size_t)ids[k] * D + d] * (k % 5 == 0 ? 0.1 : 2.0) : 1.0;
    }
    // host variant: first with no room, then with room
    std::vector<int32_t> hst(n, -9), hkeep(n, -9);
    std::vector<int64_t> hoff(n + 1, -1);
    double t0 = kSentinel;
    CHECK(tpamd_planner_set_stop_trajectories(ps, n, ids.data(), tns.data(), am.data(), 1e-3, hst.data(), hkeep.data(),
                                              hoff.data(), 0, &t0, nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(hoff[0] == 0 && hoff[n] > 0 && t0 == kSentinel);
    const int64_t total = hoff[n];
    std::vector<double> ht(total), hq(total * D), hqd(total * D), hqdd(total * D);
    CHECK(tpamd_planner_set_stop_trajectories(ps, n, ids.data(), tns.data(), am.data(), 1e-3, hst.data(), hkeep.data(),
                                              hoff.data(), total, ht.data(), hq.data(), hqd.data(), hqdd.data()) == 0);
    int ok = 0, nf = 0;
    for (int k = 0; k < n; k++) {       // each planner against the mirror on its own download
      const int c = sum[ids[k]].num_samples;
      std::vector<double> t1(c), q1(c * D), v1(c * D), a1(c * D);
      if (c > 0)
        CHECK(tpamd_planner_set_download_trajectory(ps, ids[k], 0, c, t1.data(), nullptr, nullptr, nullptr, q1.data(),
                                                    v1.data(), a1.data()) == 0);
      const Rows r{t1.data(), q1.data(), v1.data(), a1.data(), c, D};
      const MirrorStop m = Mirror(r, false, 0, (double)tns[k] / 1e9, &am[(size_t)k * D], 1e-3);
      CHECK(hst[k] == m.status);
      const size_t o = hoff[k];
      CHECK(SameStop(m, r, hkeep[k], ht.data() + o, hq.data() + o * D, hqd.data() + o * D, hqdd.data() + o * D,
                     (int)(hoff[k + 1] - hoff[k])));
      ok += hst[k] == TPAMD_PLAN_OK;
      nf += hst[k] == TPAMD_PLAN_NOT_FOUND;
    }
    tot_ok += ok;
    tot_nf += nf;
    CHECK(hst[n - 1] == TPAMD_PLAN_OK && hkeep[n - 1] == 0 && hoff[n] == hoff[n - 1]);     // never planned
    // device variant on a non-blocking stream, bad ids appended, a Plan enqueued right after
    std::vector<int32_t> dids = ids;
    dids.push_back(-1); dids.push_back(B);
    std::vector<int64_t> dtns = tns;
    dtns.push_back(start); dtns.push_back(start);
    std::vector<double> dam = am;
    dam.resize((size_t)(n + 2) * D, 1.0);
    const int dn = n + 2;
    int32_t *d_ids = nullptr, *d_res = nullptr;
    int64_t *d_t = nullptr, *d_off = nullptr, *d_off2 = nullptr;
    double *d_am = nullptr, *d_rows = nullptr, *d_rows2 = nullptr;
    HIP_OK(hipMalloc(&d_ids, dn * 4)); HIP_OK(hipMalloc(&d_t, dn * 8)); HIP_OK(hipMalloc(&d_am, dn * D * 8));
    HIP_OK(hipMalloc(&d_res, 4 * dn * 4)); HIP_OK(hipMalloc(&d_off, (dn + 1) * 8)); HIP_OK(hipMalloc(&d_off2, (dn + 1) * 8));
    HIP_OK(hipMalloc(&d_rows, (size_t)total * (1 + 3 * D) * 8)); HIP_OK(hipMalloc(&d_rows2, (size_t)total * 8));
    std::vector<double> sent((size_t)total * (1 + 3 * D), kSentinel);
    HIP_OK(hipMemcpy(d_ids, dids.data(), dn * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_t, dtns.data(), dn * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_am, dam.data(), dn * D * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rows, sent.data(), sent.size() * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rows2, sent.data(), (size_t)total * 8, hipMemcpyHostToDevice));
    double *rt = d_rows, *rq = rt + total, *rqd = rq + total * D, *rqdd = rqd + total * D;
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, dn, d_ids, d_t, d_am, 1e-3, d_res, d_res + dn, d_off, total, rt,
                                                     rq, rqd, rqdd, stream) == 0);
    // a too-small capacity: statuses and offsets written, no row
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, dn, d_ids, d_t, d_am, 1e-3, d_res + 2 * dn, d_res + 3 * dn, d_off2,
                                                     total - 1, d_rows2, nullptr, nullptr, nullptr, stream) == 0);
    start += 150 * kMs;
    plan_both(start, 500 * kMs);          // must not overwrite what the stops are still reading
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<int32_t> gres(4 * dn);
    std::vector<int64_t> goff(dn + 1), goff2(dn + 1);
    std::vector<double> grows(sent.size()), grows2(total);
    HIP_OK(hipMemcpy(gres.data(), d_res, 4 * dn * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(goff.data(), d_off, (dn + 1) * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(goff2.data(), d_off2, (dn + 1) * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(grows.data(), d_rows, grows.size() * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(grows2.data(), d_rows2, grows2.size() * 8, hipMemcpyDeviceToHost));
    CHECK(std::memcmp(gres.data(), hst.data(), n * 4) == 0 && std::memcmp(gres.data() + dn, hkeep.data(), n * 4) == 0);
    CHECK(std::memcmp(gres.data() + 2 * dn, gres.data(), 2 * dn * 4) == 0);
    for (int k = n; k < dn; k++) CHECK(gres[k] == TPAMD_PLAN_INVALID_ARGUMENT && gres[dn + k] == 0);
    CHECK(std::memcmp(goff.data(), hoff.data(), (n + 1) * 8) == 0 && goff[n + 1] == total && goff[n + 2] == total);
    CHECK(std::memcmp(goff2.data(), goff.data(), (dn + 1) * 8) == 0);
    CHECK(SameBitsOrNaN(grows.data(), ht.data(), total) && SameBitsOrNaN(grows.data() + total, hq.data(), total * D) &&
          SameBitsOrNaN(grows.data() + total + total * D, hqd.data(), total * D) &&
          SameBitsOrNaN(grows.data() + total + 2 * total * D, hqdd.data(), total * D));
    bool untouched = true;
    for (double v : grows2) untouched &= v == kSentinel;
    CHECK(untouched);
    for (void *p : {(void *)d_ids, (void *)d_t, (void *)d_am, (void *)d_res, (void *)d_off, (void *)d_off2, (void *)d_rows,
                    (void *)d_rows2})
      HIP_OK(hipFree(p));
  }
  // count = 0 writes offsets[0] = 0 (host and device)
  {
    int64_t off0 = -1;
    int32_t s0 = -9, k0 = -9;
    double a0 = 1.0;
    CHECK(tpamd_planner_set_stop_trajectories(ps, 0, nullptr, &start, &a0, 1e-3, &s0, &k0, &off0, 0, nullptr, nullptr,
                                              nullptr, nullptr) == 0 && off0 == 0 && s0 == -9);
    int64_t *d_off = nullptr;
    HIP_OK(hipMalloc(&d_off, 8));
    HIP_OK(hipMemcpy(d_off, &off0, 8, hipMemcpyHostToDevice));
    off0 = -1;
    HIP_OK(hipMemcpy(d_off, &off0, 8, hipMemcpyHostToDevice));
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, 0, nullptr, (const int64_t *)d_off, (const double *)d_off, 1e-3,
                                                     (int32_t *)d_off, (int32_t *)d_off, d_off, 0, nullptr, nullptr,
                                                     nullptr, nullptr, stream) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(&off0, d_off, 8, hipMemcpyDeviceToHost));
    CHECK(off0 == 0);
    HIP_OK(hipFree(d_off));
  }
  // call-level errors change nothing
  {
    const int32_t good[2] = {0, 1}, bad[2] = {0, B};
    const int64_t t2[2] = {start, start};
    std::vector<double> a2(2 * D, 1.0);
    int32_t st[2] = {-9, -9}, kp[2] = {-9, -9};
    int64_t off[3] = {-1, -1, -1};
    double rows[4] = {kSentinel, kSentinel, kSentinel, kSentinel};
    const double *am = a2.data();
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, bad, t2, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, -1, good, t2, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, B + 1, nullptr, t2, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(nullptr, 2, good, t2, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, nullptr, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, t2, nullptr, 1e-3, st, kp, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, t2, am, 1e-3, nullptr, kp, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, t2, am, 1e-3, st, nullptr, off, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, t2, am, 1e-3, st, kp, nullptr, 4, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories(ps, 2, good, t2, am, 1e-3, st, kp, off, -1, rows, 0, 0, 0) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, 2, good, t2, am, 1e-3, st, kp, nullptr, 4, rows, 0, 0, 0,
                                                     stream) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_stop_trajectories_device(ps, B + 1, nullptr, t2, am, 1e-3, st, kp, off, 4, rows, 0, 0, 0,
                                                     stream) == TPAMD_E_INVALID_ARGUMENT);
    bool untouched = off[0] == -1 && off[2] == -1 && st[0] == -9 && kp[1] == -9;
    for (double v : rows) untouched &= v == kSentinel;
    CHECK(untouched);
  }
  HIP_OK(hipStreamDestroy(stream));
  tpamd_planner_set_destroy(ps);
  tpamd_planner_set_destroy(twin);
  tpamd_engine_destroy(e);
  CHECK(tot_ok > 150 && tot_nf > 0);
  std::printf("stop C-ABI (D %d, %s): %d rounds of device stops with a Plan right after (ok %d, not found %d), "
              "errors ok\n", D, skip ? "skip" : "uniform", rounds, tot_ok, tot_nf);
}

// ------------------------------------------------------------------ the batch form
// One batch call (host entry, and the device entry on the same rows) against the mirror per row.
static void CheckBatch(tpamd_engine *e, int B, int M, int D, const std::vector<double> &t, const std::vector<double> &q,
                       const std::vector<double> &qd, const std::vector<double> &qdd, const std::vector<int32_t> *count,
                       bool by_index, long long *ok, long long *other) {
  std::vector<double> am((size_t)B * D), stime(B);
  std::vector<int32_t> sidx(B);
  for (int b = 0; b < B; b++) {
    const int n = count ? (*count)[b] : M;
    std::vector<double> row(t.begin() + (size_t)b * M, t.begin() + (size_t)b * M + n);
    stime[b] = (double)StopTimeNs(row, RndInt(0, 4), 0) / 1e9;
    sidx[b] = RndInt(0, 9) == 0 ? RndInt(-1, n) : RndInt(1, std::max(1, n - 1));
    const double scale = RndInt(0, 3) == 0 ? 0.1 : 2.0 + 4.0 * Rnd();
    for (int d = 0; d < D; d++) am[(size_t)b * D + d] = scale;
  }
  const double kSentinel = -777.0;
  std::vector<double> ot((size_t)B * M, kSentinel), oqd((size_t)B * M * D, kSentinel), oqdd((size_t)B * M * D, kSentinel);
  std::vector<int32_t> st(B), keep(B), first(B), last(B);
  tpamd_stop_trajectory_args a{};
  a.num_paths = B; a.stride = M; a.num_dofs = D;
  a.time = t.data(); a.qd = qd.data(); a.qdd = qdd.data(); a.count = count ? count->data() : nullptr;
  a.max_acceleration = am.data(); a.time_step = 1e-3;
  a.stop_time = by_index ? nullptr : stime.data(); a.stop_index = by_index ? sidx.data() : nullptr;
  a.status = st.data(); a.keep = keep.data(); a.first = first.data(); a.last = last.data();
  a.out_time = ot.data(); a.out_qd = oqd.data(); a.out_qdd = oqdd.data();
  CHECK(tpamd_stop_trajectories_host(e, &a) == 0);
  for (int b = 0; b < B; b++) {
    const int n = count ? (*count)[b] : M;
    const size_t o = (size_t)b * M;
    const Rows r{t.data() + o, q.data() + o * D, qd.data() + o * D, qdd.data() + o * D, n, D};
    const MirrorStop m = Mirror(r, by_index, sidx[b], stime[b], &am[(size_t)b * D], 1e-3);
    CHECK(st[b] == m.status);
    const int seg = last[b] - first[b] + 1;
    CHECK(seg >= 0 && (seg == 0 || (first[b] >= 0 && last[b] < n)));
    if (seg < 0) continue;
    CHECK(SameStop(m, r, keep[b], ot.data() + o + first[b], q.data() + (o + first[b]) * D,
                   oqd.data() + (o + first[b]) * D, oqdd.data() + (o + first[b]) * D, seg));
    for (int i = 0; i < M; i++)
      if (i < first[b] || i > last[b]) CHECK(ot[o + i] == kSentinel && oqd[(o + i) * D] == kSentinel);
    (m.status == TPAMD_PLAN_OK ? *ok : *other) += 1;
  }
  // the device entry on the same rows gives the same bytes
  double *d = nullptr;
  const size_t nd = (size_t)B * M * (1 + 2 * D) * 2 + (size_t)B * D + B;
  HIP_OK(hipMalloc(&d, nd * 8 + (size_t)B * 4 * 6));
  double *dt = d, *dqd = dt + (size_t)B * M, *dqdd = dqd + (size_t)B * M * D, *dot = dqdd + (size_t)B * M * D,
         *doqd = dot + (size_t)B * M, *doqdd = doqd + (size_t)B * M * D, *dam = doqdd + (size_t)B * M * D,
         *dst = dam + (size_t)B * D;
  int32_t *di = (int32_t *)(d + nd);
  std::vector<double> sent((size_t)B * M * D, kSentinel);
  HIP_OK(hipMemcpy(dt, t.data(), (size_t)B * M * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dqd, qd.data(), (size_t)B * M * D * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dqdd, qdd.data(), (size_t)B * M * D * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dot, sent.data(), (size_t)B * M * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(doqd, sent.data(), (size_t)B * M * D * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(doqdd, sent.data(), (size_t)B * M * D * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dam, am.data(), (size_t)B * D * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(dst, stime.data(), (size_t)B * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(di + 4 * B, sidx.data(), (size_t)B * 4, hipMemcpyHostToDevice));
  if (count) HIP_OK(hipMemcpy(di + 5 * B, count->data(), (size_t)B * 4, hipMemcpyHostToDevice));
  tpamd_stop_trajectory_args da = a;
  da.time = dt; da.qd = dqd; da.qdd = dqdd; da.count = count ? di + 5 * B : nullptr; da.max_acceleration = dam;
  da.stop_time = by_index ? nullptr : dst; da.stop_index = by_index ? di + 4 * B : nullptr;
  da.status = di; da.keep = di + B; da.first = di + 2 * B; da.last = di + 3 * B;
  da.out_time = dot; da.out_qd = doqd; da.out_qdd = doqdd;
  CHECK(tpamd_stop_trajectories_device(e, &da, nullptr) == 0);
  HIP_OK(hipDeviceSynchronize());
  std::vector<int32_t> gi(4 * B);
  std::vector<double> got((size_t)B * M), gqd((size_t)B * M * D), gqdd((size_t)B * M * D);
  HIP_OK(hipMemcpy(gi.data(), di, (size_t)B * 16, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(got.data(), dot, got.size() * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(gqd.data(), doqd, gqd.size() * 8, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(gqdd.data(), doqdd, gqdd.size() * 8, hipMemcpyDeviceToHost));
  CHECK(std::memcmp(gi.data(), st.data(), B * 4) == 0 && std::memcmp(gi.data() + B, keep.data(), B * 4) == 0 &&
        std::memcmp(gi.data() + 2 * B, first.data(), B * 4) == 0 && std::memcmp(gi.data() + 3 * B, last.data(), B * 4) == 0);
  CHECK(SameBitsOrNaN(got.data(), ot.data(), got.size()) && SameBitsOrNaN(gqd.data(), oqd.data(), gqd.size()) &&
        SameBitsOrNaN(gqdd.data(), oqdd.data(), gqdd.size()));
  HIP_OK(hipFree(d));
}

static void TestBatch() {
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) return;
  long long ok = 0, other = 0;
  int calls = 0;
  for (int D : {3, 7, 14}) {
    g_seed = 11000 + D;
    const int B = 96, N = 300;
    std::vector<std::shared_ptr<TimeableJointSplinePath>> paths;
    for (int b = 0; b < B; b++) paths.push_back(RandomPath(D, N, RndInt(3, 6), 0.3 + 0.4 * (b % 7) / 7.0));
    BatchPathTiming bt;
    CHECK(bt.SetPaths(paths).ok());
    BatchTimingResult r;
    CHECK(bt.ComputeTimingProfiles(0.5, &r).ok());
    if (r.time.size() != (size_t)B * N) continue;
    // solver outputs: uniform rows, then a ragged count
    std::vector<int32_t> ragged(B);
    for (int b = 0; b < B; b++) ragged[b] = b % 9 == 0 ? RndInt(0, 2) : RndInt(3, N);
    for (bool by_index : {false, true}) {
      CheckBatch(e, B, N, D, r.time, r.q, r.qd, r.qdd, nullptr, by_index, &ok, &other);
      CheckBatch(e, B, N, D, r.time, r.q, r.qd, r.qdd, &ragged, by_index, &ok, &other);
      calls += 2;
    }
    // resampled rows (uniform and skip), their counts
    for (int skip = 0; skip < 2; skip++) {
      const int M = 4096;
      std::vector<double> amax((size_t)B * D), start(B, 0.5);
      for (int b = 0; b < B; b++)
        for (int d = 0; d < D; d++) amax[(size_t)b * D + d] = paths[b]->GetMaxJointAcceleration()[d];
      std::vector<double> ot((size_t)B * M), os((size_t)B * M), osd((size_t)B * M), osdd((size_t)B * M),
          oq((size_t)B * M * D), oqd((size_t)B * M * D), oqdd((size_t)B * M * D);
      std::vector<int32_t> cnt(B);
      tpamd_resample_args ra{};
      ra.num_paths = B; ra.num_samples = N; ra.num_dofs = D; ra.max_out = M;
      ra.time = r.time.data(); ra.s = r.s.data(); ra.sd = r.sd.data(); ra.sdd = r.sdd.data();
      ra.q = r.q.data(); ra.qd = r.qd.data(); ra.qdd = r.qdd.data();
      ra.max_acceleration = amax.data(); ra.start_sec = start.data(); ra.time_step = skip ? 4e-3 : 1e-3;
      ra.status = r.status.data();
      ra.out_time = ot.data(); ra.out_s = os.data(); ra.out_sd = osd.data(); ra.out_sdd = osdd.data();
      ra.out_q = oq.data(); ra.out_qd = oqd.data(); ra.out_qdd = oqdd.data(); ra.count = cnt.data();
      CHECK((skip ? tpamd_resample_skip_host(e, &ra) : tpamd_resample_uniform_host(e, &ra)) == 0);
      for (int b = 0; b < B; b++) cnt[b] = std::min(std::max(cnt[b], 0), M);
      for (bool by_index : {false, true}) {
        CheckBatch(e, B, M, D, ot, oq, oqd, oqdd, &cnt, by_index, &ok, &other);
        calls++;
      }
    }
  }
  // call-level errors
  {
    tpamd_stop_trajectory_args a{};
    double x = 0;
    int32_t i = 0;
    a.num_paths = 1; a.stride = 1; a.num_dofs = 3;
    a.time = a.qd = a.qdd = a.max_acceleration = a.stop_time = &x;
    a.status = a.keep = a.first = a.last = &i;
    a.out_time = a.out_qd = a.out_qdd = &x;
    tpamd_stop_trajectory_args b = a;
    b.num_dofs = 17;
    CHECK(tpamd_stop_trajectories_host(e, &b) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.num_dofs = 0;
    CHECK(tpamd_stop_trajectories_host(e, &b) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.stride = 0;
    CHECK(tpamd_stop_trajectories_device(e, &b, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.stop_time = nullptr;
    CHECK(tpamd_stop_trajectories_host(e, &b) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.out_qdd = nullptr;
    CHECK(tpamd_stop_trajectories_device(e, &b, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.num_paths = -1;
    CHECK(tpamd_stop_trajectories_host(e, &b) == TPAMD_E_INVALID_ARGUMENT);
    b = a; b.num_paths = 0;
    CHECK(tpamd_stop_trajectories_host(e, &b) == 0);
    CHECK(tpamd_stop_trajectories_host(nullptr, &a) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_stop_trajectories_device(e, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  }
  tpamd_engine_destroy(e);
  CHECK(ok > 500 && other > 200);
  std::printf("batch stop vs mirror: %d calls, ok %lld, other statuses %lld\n", calls, ok, other);
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) {
      TestSetAgainstMirror(m, D);
      TestSetCabi(m, D);
    }
  TestBatch();
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("%d CHECKS FAILED\n", g_fail);
  return g_fail == 0 ? 0 : 1;
}

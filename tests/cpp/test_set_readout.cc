// GPU test of the planner-set readouts (run by tests/test_gpu_set_readout.py):
//   PathTimingTrajectorySet::GetTrajectories (tpamd_planner_set_download_trajectories) against
//   GetTrajectory of every planner, byte for byte, for all planners, a subset and a list with
//   repeats;
//   PathTimingTrajectorySet::GetSetpoints (tpamd_planner_set_sample_at_ticks) against one mirror
//   planner per set member (TrajectoryPlanner::Get{Position,Velocity,Acceleration}AtTime), values
//   and statuses, on tick grids that start before, inside, on a sample of and near the end of each
//   trajectory; a few planners also against the oracle's planner interpolated by the same formula.
// 260-planner sets at D = 3 and 7, both sampling methods, paths of different sizes, planners that
// never get a path, several Plan rounds with a switch and a reset in between. A twin set that never
// reads out must give the same Plan results, summaries and PCIe bytes.
// Then the C-ABI: both _device variants on a non-blocking stream with a Plan enqueued right after
// them equal the host variants; sentinels show that non-OK ticks and too-small capacities leave the
// arrays untouched; bad ids, overflowing tick times and every call-level error.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
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
    w.push_back(v);
  }
  return w;
}

static std::shared_ptr<TimeableJointSplinePath> RandomPath(int D, int N, int W, double fraction) {
  std::vector<VectorXd> wps = RandomWaypoints(W, D);
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

// TrajectoryPlanner's getters on a downloaded trajectory (the reference for planners whose mirror
// parted ways with the set, see test_set_switch.cc)
struct BufferProbe : TrajectoryPlanner {
  Status Plan(Time, tpamd::compat::Duration) override { return Status(); }
  Status SetPath(std::shared_ptr<TimeablePath>) override { return Status(); }
  void ResetDerived() override {}
  void Fill(const PlannedTrajectory &t, int D) {
    const size_t n = t.time.size();
    time_ = t.time;
    positions_.assign(n, VectorXd(D)); velocities_.assign(n, VectorXd(D)); accelerations_.assign(n, VectorXd(D));
    for (size_t i = 0; i < n; i++)
      for (int d = 0; d < D; d++) {
        positions_[i][d] = t.positions[i * D + d];
        velocities_[i][d] = t.velocities[i * D + d];
        accelerations_[i][d] = t.accelerations[i * D + d];
      }
  }
};

static bool SameTrajectory(const PlannedTrajectory &a, const PlannedTrajectory &b) {
  return SameBits(a.time, b.time) && SameBits(a.path_parameter, b.path_parameter) &&
         SameBits(a.path_parameter_derivative, b.path_parameter_derivative) &&
         SameBits(a.second_path_parameter_derivative, b.second_path_parameter_derivative) &&
         SameBits(a.positions, b.positions) && SameBits(a.velocities, b.velocities) &&
         SameBits(a.accelerations, b.accelerations);
}

// The oracle planner's samples at a time, by the host formula (upper_bound bracket, lerp)
static int OracleAt(const tpo_planner *o, int D, int64_t ns, std::vector<double> out[3]) {
  const int M = tpo_planner_num_samples(o);
  const double *t = tpo_planner_time(o);
  if (M == 0) return TPAMD_PLAN_FAILED_PRECONDITION;
  const double ts = (double)ns / 1e9;
  if (ts < t[0] || ts > t[M - 1]) return TPAMD_PLAN_OUT_OF_RANGE;
  const int u = (int)(std::upper_bound(t, t + M, ts) - t);
  const double *src[3] = {tpo_planner_positions(o), tpo_planner_velocities(o), tpo_planner_accelerations(o)};
  for (int a = 0; a < 3; a++) {
    out[a].assign(D, 0.0);
    for (int d = 0; d < D; d++) {
      if (u == M) { out[a][d] = src[a][(size_t)(M - 1) * D + d]; continue; }
      const int l = u - 1;
      const double f = (ts - t[l]) / (t[u] - t[l]);
      const double x = src[a][(size_t)l * D + d], y = src[a][(size_t)u * D + d];
      out[a][d] = x + f * (y - x);
    }
  }
  return TPAMD_PLAN_OK;
}

static int Code(const tpamd::compat::Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return TPAMD_PLAN_OK;
    case StatusCode::kFailedPrecondition: return TPAMD_PLAN_FAILED_PRECONDITION;
    case StatusCode::kOutOfRange: return TPAMD_PLAN_OUT_OF_RANGE;
    case StatusCode::kInvalidArgument: return TPAMD_PLAN_INVALID_ARGUMENT;
    default: return TPAMD_PLAN_INTERNAL;
  }
}

static void TestReadoutAgainstMirrors(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, P0 = 7, with_path = 250;     // planners 250.. never get a path
  g_seed = 3000 + D * 7 + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  const int64_t step_ts = opt.GetTimeStep().nanos();
  PathTimingTrajectorySet set(opt, B, P0), twin(opt, B, P0);
  CHECK(set.status().ok() && twin.status().ok());
  if (!set.status().ok() || !twin.status().ok()) return;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(with_path);
  for (int b = 0; b < with_path; b++) paths[b] = RandomPath(D, N, RndInt(3, 7), 0.3 + 0.4 * (b % 7) / 7.0);
  CHECK(set.SetPaths(paths).ok() && twin.SetPaths(paths).ok());
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) {
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    if (b < with_path) CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  const int kOracle[3] = {0, 101, 200};     // never switched or reset
  auto is_oracle = [&](int b) { return b == kOracle[0] || b == kOracle[1] || b == kOracle[2]; };
  std::vector<tpo_planner *> oracle;
  for (int b : kOracle) {
    tpo_planner *o = tpo_planner_create(D, N, paths[b]->GetPathSamplingDistance(), paths[b]->options().constraint_safety(),
                                        step_ts, skip ? 1 : 0, opt.GetMaxPlanningIterations(),
                                        opt.GetMaxInitialVelocityError());
    tpo_planner_set_limits(o, paths[b]->GetMaxJointVelocity().data(), paths[b]->GetMaxJointAcceleration().data());
    tpo_planner_set_spline(o, paths[b]->knots().data(), (int)paths[b]->knots().size(),
                           paths[b]->packed_control_points().data(), paths[b]->num_control_points(), TPO_PATH_NEW);
    oracle.push_back(o);
  }
  std::vector<bool> diverged(B, false), was_reset(B, false);
  std::vector<int> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  const std::vector<size_t> all_ids(all.begin(), all.end());
  const int T = 40;
  long long cat_ok = 0, cat_on_sample = 0, cat_oor = 0, cat_fp = 0, cat_oracle = 0, cat_last = 0;
  int plans = 0, switched = 0, reported = 0;
  int64_t start = 2000 * kMs;
  for (int round = 0; round < 8; round++) {
    const bool to_end = round >= 6;
    const int64_t horizon = to_end ? (int64_t)100000 * kMs : 500 * kMs;
    const auto st = set.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    const auto tw = twin.Plan(FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    std::vector<PathTimingTrajectory *> batch;
    for (int b = 0; b < B; b++) batch.push_back(mirrors[b].get());
    const auto ms = PathTimingTrajectory::PlanBatch(batch, FromUnixNanos(start), tpamd::compat::Nanoseconds(horizon));
    plans++;
    // the set that reads out plans as the twin that never does
    CHECK(set.LastPlanBytesOverPcie() == twin.LastPlanBytesOverPcie());
    for (int b = 0; b < B; b++) {
      CHECK(st[b].code() == tw[b].code());
      CHECK(set.GetNumTimeSamples(b) == twin.GetNumTimeSamples(b));
      CHECK(ToUnixNanos(set.GetEndTime(b)) == ToUnixNanos(twin.GetEndTime(b)));
      CHECK(ToUnixNanos(set.GetStartTime(b)) == ToUnixNanos(twin.GetStartTime(b)));
      CHECK(ToUnixNanos(set.GetFinalDecelStart(b)) == ToUnixNanos(twin.GetFinalDecelStart(b)));
      CHECK(set.IsTrajectoryAtEnd(b) == twin.IsTrajectoryAtEnd(b) && set.WindowsOfLastPlan(b) == twin.WindowsOfLastPlan(b));
    }
    for (size_t i = 0; i < oracle.size(); i++) {
      const int rc = tpo_planner_plan(oracle[i], start, horizon);
      CHECK((rc == TPO_PLAN_OK) == ms[kOracle[i]].ok());
    }
    // the per-planner route: GetTrajectory of every planner
    std::vector<PlannedTrajectory> ref(B);
    for (int b = 0; b < B; b++) {
      CHECK(set.GetTrajectory(b, &ref[b]).ok());
      if (diverged[b]) continue;
      CHECK(st[b].code() == ms[b].code());
      const PathTimingTrajectory &m = *mirrors[b];
      const bool same = SameBits(ref[b].time, m.GetTime()) && SameBits(ref[b].positions, Flatten(m.GetPositions())) &&
                        SameBits(ref[b].velocities, Flatten(m.GetVelocities())) &&
                        SameBits(ref[b].accelerations, Flatten(m.GetAccelerations()));
      CHECK(same);
      // a failed first window of a new or modified path: the set keeps the path sampled and the
      // mirror does not; such planners are compared with their own download from then on
      if (ms[b].code() == StatusCode::kInvalidArgument || !same) diverged[b] = true;
    }
    // the packed download: all, a subset, a list with repeats
    {
      std::vector<PlannedTrajectory> got;
      CHECK(set.GetTrajectories(all_ids, &got).ok() && got.size() == (size_t)B);
      for (int b = 0; b < B && got.size() == (size_t)B; b++) CHECK(SameTrajectory(got[b], ref[b]));
      std::vector<size_t> sub;
      for (int b = B - 1; b >= 0; b -= 3) sub.push_back(b);
      CHECK(set.GetTrajectories(sub, &got).ok() && got.size() == sub.size());
      for (size_t k = 0; k < sub.size() && got.size() == sub.size(); k++) CHECK(SameTrajectory(got[k], ref[sub[k]]));
      const std::vector<size_t> rep = {5, 5, 17, 259, 5, 0, 101, 17};
      CHECK(set.GetTrajectories(rep, &got).ok() && got.size() == rep.size());
      for (size_t k = 0; k < rep.size() && got.size() == rep.size(); k++) CHECK(SameTrajectory(got[k], ref[rep[k]]));
      CHECK(set.GetTrajectories({}, &got).ok() && got.empty());
    }
    // setpoints: grids before, on a sample of, inside and near the end of each trajectory
    std::vector<Time> starts(B);
    std::vector<int64_t> start_ns(B);
    for (int b = 0; b < B; b++) {
      const auto &t = ref[b].time;
      int64_t s0 = start;
      if (!t.empty()) {
        const int64_t first = (int64_t)llround(t.front() * 1e9), last = (int64_t)llround(t.back() * 1e9);
        switch ((b + round) % 4) {
          case 0: s0 = first - 7 * step_ts; break;
          case 1: s0 = (int64_t)llround(t[RndInt(0, (int)t.size() - 1)] * 1e9); break;
          case 2: s0 = first + (int64_t)(Rnd() * (double)(last - first)); break;
          default: s0 = last - 20 * step_ts; break;
        }
      }
      start_ns[b] = s0;
      starts[b] = FromUnixNanos(s0);
    }
    for (int pass = 0; pass < 2; pass++) {
      const auto step = tpamd::compat::Nanoseconds(pass == 0 ? step_ts : 3 * kMs + 1);
      TrajectorySetpoints sp;
      CHECK(set.GetSetpoints(all_ids, starts, step, T, &sp).ok());
      CHECK(sp.num_planners == (size_t)B && sp.num_ticks == (size_t)T && sp.num_dofs == (size_t)D);
      if (sp.status.size() != (size_t)B * T) continue;
      for (int b = 0; b < B; b++) {
        BufferProbe probe;
        probe.Fill(ref[b], D);
        const TrajectoryPlanner &R = diverged[b] ? (const TrajectoryPlanner &)probe : *mirrors[b];
        for (int j = 0; j < T; j++) {
          const int64_t ns = start_ns[b] + j * step.nanos();
          const auto wq = R.GetPositionAtTime(FromUnixNanos(ns)), wqd = R.GetVelocityAtTime(FromUnixNanos(ns)),
                     wqdd = R.GetAccelerationAtTime(FromUnixNanos(ns));
          const size_t i = (size_t)b * T + j;
          const int got = Code(sp.status[i]);
          CHECK(got == Code(wq.status()) && got == Code(wqd.status()) && got == Code(wqdd.status()));
          if (got == TPAMD_PLAN_OK && wq.ok() && wqd.ok() && wqdd.ok()) {
            const bool same = SameBits(sp.positions.data() + i * D, (*wq).data(), D) &&
                              SameBits(sp.velocities.data() + i * D, (*wqd).data(), D) &&
                              SameBits(sp.accelerations.data() + i * D, (*wqdd).data(), D);
            CHECK(same);
            if (!same && ++reported <= 8) std::printf("  planner %d tick %d differs\n", b, j);
            cat_ok++;
            const auto &t = ref[b].time;
            const double ts = (double)ns / 1e9;
            if (std::binary_search(t.begin(), t.end(), ts)) cat_on_sample++;
            if (!t.empty() && ts == t.back()) cat_last++;
          } else {
            CHECK(std::isnan(sp.positions[i * D]) && std::isnan(sp.accelerations[i * D + D - 1]));
            cat_oor += got == TPAMD_PLAN_OUT_OF_RANGE;
            cat_fp += got == TPAMD_PLAN_FAILED_PRECONDITION;
          }
          if ((b >= with_path || was_reset[b]) && round > 0) CHECK(got == TPAMD_PLAN_FAILED_PRECONDITION);
        }
      }
      // the oracle planners by the same host formula
      for (size_t o = 0; o < oracle.size(); o++) {
        const int b = kOracle[o];
        if (diverged[b]) continue;
        for (int j = 0; j < T; j++) {
          std::vector<double> w[3];
          const int rc = OracleAt(oracle[o], D, start_ns[b] + j * step.nanos(), w);
          const size_t i = (size_t)b * T + j;
          CHECK(rc == Code(sp.status[i]));
          if (rc == TPAMD_PLAN_OK) {
            CHECK(SameBits(sp.positions.data() + i * D, w[0].data(), D) &&
                  SameBits(sp.velocities.data() + i * D, w[1].data(), D) &&
                  SameBits(sp.accelerations.data() + i * D, w[2].data(), D));
            cat_oracle++;
          }
        }
      }
      // a list with repeats gives the rows of the full call
      const std::vector<size_t> rep = {17, 3, 17, 255, 0};
      std::vector<Time> rs;
      for (size_t b : rep) rs.push_back(starts[b]);
      TrajectorySetpoints sr;
      CHECK(set.GetSetpoints(rep, rs, step, T, &sr).ok());
      for (size_t k = 0; k < rep.size() && sr.status.size() == rep.size() * T; k++)
        for (int j = 0; j < T; j++) {
          const size_t a = k * T + j, f = rep[k] * T + j;
          CHECK(sr.status[a].code() == sp.status[f].code());
          if (sp.status[f].ok())
            CHECK(SameBits(sr.positions.data() + a * D, sp.positions.data() + f * D, D) &&
                  SameBits(sr.accelerations.data() + a * D, sp.accelerations.data() + f * D, D));
        }
    }
    const int64_t next = start + 150 * kMs;
    if (round == 2) {      // a seeded subset switches to new waypoints (set and twin alike)
      std::vector<size_t> ids;
      std::vector<Time> times;
      std::vector<std::vector<VectorXd>> wps;
      for (int b = 0; b < with_path; b++) {
        if (is_oracle(b) || Rnd() > 0.3) continue;
        ids.push_back(b);
        times.push_back(FromUnixNanos(next));
        wps.push_back(RandomWaypoints(RndInt(1, 5), D));
      }
      const auto got = set.SwitchToWaypointPaths(ids, times, wps);
      const auto got_twin = twin.SwitchToWaypointPaths(ids, times, wps);
      for (size_t k = 0; k < ids.size(); k++) {
        const int b = (int)ids[k];
        CHECK(got[k].code() == got_twin[k].code());
        if (diverged[b]) continue;
        PathTimingTrajectory &m = *mirrors[b];
        auto stop = m.GetPathStopParameter(times[k]);
        StatusCode want = StatusCode::kOk;
        if (!stop.ok()) {
          want = stop.status().code();
        } else {
          const auto v = m.GetVelocityAtTime(times[k]);
          if (!v.ok()) want = v.status().code();
          else {
            const auto e = paths[b]->SwitchToWaypointPath(*stop, {wps[k].data(), wps[k].size()});
            if (!e.ok()) { want = e.code(); diverged[b] = true; }
            else CHECK(paths[b]->SetInitialVelocity({(*v).data(), (*v).size()}).ok());
          }
        }
        CHECK(got[k].code() == want);
        switched += want == StatusCode::kOk;
      }
    }
    if (round == 3) {      // a few planners are reset: no path, no samples from now on
      for (int b = 10; b < with_path; b += 37) {
        if (is_oracle(b)) continue;
        set.Reset(b);
        twin.Reset(b);
        mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);     // Reset: no path, no plan
        was_reset[b] = true;
        diverged[b] = true;      // compared through its (empty) download from now on
      }
    }
    start = to_end ? start + 3000 * kMs : next;
  }
  // the twin's trajectories, read once at the end, are the set's
  for (int b = 0; b < B; b++) {
    PlannedTrajectory a, c;
    CHECK(set.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok() && SameTrajectory(a, c));
  }
  int div = 0;
  for (int b = 0; b < B; b++) div += diverged[b];
  CHECK(cat_ok > 1000 && cat_on_sample > 100 && cat_oor > 100 && cat_fp > 100 && cat_oracle > 50);
  CHECK(switched > 20 && div < B / 2);
  for (auto *o : oracle) tpo_planner_destroy(o);
  std::printf("readout vs mirrors (D %d, %s): %d plans, ticks ok %lld (on a sample %lld, on the last %lld), out of range "
              "%lld, no samples %lld, oracle ticks %lld, %d switched, %d compared through their download\n",
              D, skip ? "skip" : "uniform", plans, cat_ok, cat_on_sample, cat_last, cat_oor, cat_fp, cat_oracle, switched,
              div);
}

// ------------------------------------------------------------------ the C-ABI
struct RawSets {
  tpamd_engine *e = nullptr;
  tpamd_planner_set *ps = nullptr, *twin = nullptr;
};

static void TestCabi(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 260, N = 300, with_path = 250, T = 30;
  g_seed = 5000 + D + (skip ? 1 : 0);
  const int64_t step_ts = skip ? 4 * kMs : kMs;
  RawSets r;
  CHECK(tpamd_engine_create(0, &r.e) == 0);
  if (!r.e) return;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 7;
  cfg.sampling_method = skip ? 1 : 0;
  cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8; cfg.max_initial_velocity_error = 1e-2;
  cfg.time_step_ns = step_ts;
  CHECK(tpamd_planner_set_create(r.e, &cfg, &r.ps) == 0 && tpamd_planner_set_create(r.e, &cfg, &r.twin) == 0);
  if (!r.ps || !r.twin) return;
  {
    std::vector<int32_t> np(with_path), state(with_path, 1);
    std::vector<double> knots, cps, vmax, amax, delta, iv(with_path * D, 0.0);
    for (int b = 0; b < with_path; b++) {
      auto p = RandomPath(D, N, RndInt(3, 7), 0.3 + 0.4 * (b % 7) / 7.0);
      np[b] = p->num_control_points();
      knots.insert(knots.end(), p->knots().begin(), p->knots().end());
      cps.insert(cps.end(), p->packed_control_points().begin(), p->packed_control_points().end());
      vmax.insert(vmax.end(), p->GetMaxJointVelocity().begin(), p->GetMaxJointVelocity().end());
      amax.insert(amax.end(), p->GetMaxJointAcceleration().begin(), p->GetMaxJointAcceleration().end());
      delta.push_back(p->GetPathSamplingDistance());
    }
    for (tpamd_planner_set *s : {r.ps, r.twin})
      CHECK(tpamd_planner_set_upload_paths_ragged(s, with_path, nullptr, np.data(), knots.data(), cps.data(), vmax.data(),
                                                  amax.data(), delta.data(), iv.data(), state.data()) == 0);
  }
  std::vector<tpamd_planner_summary> sum(B), sum_twin(B);
  int64_t start = 1000 * kMs;
  auto plan_both = [&](int64_t s0, int64_t h) {
    std::vector<int64_t> s(B, s0), hz(B, h);
    CHECK(tpamd_planner_set_plan(r.ps, s.data(), hz.data(), sum.data()) == 0);
    CHECK(tpamd_planner_set_plan(r.twin, s.data(), hz.data(), sum_twin.data()) == 0);
    CHECK(std::memcmp(sum.data(), sum_twin.data(), B * sizeof(tpamd_planner_summary)) == 0);
    size_t a[2], c[2];
    tpamd_planner_set_last_plan_bytes(r.ps, &a[0], &a[1]);
    tpamd_planner_set_last_plan_bytes(r.twin, &c[0], &c[1]);
    CHECK(a[0] == c[0] && a[1] == c[1]);
  };
  plan_both(start, 500 * kMs);
  const int32_t reset_id = 7;
  CHECK(tpamd_planner_set_reset(r.ps, 1, &reset_id) == 0 && tpamd_planner_set_reset(r.twin, 1, &reset_id) == 0);
  sum[reset_id] = sum_twin[reset_id] = tpamd_planner_summary{};     // no samples after the reset
  const double kSentinel = -12345.0;
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  int rounds = 0;
  for (int round = 0; round < 3; round++, rounds++) {
    // listed planners: all, then a list with repeats and (device only) bad ids
    std::vector<int32_t> ids;
    for (int b = 0; b < B; b++) ids.push_back((b * 37 + round) % B);
    ids.push_back(3); ids.push_back(3); ids.push_back(259); ids.push_back(reset_id);
    const int n = (int)ids.size();
    std::vector<int64_t> st0(n);
    for (int k = 0; k < n; k++) {
      const tpamd_planner_summary &s = sum[ids[k]];
      st0[k] = (k % 3 == 0) ? s.start_time_ns - 5 * step_ts : (k % 3 == 1) ? s.start_time_ns : s.end_time_ns - 10 * step_ts;
    }
    // host variants
    const size_t ticks = (size_t)n * T;
    std::vector<double> hq(ticks * D, kSentinel), hqd(ticks * D, kSentinel), hqdd(ticks * D, kSentinel);
    std::vector<int32_t> hst(ticks, -9);
    const size_t bytes_before = tpamd_planner_set_device_bytes(r.ps);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, n, ids.data(), st0.data(), step_ts, T, hq.data(), hqd.data(),
                                            hqdd.data(), hst.data()) == 0);
    CHECK(tpamd_planner_set_device_bytes(r.ps) > bytes_before || round > 0);   // the staging is the set's
    int ok = 0, oor = 0, fp = 0;
    for (size_t i = 0; i < ticks; i++) {
      ok += hst[i] == TPAMD_PLAN_OK;
      oor += hst[i] == TPAMD_PLAN_OUT_OF_RANGE;
      fp += hst[i] == TPAMD_PLAN_FAILED_PRECONDITION;
      if (hst[i] != TPAMD_PLAN_OK) CHECK(hq[i * D] == kSentinel && hqd[i * D + D - 1] == kSentinel && hqdd[i * D] == kSentinel);
    }
    CHECK(ok > 0 && oor > 0 && fp >= T);
    for (int j = 0; j < T; j++) CHECK(hst[(size_t)(n - 1) * T + j] == TPAMD_PLAN_FAILED_PRECONDITION);   // reset
    int64_t total = 0;
    for (int k = 0; k < n; k++) total += sum[ids[k]].num_samples;
    std::vector<int64_t> hoff(n + 1, -1);
    std::vector<double> ht(total), hs(total), hsd(total), hsdd(total), hpq(total * D), hpqd(total * D), hpqdd(total * D);
    CHECK(tpamd_planner_set_download_trajectories(r.ps, n, ids.data(), hoff.data(), total, ht.data(), hs.data(),
                                                  hsd.data(), hsdd.data(), hpq.data(), hpqd.data(), hpqdd.data()) == 0);
    CHECK(hoff[0] == 0 && hoff[n] == total);
    for (int k = 0; k < n; k++) {      // each range equals the single-planner download
      const int c = (int)(hoff[k + 1] - hoff[k]);
      CHECK(c == sum[ids[k]].num_samples);
      if (c <= 0) continue;
      std::vector<double> t1(c), q1(c * D), a1(c * D);
      CHECK(tpamd_planner_set_download_trajectory(r.ps, ids[k], 0, c, t1.data(), nullptr, nullptr, nullptr, q1.data(),
                                                  nullptr, a1.data()) == 0);
      CHECK(SameBits(t1.data(), ht.data() + hoff[k], c) && SameBits(q1.data(), hpq.data() + hoff[k] * D, c * D) &&
            SameBits(a1.data(), hpqdd.data() + hoff[k] * D, c * D));
    }
    // device variants on a non-blocking stream; bad ids appended; a Plan enqueued right after
    std::vector<int32_t> dids = ids;
    dids.push_back(-1); dids.push_back(B);
    std::vector<int64_t> dst0 = st0;
    dst0.push_back(start); dst0.push_back(start);
    const int dn = n + 2;
    const size_t dticks = (size_t)dn * T;
    int32_t *d_ids = nullptr, *d_st = nullptr;
    int64_t *d_start = nullptr, *d_off = nullptr, *d_off2 = nullptr;
    double *d_q = nullptr, *d_qd = nullptr, *d_qdd = nullptr, *d_rows = nullptr, *d_rows2 = nullptr;
    HIP_OK(hipMalloc(&d_ids, dn * 4)); HIP_OK(hipMalloc(&d_start, dn * 8)); HIP_OK(hipMalloc(&d_st, dticks * 4));
    HIP_OK(hipMalloc(&d_q, dticks * D * 8)); HIP_OK(hipMalloc(&d_qd, dticks * D * 8)); HIP_OK(hipMalloc(&d_qdd, dticks * D * 8));
    HIP_OK(hipMalloc(&d_off, (dn + 1) * 8)); HIP_OK(hipMalloc(&d_off2, (dn + 1) * 8));
    HIP_OK(hipMalloc(&d_rows, (size_t)total * (4 + 3 * D) * 8)); HIP_OK(hipMalloc(&d_rows2, (size_t)total * 8));
    std::vector<double> sent(std::max(dticks * D, (size_t)total * (4 + 3 * D)), kSentinel);
    HIP_OK(hipMemcpy(d_ids, dids.data(), dn * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_start, dst0.data(), dn * 8, hipMemcpyHostToDevice));
    for (double *p : {d_q, d_qd, d_qdd}) HIP_OK(hipMemcpy(p, sent.data(), dticks * D * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rows, sent.data(), (size_t)total * (4 + 3 * D) * 8, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(d_rows2, sent.data(), (size_t)total * 8, hipMemcpyHostToDevice));
    double *rt = d_rows, *rs = rt + total, *rsd = rs + total, *rsdd = rsd + total, *rq = rsdd + total,
           *rqd = rq + total * D, *rqdd = rqd + total * D;
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, dn, d_ids, d_start, step_ts, T, d_q, d_qd, d_qdd, d_st,
                                                   stream) == 0);
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, dn, d_ids, d_off, total, rt, rs, rsd, rsdd, rq, rqd, rqdd,
                                                         stream) == 0);
    // a too-small capacity: offsets written, no row
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, dn, d_ids, d_off2, total - 1, d_rows2, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, nullptr, stream) == 0);
    start += 150 * kMs;
    plan_both(start, 500 * kMs);          // must not overwrite what the readouts are still reading
    HIP_OK(hipStreamSynchronize(stream));
    std::vector<double> gq(dticks * D), gqd(dticks * D), gqdd(dticks * D), grows((size_t)total * (4 + 3 * D)), grows2(total);
    std::vector<int32_t> gst(dticks);
    std::vector<int64_t> goff(dn + 1), goff2(dn + 1);
    HIP_OK(hipMemcpy(gq.data(), d_q, dticks * D * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gqd.data(), d_qd, dticks * D * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gqdd.data(), d_qdd, dticks * D * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(gst.data(), d_st, dticks * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(goff.data(), d_off, (dn + 1) * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(goff2.data(), d_off2, (dn + 1) * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(grows.data(), d_rows, grows.size() * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(grows2.data(), d_rows2, grows2.size() * 8, hipMemcpyDeviceToHost));
    CHECK(std::memcmp(gst.data(), hst.data(), ticks * 4) == 0);
    CHECK(SameBits(gq.data(), hq.data(), ticks * D) && SameBits(gqd.data(), hqd.data(), ticks * D) &&
          SameBits(gqdd.data(), hqdd.data(), ticks * D));
    for (size_t i = ticks; i < dticks; i++) CHECK(gst[i] == TPAMD_PLAN_INVALID_ARGUMENT && gq[i * D] == kSentinel);
    CHECK(std::memcmp(goff.data(), hoff.data(), (n + 1) * 8) == 0 && goff[n + 1] == total && goff[n + 2] == total);
    CHECK(std::memcmp(goff2.data(), goff.data(), (dn + 1) * 8) == 0);
    CHECK(SameBits(grows.data(), ht.data(), total) && SameBits(grows.data() + total, hs.data(), total) &&
          SameBits(grows.data() + 2 * total, hsd.data(), total) && SameBits(grows.data() + 3 * total, hsdd.data(), total) &&
          SameBits(grows.data() + 4 * total, hpq.data(), total * D) &&
          SameBits(grows.data() + 4 * total + total * D, hpqd.data(), total * D) &&
          SameBits(grows.data() + 4 * total + 2 * total * D, hpqdd.data(), total * D));
    bool untouched = true;
    for (double v : grows2) untouched &= v == kSentinel;
    CHECK(untouched);
    for (void *p : {(void *)d_ids, (void *)d_start, (void *)d_st, (void *)d_q, (void *)d_qd, (void *)d_qdd, (void *)d_off,
                    (void *)d_off2, (void *)d_rows, (void *)d_rows2})
      HIP_OK(hipFree(p));
  }
  // ids NULL on the device, count = B; count = 0 writes offsets[0] = 0
  {
    int64_t *d_off = nullptr;
    HIP_OK(hipMalloc(&d_off, (B + 1) * 8));
    std::vector<int64_t> hoff(B + 1), goff(B + 1, -1);
    const int rc = tpamd_planner_set_download_trajectories(r.ps, B, nullptr, hoff.data(), 0, nullptr, nullptr, nullptr,
                                                           nullptr, nullptr, nullptr, nullptr);
    CHECK(rc == TPAMD_E_INVALID_ARGUMENT && hoff[0] == 0 && hoff[B] > 0);
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, B, nullptr, d_off, 0, nullptr, nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, stream) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(goff.data(), d_off, (B + 1) * 8, hipMemcpyDeviceToHost));
    CHECK(goff == hoff);
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, 0, nullptr, d_off, 0, nullptr, nullptr, nullptr, nullptr,
                                                         nullptr, nullptr, nullptr, stream) == 0);
    HIP_OK(hipStreamSynchronize(stream));
    HIP_OK(hipMemcpy(goff.data(), d_off, 8, hipMemcpyDeviceToHost));
    CHECK(goff[0] == 0);
    HIP_OK(hipFree(d_off));
  }
  // call-level errors change nothing
  {
    const int32_t good[2] = {0, 1}, bad[2] = {0, B};
    const int64_t s2[2] = {start, start};
    double q[2 * 5 * 16], t[4];
    int32_t st[10];
    int64_t off[3] = {-1, -1, -1};
    for (int i = 0; i < 10; i++) st[i] = -9;
    for (double &v : q) v = kSentinel;
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, bad, s2, step_ts, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, good, s2, 0, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, good, s2, -4, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, good, s2, step_ts, 0, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, good, s2, step_ts, 5, q, q, q, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 2, good, nullptr, step_ts, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, -1, good, s2, step_ts, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, B + 1, nullptr, s2, step_ts, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks(nullptr, 2, good, s2, step_ts, 5, q, q, q, st) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, 2, good, s2, 0, 5, q, q, q, st, stream) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, 2, good, s2, step_ts, 0, q, q, q, st, stream) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, 2, good, s2, step_ts, 5, q, q, q, nullptr, stream) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, 2, good, nullptr, step_ts, 5, q, q, q, st, stream) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_sample_at_ticks_device(r.ps, B + 1, nullptr, s2, step_ts, 5, q, q, q, st, stream) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories(r.ps, 2, bad, off, 100, t, t, t, t, q, q, q) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories(r.ps, 2, good, nullptr, 100, t, t, t, t, q, q, q) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories(r.ps, B + 1, nullptr, off, 100, t, t, t, t, q, q, q) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories(nullptr, 2, good, off, 100, t, t, t, t, q, q, q) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, 2, good, nullptr, 100, t, t, t, t, q, q, q, stream) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_trajectories_device(r.ps, -1, good, off, 100, t, t, t, t, q, q, q, stream) ==
          TPAMD_E_INVALID_ARGUMENT);
    bool untouched = off[0] == -1 && off[2] == -1;
    for (int i = 0; i < 10; i++) untouched &= st[i] == -9;
    for (double v : q) untouched &= v == kSentinel;
    CHECK(untouched);
    // a too-small capacity on the host: offsets written, no row, INVALID_ARGUMENT
    const int32_t one = 1;
    int64_t off1[2] = {-1, -1};
    t[0] = kSentinel;
    CHECK(tpamd_planner_set_download_trajectories(r.ps, 1, &one, off1, 1, t, nullptr, nullptr, nullptr, nullptr, nullptr,
                                                  nullptr) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(off1[0] == 0 && off1[1] == sum[1].num_samples && off1[1] > 1 && t[0] == kSentinel);
    // tick times that overflow int64: OUT_OF_RANGE, values untouched
    const int64_t late[1] = {LLONG_MAX - 3 * step_ts};
    CHECK(tpamd_planner_set_sample_at_ticks(r.ps, 1, &one, late, step_ts, 5, q, nullptr, nullptr, st) == 0);
    for (int j = 0; j < 5; j++) CHECK(st[j] == TPAMD_PLAN_OUT_OF_RANGE);
    CHECK(q[0] == kSentinel);
  }
  HIP_OK(hipStreamDestroy(stream));
  tpamd_planner_set_destroy(r.ps);
  tpamd_planner_set_destroy(r.twin);
  tpamd_engine_destroy(r.e);
  std::printf("readout C-ABI (D %d, %s): %d rounds of device readouts with a Plan right after, errors ok\n", D,
              skip ? "skip" : "uniform", rounds);
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) {
      TestReadoutAgainstMirrors(m, D);
      TestCabi(m, D);
    }
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("%d CHECKS FAILED\n", g_fail);
  return g_fail == 0 ? 0 : 1;
}

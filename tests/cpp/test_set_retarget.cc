// GPU test of the planner-set retarget (run by tests/test_gpu_set_retarget.py):
// PathTimingTrajectorySet::RetargetWaypointPaths / tpamd_planner_set_retarget(_device) redirect
// moving planners onto new waypoints on the device. For 70-planner sets at D = 3 and 7 with both
// sampling methods (N = 100, delta 0.005, horizon 0.4 s, vmax in [1, 2], amax in [2, 5], waypoints
// in [-1.5, 1.5], 2-4 per path):
//   1. one call with shuffled ids over a subset of the planners, retargeted at about 15 %, 50 % and
//      90 % of their trajectories, some without new waypoints (W = 0), some at their path's last
//      sample (at rest: no stopping waypoint) or a nanosecond before it, a planner without a plan, a time outside the plan and a
//      non-positive stopping acceleration (the right status; the slot is the untouched twin's, by
//      GetPath and by the next Plan);
//   2. position, velocity and stopping point equal the mirror's TrajectoryBuffer::Get*AtTime and
//      ComputeStoppingPoint; the resident spline equals the mirror path's;
//   3. three successive Plans: every planner equals one mirror PathTimingTrajectory given
//      GetPositionAtTime / GetVelocityAtTime on its trajectory in a TrajectoryBuffer,
//      ComputeStoppingPoint, SetWaypoints, the limits, SetInitialVelocity and SetPath. Every moving
//      planner's first Plan after the retarget is OK; the retarget itself leaves the trajectories
//      as they were, and the new trajectory joins the old at the retarget time;
//   4. a second retarget with long waypoint lists grows the per-planner capacity.
// Then through the C-ABI: 5. the _device entry on a non-blocking stream, with a Plan enqueued right
// after it, equals the host entry; a Cartesian set gives TPAMD_E_UNSUPPORTED and call-level errors
// change nothing.
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
#include "../../x-edr-trajectory-planning_amd/host/path_tools.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"

#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::Nanoseconds;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static bool SameRow(const double *a, const VectorXd &b) { return std::memcmp(a, b.data(), b.size() * 8) == 0; }
static VectorXd RandomVec(int D, double lo, double hi) {
  VectorXd v(D);
  for (int d = 0; d < D; d++) v[d] = lo + (hi - lo) * Rnd();
  return v;
}
static std::vector<VectorXd> RandomWaypoints(int W, int D) {
  std::vector<VectorXd> w;
  for (int i = 0; i < W; i++) w.push_back(RandomVec(D, -1.5, 1.5));
  return w;
}

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

// What the reference-named sequence gives one mirror planner at `time`: position, velocity, stopping
// point and the new path (null where a step fails; *code says which).
struct MirrorRetarget {
  StatusCode code = StatusCode::kOk;
  VectorXd position, velocity, stop;
  bool at_rest = false;
  std::shared_ptr<TimeableJointSplinePath> path;
};

static MirrorRetarget RetargetMirror(const PathTimingTrajectory &m, int64_t time_ns, int D, int N, double delta,
                                     double rounding, const std::vector<VectorXd> &wps, const VectorXd &vmax,
                                     const VectorXd &amax, const VectorXd &stop_acc) {
  MirrorRetarget r;
  auto made = TrajectoryBuffer::Create();
  CHECK(made.ok());
  const std::shared_ptr<TrajectoryBuffer> buffer = made.value();
  if (m.GetNumTimeSamples() > 0)
    CHECK(buffer->InsertSegment({m.GetTime().data(), m.GetTime().size()}, {m.GetPositions().data(), m.GetPositions().size()},
                                {m.GetVelocities().data(), m.GetVelocities().size()},
                                {m.GetAccelerations().data(), m.GetAccelerations().size()}).ok());
  const auto pos = buffer->GetPositionAtTime(FromUnixNanos(time_ns));
  const auto vel = buffer->GetVelocityAtTime(FromUnixNanos(time_ns));
  if (!pos.ok() || !vel.ok()) {
    r.code = pos.status().code();
    return r;
  }
  const auto stop = ComputeStoppingPoint({pos.value().data(), (size_t)D}, {vel.value().data(), (size_t)D},
                                         {stop_acc.data(), (size_t)D}, rounding);
  if (!stop.ok()) {
    r.code = stop.status().code();
    return r;
  }
  r.position = pos.value(); r.velocity = vel.value(); r.stop = stop.value();
  r.at_rest = r.velocity.maxAbs() < 100 * 2.220446049250313e-16;
  std::vector<VectorXd> list = {r.position};
  if (!r.at_rest) list.push_back(r.stop);
  list.insert(list.end(), wps.begin(), wps.end());
  r.path = HostPath(D, N, delta, rounding, list, vmax, amax, &r.velocity);
  return r;
}

static void TestAgainstMirrors(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 70, N = 100, P0 = 10;
  const int kNoPlan = 67, kOutside = 68, kBadAcc = 69, kFirstAtEnd = 60;    // the special planners
  const double delta = 0.005, rounding = 0.2;
  const int64_t step = (skip ? 4 : 1) * kMs, horizon = 400 * kMs, start = 2000 * kMs;
  g_seed = 9100 + D * 13 + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(skip ? 4 : 1)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet dev(opt, B, P0), twin(opt, B, P0);
  CHECK(dev.status().ok() && twin.status().ok());
  if (!dev.status().ok() || !twin.status().ok()) return;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  std::vector<size_t> loaded;
  std::vector<std::vector<VectorXd>> wps;
  std::vector<VectorXd> vmax(B), amax(B), lv, la;
  for (int b = 0; b < B; b++) {
    vmax[b] = RandomVec(D, 1.0, 2.0);
    amax[b] = RandomVec(D, 2.0, 5.0);
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    if (b == kNoPlan) continue;
    loaded.push_back(b);
    wps.push_back(RandomWaypoints(RndInt(2, 4), D));
    lv.push_back(vmax[b]);
    la.push_back(amax[b]);
    paths[b] = HostPath(D, N, delta, rounding, wps.back(), vmax[b], amax[b], nullptr);
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  for (PathTimingTrajectorySet *s : {&dev, &twin}) {
    const auto st = s->SetWaypointPaths(loaded, wps, lv, la, {}, rounding, delta);
    for (const auto &x : st) CHECK(x.ok());
  }
  // the first Plan: 0.4 s for the moving planners, to the end of the path for kFirstAtEnd .. kNoPlan - 1
  std::vector<Time> starts(B, FromUnixNanos(start));
  std::vector<Duration> horizons(B, Nanoseconds(horizon));
  for (int b = kFirstAtEnd; b < kNoPlan; b++) horizons[b] = Nanoseconds((int64_t)100000 * kMs);
  const auto first = dev.Plan(starts, horizons);
  const auto first_twin = twin.Plan(starts, horizons);
  for (int b = 0; b < B; b++) {
    CHECK(first[b].code() == first_twin[b].code());
    if (b == kNoPlan) {
      CHECK(first[b].code() == StatusCode::kFailedPrecondition);
      continue;
    }
    CHECK(first[b].ok());
    CHECK(mirrors[b]->Plan(starts[b], horizons[b]).ok());
    CHECK(CompareOne(dev, b, *mirrors[b], paths[b].get()) == 0);
  }
  // 1. one retarget call: a shuffled subset (every fifth planner below kFirstAtEnd keeps its path)
  std::vector<size_t> ids;
  for (int b = 0; b < B; b++)
    if (b >= kFirstAtEnd || b % 5 != 4) ids.push_back(b);
  for (size_t i = ids.size() - 1; i > 0; i--) std::swap(ids[i], ids[RndInt(0, (int)i)]);
  const size_t n = ids.size();
  std::vector<Time> when(n);
  std::vector<std::vector<VectorXd>> nw(n);
  std::vector<VectorXd> nv(n), na(n), sacc(n);
  std::vector<int64_t> t_ns(B, start);
  int without_waypoints = 0;
  for (size_t k = 0; k < n; k++) {
    const int b = (int)ids[k];
    const int64_t t0 = ToUnixNanos(dev.GetStartTime(b)), t1 = ToUnixNanos(dev.GetEndTime(b));
    const double fraction = k % 3 == 0 ? 0.15 : k % 3 == 1 ? 0.5 : 0.9;
    int64_t t = t0 + (int64_t)std::llround(fraction * (double)(t1 - t0) / (double)step) * step;
    if (b >= kFirstAtEnd && b < kNoPlan) {
      // the last sample, where the planner is at rest -- if its time is a whole number of
      // nanoseconds as a double; otherwise the nanosecond before it, where it still creeps
      PlannedTrajectory last;
      CHECK(dev.GetTrajectory(b, &last).ok() && !last.time.empty());
      t = (int64_t)std::llround(last.time.back() * 1e9);
      if ((double)t / 1e9 > last.time.back()) t -= 1;
    }
    if (b == kOutside) t = t1 + 10000 * kMs;
    if (b == kNoPlan) t = start + 100 * kMs;
    t_ns[b] = t;
    when[k] = FromUnixNanos(t);
    const int W = k % 7 == 3 ? 0 : RndInt(2, 4);
    without_waypoints += W == 0;
    nw[k] = RandomWaypoints(W, D);
    nv[k] = RandomVec(D, 1.0, 2.0);
    na[k] = RandomVec(D, 2.0, 5.0);
    sacc[k] = na[k];
    const double scale = k % 3 == 0 ? 1.0 : k % 3 == 1 ? 0.8 : 0.72;
    for (int d = 0; d < D; d++) sacc[k][d] = na[k][d] * scale;
    if (b == kBadAcc) sacc[k][D / 2] = k % 2 ? 0.0 : -1.0;
  }
  std::vector<PlannedTrajectory> before(B);
  for (int b = 0; b < B; b++) CHECK(dev.GetTrajectory(b, &before[b]).ok());
  const auto got = dev.RetargetWaypointPaths(ids, when, nw, nv, na, rounding, delta, sacc);
  CHECK(got.size() == n);
  int moving = 0, at_rest = 0, creeping = 0, refused = 0, max_points = 0;
  std::vector<char> retargeted(B, 0), is_moving(B, 0);
  std::vector<VectorXd> read_position(B), read_velocity(B);
  // the retarget leaves every trajectory as it was
  for (int b = 0; b < B; b++) {
    PlannedTrajectory after;
    CHECK(dev.GetTrajectory(b, &after).ok());
    CHECK(SameBits(after.time, before[b].time) && SameBits(after.positions, before[b].positions) &&
          SameBits(after.velocities, before[b].velocities) && SameBits(after.accelerations, before[b].accelerations));
  }
  for (size_t k = 0; k < n; k++) {
    const int b = (int)ids[k];
    const MirrorRetarget r = RetargetMirror(*mirrors[b], t_ns[b], D, N, delta, rounding, nw[k], nv[k], na[k], sacc[k]);
    CHECK(got[k].code() == r.code);
    if (b == kNoPlan) CHECK(got[k].code() == StatusCode::kFailedPrecondition);
    if (b == kOutside) CHECK(got[k].code() == StatusCode::kOutOfRange);
    if (b == kBadAcc) {
      CHECK(got[k].code() == StatusCode::kInvalidArgument);
      CHECK(got[k].message() == "Acceleration limits must be strictly positive.");
    }
    const double *pos = dev.LastRetargetPositions().data() + k * D, *vel = dev.LastRetargetVelocities().data() + k * D,
                 *stop = dev.LastRetargetStoppingPoints().data() + k * D;
    if (!r.path) {
      // refused: NaN rows, and the slot is the untouched twin's
      refused++;
      CHECK(b == kNoPlan || b == kOutside || b == kBadAcc);
      CHECK(std::isnan(pos[0]) && std::isnan(vel[0]) && std::isnan(stop[0]));
      std::vector<double> k1, c1, k2, c2;
      CHECK(dev.GetPath(b, &k1, &c1).ok() && twin.GetPath(b, &k2, &c2).ok());
      CHECK(SameBits(k1, k2) && SameBits(c1, c2));
      continue;
    }
    // 2. the readout, the stopping point and the resident spline are the mirror's
    CHECK(SameRow(pos, r.position) && SameRow(vel, r.velocity) && SameRow(stop, r.stop));
    std::vector<double> k1, c1;
    CHECK(dev.GetPath(b, &k1, &c1).ok());
    CHECK(SameBits(k1, r.path->knots()) && SameBits(c1, r.path->packed_control_points()));
    const int W = (int)nw[k].size(), listed = W + (r.at_rest ? 1 : 2);
    CHECK((int)dev.NumControlPoints(b) == (listed == 1 ? 4 : 3 * listed - 2));
    max_points = std::max(max_points, (int)dev.NumControlPoints(b));
    const bool at_end = b >= kFirstAtEnd && b < kNoPlan;
    CHECK(!r.at_rest || at_end);
    (r.at_rest ? at_rest : at_end ? creeping : moving)++;
    is_moving[b] = !at_end;
    read_position[b] = r.position;
    read_velocity[b] = r.velocity;
    retargeted[b] = 1;
    paths[b] = r.path;
    vmax[b] = nv[k]; amax[b] = na[k];
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
  }
  CHECK(refused == 3 && at_rest + creeping == kNoPlan - kFirstAtEnd && moving > 40 && without_waypoints >= 8);
  if (!skip) CHECK(at_rest >= 1);      // uniform samples end on the time grid
  CHECK(max_points > P0);                                       // the capacity grew
  // 3. three successive Plans, each planner from its own time
  int compared = 0, first_ok = 0, kept_samples = 0, reported = 0;
  double worst_dt = 0.0, worst_dq = 0.0, worst_dv = 0.0;
  for (int round = 0; round < 3; round++) {
    for (int b = 0; b < B; b++) {
      const int64_t from = retargeted[b] ? t_ns[b] : start + 152 * kMs;
      starts[b] = FromUnixNanos(from + round * 100 * kMs);
      horizons[b] = Nanoseconds(horizon);
    }
    const auto sd = dev.Plan(starts, horizons);
    const auto st = round == 0 ? twin.Plan(starts, horizons) : std::vector<Status>();
    for (int b = 0; b < B; b++) {
      if (b == kNoPlan) {
        CHECK(sd[b].code() == StatusCode::kFailedPrecondition);
        continue;
      }
      const Status ms = mirrors[b]->Plan(starts[b], horizons[b]);
      CHECK(sd[b].code() == ms.code());
      const int bad = CompareOne(dev, b, *mirrors[b], paths[b].get());
      CHECK(bad == 0);
      if (bad && ++reported <= 12)
        std::printf("  D %d %s round %d planner %d: differences 0x%x (status %d / mirror %d)\n", D,
                    skip ? "skip" : "uniform", round, b, bad, (int)sd[b].code(), (int)ms.code());
      compared++;
      if (round != 0) continue;
      if (is_moving[b]) {          // the condition: no moving planner's first Plan may fail
        CHECK(sd[b].ok());
        first_ok += sd[b].ok();
      }
      if (b == kOutside || b == kBadAcc) {                      // refused: the next Plan is the twin's
        PlannedTrajectory a, c;
        CHECK(st[b].code() == sd[b].code());
        CHECK(dev.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok());
        CHECK(SameBits(a.time, c.time) && SameBits(a.positions, c.positions) && SameBits(a.velocities, c.velocities));
      }
      if (!is_moving[b] || !retargeted[b] || !sd[b].ok()) continue;
      // the new trajectory starts at the retarget time, from the position and velocity read out there
      PlannedTrajectory now;
      CHECK(dev.GetTrajectory(b, &now).ok() && !now.time.empty());
      if (now.time.empty()) continue;
      const double t_sec = (double)t_ns[b] / 1e9;
      double dq = 0.0, dv = 0.0;
      for (int d = 0; d < D; d++) {
        dq = std::fmax(dq, std::fabs(now.positions[d] - read_position[b][d]));
        dv = std::fmax(dv, std::fabs(now.velocities[d] - read_velocity[b][d]));
      }
      worst_dt = std::fmax(worst_dt, std::fabs(now.time[0] - t_sec));
      worst_dq = std::fmax(worst_dq, dq);
      worst_dv = std::fmax(worst_dv, dv);
      // a first sample within a nanosecond of the time; with |qd| <= 2 sqrt(D) and |qdd| <= 5 sqrt(D)
      // that is 1e-8 in position and 1e-7 in velocity at the most
      const bool joins = std::fabs(now.time[0] - t_sec) <= 1e-9 && dq <= 1e-8 && dv <= 1e-7;
      CHECK(joins);
      kept_samples += joins;
    }
  }
  CHECK(first_ok == moving);
  CHECK(kept_samples == moving);
  // 4. long waypoint lists: the capacity grows again; the mirrors follow
  std::vector<size_t> some;
  std::vector<Time> some_when;
  std::vector<std::vector<VectorXd>> some_wps;
  std::vector<VectorXd> some_v, some_a;
  for (int b = 0; b < 12; b++) {
    if (!retargeted[b] || !is_moving[b]) continue;
    const int64_t t = t_ns[b] + 240 * kMs;
    if (t > ToUnixNanos(dev.GetEndTime(b)) || t < ToUnixNanos(dev.GetStartTime(b))) continue;
    some.push_back(b);
    some_when.push_back(FromUnixNanos(t));
    some_wps.push_back(RandomWaypoints(RndInt(20, 26), D));
    some_v.push_back(vmax[b]);
    some_a.push_back(amax[b]);
  }
  CHECK(some.size() >= 4);
  const auto grown = dev.RetargetWaypointPaths(some, some_when, some_wps, some_v, some_a, rounding, delta);
  int long_ok = 0;
  for (size_t k = 0; k < some.size(); k++) {
    const int b = (int)some[k];
    const MirrorRetarget r = RetargetMirror(*mirrors[b], ToUnixNanos(some_when[k]), D, N, delta, rounding, some_wps[k],
                                            some_v[k], some_a[k], some_a[k]);
    CHECK(got.size() && grown[k].code() == r.code && r.path);
    if (!r.path) continue;
    paths[b] = r.path;
    CHECK(mirrors[b]->SetPath(paths[b]).ok());
    max_points = std::max(max_points, (int)dev.NumControlPoints(b));
    starts[b] = some_when[k];
    const Status ms = mirrors[b]->Plan(starts[b], horizons[b]);
    (void)ms;
    long_ok++;
  }
  const auto sl = dev.Plan(starts, horizons);
  for (size_t k = 0; k < some.size(); k++) {
    const int b = (int)some[k];
    CHECK(CompareOne(dev, b, *mirrors[b], paths[b].get()) == 0);
    CHECK(sl[b].ok());
  }
  CHECK(max_points >= 3 * 22 - 2);
  std::printf("retarget vs mirrors (D %d, %s): %d moving planners retargeted and planned OK, %d at rest and %d creeping "
              "at their path's end, %d without waypoints, %d refused and unchanged, %d planner states bit-equal to the "
              "mirrors, %d new trajectories join the old (time %.1e s, position %.1e, velocity %.1e at the most), %d long "
              "lists, largest P %d (capacity started at %d)\n",
              D, skip ? "skip" : "uniform", moving, at_rest, creeping, without_waypoints, refused, compared, kept_samples,
              worst_dt, worst_dq, worst_dv, long_ok, max_points, P0);
}

// 5. through the C-ABI
static void TestCAbi(int D, int method) {
  const int B = 70, N = 100;
  g_seed = 777 + D + method;
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) return;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = N; cfg.num_points = 4;
  cfg.sampling_method = method; cfg.max_planning_iterations = 200; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = method ? 4 * kMs : kMs;
  tpamd_planner_set *h = nullptr, *d = nullptr, *c = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &h) == 0 && tpamd_planner_set_create(e, &cfg, &d) == 0);
  CHECK(tpamd_planner_set_create_cartesian(e, &cfg, 4 * N, &c) == 0);
  if (!h || !d || !c) return;
  // planners 0 .. B-2 get paths and a plan; B-1 has neither
  std::vector<int32_t> offsets = {0};
  std::vector<double> wps, vmax, amax, delta;
  for (int b = 0; b < B - 1; b++) {
    const int W = RndInt(2, 4);
    for (const auto &w : RandomWaypoints(W, D)) wps.insert(wps.end(), w.begin(), w.end());
    offsets.push_back(offsets.back() + W);
    for (int j = 0; j < D; j++) { vmax.push_back(1.0 + Rnd()); amax.push_back(2.0 + 3.0 * Rnd()); }
    delta.push_back(0.005);
  }
  std::vector<int32_t> np0(B), st0(B);
  std::vector<int64_t> s(B, 1000 * kMs), hz(B, 400 * kMs);
  std::vector<tpamd_planner_summary> sum_h(B), sum_d(B);
  for (tpamd_planner_set *ps : {h, d}) {
    CHECK(tpamd_planner_set_set_waypoints(ps, B - 1, nullptr, offsets.data(), wps.data(), 0.2, vmax.data(), amax.data(),
                                          delta.data(), nullptr, np0.data(), st0.data()) == 0);
    CHECK(tpamd_planner_set_plan(ps, s.data(), hz.data(), ps == h ? sum_h.data() : sum_d.data()) == 0);
  }
  CHECK(std::memcmp(sum_h.data(), sum_d.data(), B * sizeof(tpamd_planner_summary)) == 0);
  // the retarget: all planners, shuffled; per-planner times, W = 0 now and then, one bad stopping
  // acceleration, one time outside, the planner without a plan
  std::vector<int32_t> ids(B), roff = {0};
  for (int b = 0; b < B; b++) ids[b] = b;
  for (int i = B - 1; i > 0; i--) std::swap(ids[i], ids[RndInt(0, i)]);
  std::vector<int64_t> t(B);
  std::vector<double> rw, rv, ra, rd, rs;
  for (int k = 0; k < B; k++) {
    const int b = ids[k];
    const int64_t t0 = sum_h[b].start_time_ns, t1 = sum_h[b].end_time_ns;
    const int64_t step = cfg.time_step_ns;
    t[k] = b == B - 1 ? 1100 * kMs : t0 + (int64_t)std::llround((0.15 + 0.75 * Rnd()) * (double)(t1 - t0) / (double)step) * step;
    if (k == 11) t[k] = t1 + 5000 * kMs;
    const int W = k % 6 == 2 ? 0 : RndInt(2, 4);
    for (const auto &w : RandomWaypoints(W, D)) rw.insert(rw.end(), w.begin(), w.end());
    roff.push_back(roff.back() + W);
    for (int j = 0; j < D; j++) {
      rv.push_back(1.0 + Rnd());
      ra.push_back(2.0 + 3.0 * Rnd());
      rs.push_back(ra.back() * 0.8);
    }
    if (k == 23) rs[(size_t)k * D] = 0.0;
    rd.push_back(0.005);
  }
  const double rounding = 0.15;
  const size_t n = B;
  std::vector<int32_t> np_h(n, -1), st_h(n, -1), np_d(n, -1), st_d(n, -1);
  std::vector<double> out_h(3 * n * D, -7.0), out_d(3 * n * D, -7.0);
  CHECK(tpamd_planner_set_retarget(h, B, ids.data(), t.data(), roff.data(), rw.data(), rounding, rv.data(), ra.data(),
                                   rd.data(), rs.data(), np_h.data(), st_h.data(), out_h.data(), out_h.data() + n * D,
                                   out_h.data() + 2 * n * D) == 0);
  int ok = 0;
  for (int k = 0; k < B; k++) {
    const int want = ids[k] == B - 1 ? TPAMD_PLAN_FAILED_PRECONDITION
                     : k == 11       ? TPAMD_PLAN_OUT_OF_RANGE
                     : k == 23       ? TPAMD_PLAN_INVALID_ARGUMENT
                                     : TPAMD_PLAN_OK;
    CHECK(st_h[k] == want);
    ok += st_h[k] == TPAMD_PLAN_OK;
    if (st_h[k] != TPAMD_PLAN_OK) CHECK(out_h[(size_t)k * D] == -7.0);        // rows of refused planners stay
  }
  CHECK(ok == B - 3);
  // the device entry: inputs in device memory, a non-blocking stream, a Plan enqueued right after
  int64_t *d_t = nullptr;
  double *d_w = nullptr, *d_v = nullptr, *d_a = nullptr, *d_dl = nullptr, *d_s = nullptr, *d_out = nullptr;
  int32_t *d_np = nullptr, *d_st = nullptr;
  HIP_OK(hipMalloc(&d_t, n * 8)); HIP_OK(hipMalloc(&d_w, rw.size() * 8 + 8)); HIP_OK(hipMalloc(&d_v, rv.size() * 8));
  HIP_OK(hipMalloc(&d_a, ra.size() * 8)); HIP_OK(hipMalloc(&d_dl, n * 8)); HIP_OK(hipMalloc(&d_s, rs.size() * 8));
  HIP_OK(hipMalloc(&d_out, out_d.size() * 8)); HIP_OK(hipMalloc(&d_np, n * 4)); HIP_OK(hipMalloc(&d_st, n * 4));
  HIP_OK(hipMemcpy(d_t, t.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_w, rw.data(), rw.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_v, rv.data(), rv.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_a, ra.data(), ra.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_dl, rd.data(), n * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_s, rs.data(), rs.size() * 8, hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(d_out, out_d.data(), out_d.size() * 8, hipMemcpyHostToDevice));
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  CHECK(tpamd_planner_set_retarget_device(d, B, ids.data(), d_t, roff.data(), d_w, rounding, d_v, d_a, d_dl, d_s, d_np,
                                          d_st, d_out, d_out + n * D, d_out + 2 * n * D, stream) == 0);
  std::vector<int64_t> s2(B), hz2(B, 400 * kMs);
  for (int k = 0; k < B; k++) s2[ids[k]] = st_h[k] == TPAMD_PLAN_OK ? t[k] : 1152 * kMs;
  CHECK(tpamd_planner_set_plan(d, s2.data(), hz2.data(), sum_d.data()) == 0);
  CHECK(tpamd_planner_set_plan(h, s2.data(), hz2.data(), sum_h.data()) == 0);
  CHECK(std::memcmp(sum_h.data(), sum_d.data(), B * sizeof(tpamd_planner_summary)) == 0);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipMemcpy(np_d.data(), d_np, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(st_d.data(), d_st, n * 4, hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(out_d.data(), d_out, out_d.size() * 8, hipMemcpyDeviceToHost));
  CHECK(np_d == np_h && st_d == st_h && SameBits(out_d, out_h));
  int planned = 0;
  for (int k = 0; k < B; k++) planned += st_h[k] == TPAMD_PLAN_OK && sum_h[ids[k]].status == TPAMD_PLAN_OK;
  CHECK(planned == ok);                                         // every retargeted planner's Plan is OK
  auto path_of = [&](tpamd_planner_set *ps, int b, std::vector<double> *k, std::vector<double> *cp) {
    int32_t P = 0;
    CHECK(tpamd_planner_set_download_path(ps, b, &P, nullptr, nullptr, 0) == 0);
    k->assign(P ? P + 3 : 0, 0.0);
    cp->assign((size_t)P * D, 0.0);
    if (P) CHECK(tpamd_planner_set_download_path(ps, b, &P, k->data(), cp->data(), P) == 0);
    return P;
  };
  int same = 0;
  for (int k = 0; k < B; k++) {
    std::vector<double> k1, c1, k2, c2;
    const int P1 = path_of(h, ids[k], &k1, &c1), P2 = path_of(d, ids[k], &k2, &c2);
    same += P1 == P2 && P1 == np_h[k] && SameBits(k1, k2) && SameBits(c1, c2);
  }
  CHECK(same == B);
  for (int b = 0; b < B; b++) {
    const int rows = (int)sum_h[b].num_samples;
    CHECK(rows == (int)sum_d[b].num_samples);
    if (rows == 0) continue;
    std::vector<double> a((size_t)rows * (1 + 2 * D)), bb(a.size());
    CHECK(tpamd_planner_set_download_trajectory(h, b, 0, rows, a.data(), nullptr, nullptr, nullptr, a.data() + rows,
                                                a.data() + rows * (1 + D), nullptr) == 0);
    CHECK(tpamd_planner_set_download_trajectory(d, b, 0, rows, bb.data(), nullptr, nullptr, nullptr, bb.data() + rows,
                                                bb.data() + rows * (1 + D), nullptr) == 0);
    CHECK(SameBits(a, bb));
  }
  // a Cartesian set, and call-level errors: nothing is written
  std::vector<int32_t> st3(3, -7), np3(3, -7), off3 = {0, 1, 2, 3}, bad_ids = {0, 2, 0}, off_dec = {0, 2, 1, 3};
  std::vector<int64_t> t3(3, 1100 * kMs);
  std::vector<double> w3(3 * D, 0.5), v3(3 * D, 1.5), a3(3 * D, 3.0), dl3(3, 0.005);
  CHECK(tpamd_planner_set_retarget(c, 3, nullptr, t3.data(), off3.data(), w3.data(), 0.2, v3.data(), a3.data(), dl3.data(),
                                   nullptr, np3.data(), st3.data(), nullptr, nullptr, nullptr) == TPAMD_E_UNSUPPORTED);
  CHECK(tpamd_planner_set_retarget_device(c, 3, nullptr, d_t, off3.data(), d_w, 0.2, d_v, d_a, d_dl, nullptr, d_np, d_st,
                                          nullptr, nullptr, nullptr, stream) == TPAMD_E_UNSUPPORTED);
  CHECK(tpamd_planner_set_retarget(h, 3, bad_ids.data(), t3.data(), off3.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                   dl3.data(), nullptr, np3.data(), st3.data(), nullptr, nullptr, nullptr) ==
        TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_retarget(h, 3, nullptr, t3.data(), off_dec.data(), w3.data(), 0.2, v3.data(), a3.data(),
                                   dl3.data(), nullptr, np3.data(), st3.data(), nullptr, nullptr, nullptr) ==
        TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_retarget(h, 3, nullptr, nullptr, off3.data(), w3.data(), 0.2, v3.data(), a3.data(), dl3.data(),
                                   nullptr, np3.data(), st3.data(), nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_retarget_device(d, 3, bad_ids.data(), d_t, off3.data(), d_w, 0.2, d_v, d_a, d_dl, nullptr, d_np,
                                          d_st, nullptr, nullptr, nullptr, stream) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(st3[0] == -7 && np3[0] == -7);
  for (int k = 0; k < 3; k++) {
    std::vector<double> k1, c1, k2, c2;
    CHECK(path_of(h, ids[k], &k1, &c1) == path_of(d, ids[k], &k2, &c2) && SameBits(k1, k2) && SameBits(c1, c2));
  }
  HIP_OK(hipStreamDestroy(stream));
  for (void *p : {(void *)d_t, (void *)d_w, (void *)d_v, (void *)d_a, (void *)d_dl, (void *)d_s, (void *)d_out,
                  (void *)d_np, (void *)d_st})
    HIP_OK(hipFree(p));
  tpamd_planner_set_destroy(c);
  tpamd_planner_set_destroy(h);
  tpamd_planner_set_destroy(d);
  tpamd_engine_destroy(e);
  std::printf("retarget C-ABI (D %d, method %d): device entry on a non-blocking stream = host entry, %d planners "
              "retargeted and planned, Cartesian set and call-level errors refused\n", D, method, planned);
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) TestAgainstMirrors(m, D);
  for (int D : {3, 7})
    for (int m : {0, 1}) TestCAbi(D, m);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

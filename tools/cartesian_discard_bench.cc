// Streaming IK tables with and without discarding the consumed rows (run on the GPU,
// tools/gpu_cartesian_discard_bench.py): the shape, paths and callbacks of tools/cartesian_stream_bench.cc
// -- 1024 planners x 7 joints, N = 1000 path samples, 4 ms time step, 750 ms horizon, a replan every
// 200 ms until every planner is at its target. Two streaming sets walk the same paths:
//   (a) keep     PlanStreaming only: nothing is ever taken out of a table
//   (b) discard  PlanStreaming, then DiscardIkRows() after every completed Plan (timed on its own)
// Reported per set: final and peak table capacity (rows per planner), tpamd_planner_set_device_bytes
// at the target and its peak, the Plan calls after which the capacity had changed (each is one
// reallocation with a copy), ms per steady replan (nobody waited for rows) and per replan with
// waiting planners (host IK callbacks included); for (b) ms per discard call and the rows the
// discards removed. The tool ASSERTS that (a) and (b) hold bit-equal trajectories after every Plan
// (exit status 1 otherwise). One JSON line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../x-edr-trajectory-planning_amd/host/timeable_path_cartesian_spline.h"

using namespace trajectory_planning;
using tpamd::compat::AngleAxisd;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Matrix6Xd;
using tpamd::compat::Milliseconds;
using tpamd::compat::Pose3d;
using tpamd::compat::Vector3d;

static const int D = 7;
static double now() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static double median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v.empty() ? 0.0 : v[v.size() / 2];
}
static Status PassThroughIk(const VectorXd &, const std::vector<Pose3d> &, const std::vector<VectorXd> &joints,
                            std::vector<VectorXd> *result) {
  *result = joints;
  return tpamd::compat::OkStatus();
}
static Status FakeJacobian(const VectorXd &q, Matrix6Xd *J) {
  for (int r = 0; r < 6; r++)
    for (int d = 0; d < D; d++) (*J)(r, d) = 0.2 * std::sin(q[d] * (r + 1.0) + 0.31 * d) + (r == d ? 1.0 : 0.0);
  return tpamd::compat::OkStatus();
}

struct Goal {
  std::vector<Pose3d> poses;
  std::vector<VectorXd> joints;
  std::vector<double> vmax, amax;
  double vt, vr, delta;
};


static std::shared_ptr<TimeableCartesianSplinePath> MakePath(const Goal &g, int N) {
  CartesianPathOptions opt;
  opt.set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(g.delta);
  opt.set_path_ik_func(PassThroughIk).set_jacobian_func(FakeJacobian);
  auto path = std::make_shared<TimeableCartesianSplinePath>(opt);
  path->SetMaxJointVelocity({g.vmax.data(), g.vmax.size()});
  path->SetMaxJointAcceleration({g.amax.data(), g.amax.size()});
  path->SetMaxCartesianVelocity(g.vt, g.vr);
  path->SetWaypoints({g.poses.data(), g.poses.size()}, {g.joints.data(), g.joints.size()});
  return path;
}

static bool SameBits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
}
// every planner's trajectory of the two sets, bit for bit
static long Differences(const PathTimingTrajectorySet &x, const PathTimingTrajectorySet &y, const std::vector<size_t> &all) {
  std::vector<PlannedTrajectory> tx, ty;
  if (!x.GetTrajectories(all, &tx).ok() || !y.GetTrajectories(all, &ty).ok() || tx.size() != ty.size()) return (long)all.size();
  long bad = 0;
  for (size_t b = 0; b < tx.size(); b++)
    bad += !(SameBits(tx[b].time, ty[b].time) && SameBits(tx[b].path_parameter, ty[b].path_parameter) &&
             SameBits(tx[b].positions, ty[b].positions) && SameBits(tx[b].velocities, ty[b].velocities) &&
             SameBits(tx[b].accelerations, ty[b].accelerations)) ||
           x.GetNumTimeSamples(b) != y.GetNumTimeSamples(b);
  return bad;
}
struct SetStats {
  std::vector<double> steady, busy, discard;
  int cap_first = 0, cap_peak = 0, cap_final = 0, cap_changes = 0;
  size_t bytes_first = 0, bytes_peak = 0, bytes_final = 0;
  long live_rows_final = 0, rows_final = 0;
};
static int Capacity(const PathTimingTrajectorySet &set) {
  int32_t cap = 0;
  set.GetIkTableInfo(0, nullptr, nullptr, &cap);
  return cap;
}
static void Observe(const PathTimingTrajectorySet &set, SetStats *s) {
  const int cap = Capacity(set);
  if (s->cap_final && cap != s->cap_final) s->cap_changes++;
  s->cap_final = cap;
  s->cap_peak = std::max(s->cap_peak, cap);
  s->bytes_final = set.DeviceBytes();
  s->bytes_peak = std::max(s->bytes_peak, s->bytes_final);
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int N = argc > 2 ? std::atoi(argv[2]) : 1000;
  const int64_t kMs = 1000000;
  unsigned long long seed = 20261016;
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  std::vector<Goal> goals(B);
  for (int b = 0; b < B; b++) {
    Goal &g = goals[b];
    const int W = 3 + (int)(rnd() * 4.0);
    for (int i = 0; i < W; i++) {
      VectorXd q(D);
      for (int d = 0; d < D; d++) q[d] = 2.0 * rnd() - 1.0;
      AngleAxisd aa;
      aa.axis = Vector3d(0, 0, 1);
      aa.angle = 0.2 + 0.6 * rnd();
      g.joints.push_back(q);
      g.poses.push_back(Pose3d(aa.toQuaternion(), Vector3d(q[0], q[1], q[2])));
    }
    for (int d = 0; d < D; d++) g.vmax.push_back(0.5 + 0.6 * rnd());
    for (int d = 0; d < D; d++) g.amax.push_back(1.2 + 1.8 * rnd());
    g.vt = 0.3 + 0.3 * rnd();
    g.vr = 0.8 + 0.4 * rnd();
    g.delta = 0.005;
    const double kend = MakePath(g, N)->knots().back();
    g.delta = ((b % 2) ? 0.25 : 0.4) * kend / (N - 1);
  }
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  const auto horizon = Milliseconds(750);
  std::vector<size_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> kp(B), dp(B);
  for (int b = 0; b < B; b++) { kp[b] = MakePath(goals[b], N); dp[b] = MakePath(goals[b], N); }
  PathTimingTrajectorySet keep(opt, B, CartesianTableCapacity{(size_t)N}), disc(opt, B, CartesianTableCapacity{(size_t)N});
  if (!keep.status().ok() || !disc.status().ok()) { std::printf("{\"error\": \"no set\"}\n"); return 1; }
  if (!keep.SetCartesianPaths(kp, /*streaming=*/true).ok() || !disc.SetCartesianPaths(dp, /*streaming=*/true).ok()) {
    std::printf("{\"error\": \"SetCartesianPaths\"}\n");
    return 1;
  }
  SetStats ks, ds;
  ks.cap_final = ds.cap_final = Capacity(keep);     // a growth within the first Plan counts too
  long differences = 0, compared = 0, suspensions = 0, rows_discarded = 0;
  int walk_plans = 0, at_target = 0;
  std::vector<int32_t> first(B, 0);
  for (int k = 0; k <= 400; k++) {
    std::vector<tpamd::compat::Time> starts(B);
    bool done = k > 0;
    for (int b = 0; b < B; b++) {
      starts[b] = k ? keep.GetNextPlanStartTime(b, FromUnixNanos(k * 200 * kMs)) : FromUnixNanos(0);
      done = done && keep.IsTrajectoryAtEnd(b);
    }
    if (done) break;
    const std::vector<tpamd::compat::Duration> hz(B, horizon);
    double t0 = now();
    keep.PlanStreaming(starts, hz);
    const double tk = now() - t0;
    const int waited = keep.SuspensionsOfLastPlan();
    t0 = now();
    disc.PlanStreaming(starts, hz);
    const double td = now() - t0;
    if (disc.SuspensionsOfLastPlan() != waited) differences++;
    Observe(keep, &ks);
    Observe(disc, &ds);
    t0 = now();
    const auto fr = disc.DiscardIkRows();
    const double tdisc = now() - t0;
    if (!fr.ok()) { std::printf("{\"error\": \"DiscardIkRows\"}\n"); return 1; }
    for (int b = 0; b < B; b++) { rows_discarded += (*fr)[b] - first[b]; first[b] = (*fr)[b]; }
    suspensions += waited;
    if (k == 0) {
      ks.cap_first = ks.cap_final; ds.cap_first = ds.cap_final;
      ks.bytes_first = ks.bytes_final; ds.bytes_first = ds.bytes_final;
    } else {          // the first Plan is the warm-up
      (waited ? ks.busy : ks.steady).push_back(1e3 * tk);
      (waited ? ds.busy : ds.steady).push_back(1e3 * td);
      ds.discard.push_back(1e3 * tdisc);
    }
    differences += Differences(keep, disc, all);
    compared += B;
    walk_plans++;
  }
  for (int b = 0; b < B; b++) {
    at_target += keep.IsTrajectoryAtEnd(b) && disc.IsTrajectoryAtEnd(b);
    int32_t f = 0, r = 0;
    disc.GetIkTableInfo(b, &f, &r, nullptr);
    ds.live_rows_final += r - f; ds.rows_final += r;
    keep.GetIkTableInfo(b, &f, &r, nullptr);
    ks.live_rows_final += r - f; ks.rows_final += r;
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"time_step_ms\": 4, \"horizon_ms\": 750, "
              "\"replan_every_ms\": 200, \"walk_plan_calls\": %d, \"planners_at_target\": %d, \"walk_suspensions\": %ld, "
              "\"trajectories_compared\": %ld, \"trajectories_different\": %ld, \"replans_no_rows\": %zu, "
              "\"replans_with_waiting\": %zu, ", B, D, N, walk_plans, at_target, suspensions, compared, differences,
              ks.steady.size(), ks.busy.size());
  const SetStats *sets[2] = {&ks, &ds};
  const char *names[2] = {"keep", "discard"};
  for (int i = 0; i < 2; i++) {
    const SetStats &s = *sets[i];
    std::printf("\"%s_table_capacity_after_first_plan\": %d, \"%s_table_capacity_peak\": %d, \"%s_table_capacity_final\": %d, "
                "\"%s_plan_calls_that_reallocated\": %d, \"%s_device_bytes_after_first_plan\": %zu, "
                "\"%s_device_bytes_peak\": %zu, \"%s_device_bytes_final\": %zu, \"%s_live_rows_final\": %ld, "
                "\"%s_path_rows_supplied\": %ld, \"%s_replan_no_rows_ms\": %.3f, \"%s_replan_with_waiting_ms\": %.3f, ",
                names[i], s.cap_first, names[i], s.cap_peak, names[i], s.cap_final, names[i], s.cap_changes, names[i],
                s.bytes_first, names[i], s.bytes_peak, names[i], s.bytes_final, names[i], s.live_rows_final, names[i],
                s.rows_final, names[i], median(s.steady), names[i], median(s.busy));
  }
  std::vector<double> sorted = ds.discard;
  std::sort(sorted.begin(), sorted.end());
  std::printf("\"discard_call_ms_median\": %.3f, \"discard_call_ms_max\": %.3f, \"discard_calls\": %zu, "
              "\"rows_discarded\": %ld}\n", median(ds.discard), sorted.empty() ? 0.0 : sorted.back(), ds.discard.size() + 1,
              rows_discarded);
  return differences == 0 && at_target == B ? 0 : 1;
}

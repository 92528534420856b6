// Streaming IK tables against whole tables (run on the GPU, tools/gpu_cartesian_stream_bench.py): the
// shape and the computing callbacks of tools/cartesian_set_bench.cc -- 1024 planners x 7 joints,
// N = 1000 path samples, 4 ms time step, 750 ms horizon, a replan every 200 ms; paths over W in 3..6
// random waypoints with delta = f kend / (N - 1), f in {0.4, 0.25} mixed; the IK callback returns the
// joint targets, the Jacobian callback is J[c][d] = 0.2 sin(q_d (c + 1) + 0.31 d) + (c == d). Two ways:
//   (a) whole      BuildIkTable on every path, SetIkTables, Plan: the table covers the path before
//                  the first Plan (the route that existed; the baseline of every figure)
//   (b) streaming  SetCartesianPaths(paths, streaming): rows 0 .. N-1, then PlanStreaming, which
//                  extends the tables from the paths when a planner waits for rows
// Per way, medians of `reps` after a warm-up: the time from a fresh path to the first trajectory split
// into IK and Jacobian callbacks on the host, upload and Plan; the replans of one walk to the target
// split into those that needed no rows and those in which planners waited (plan + append + resume;
// for (a) the same Plan calls of its own walk); resident table bytes after the first Plan and at the
// target; PCIe bytes of the last tpamd call of a Plan. The tool ASSERTS that (a) and (b) hold bit-equal
// trajectories after every Plan of the walk (exit status 1 otherwise). One JSON line.
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
static size_t TableBytes(const PathTimingTrajectorySet &set, int B) {
  size_t rows = 0;
  for (int b = 0; b < B; b++) rows += (size_t)std::max(set.GetIkTableRows(b), 0);
  return rows * (size_t)(7 * D) * 8;          // D positions and 6 D Jacobian entries per row
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int N = argc > 2 ? std::atoi(argv[2]) : 1000;
  const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
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
  std::vector<double> w_ik, w_up, w_plan, s_ik, s_up, s_plan, s_plan_ik;
  std::vector<double> w_steady, w_busy, s_steady, s_busy, s_busy_ik;
  size_t w_bytes_first = 0, w_bytes_end = 0, s_bytes_first = 0, s_bytes_end = 0, w_pcie = 0, s_pcie_steady = 0, s_pcie_resume = 0;
  long differences = 0, compared = 0, suspensions = 0;
  int walk_plans = 0, at_target = 0;
  for (int rep = 0; rep < reps + 1; rep++) {        // rep 0 is the warm-up
    // ---- (a) whole tables: fresh paths, the callbacks over the whole path, the upload, the first Plan
    std::vector<std::shared_ptr<TimeableCartesianSplinePath>> wp(B), sp(B);
    for (int b = 0; b < B; b++) { wp[b] = MakePath(goals[b], N); sp[b] = MakePath(goals[b], N); }
    IkTables tables;
    tables.row_offsets.assign(1, 0);
    double t0 = now();
    int longest = 0;
    for (int b = 0; b < B; b++) {
      if (!wp[b]->BuildIkTable(&tables.ik_positions, &tables.jacobians).ok()) { std::printf("{\"error\": \"BuildIkTable\"}\n"); return 1; }
      tables.row_offsets.push_back((int32_t)(tables.ik_positions.size() / D));
      longest = std::max(longest, tables.row_offsets[b + 1] - tables.row_offsets[b]);
      tables.path_end.push_back(wp[b]->knots().back());
      tables.max_translational_velocity.push_back(goals[b].vt);
      tables.max_rotational_velocity.push_back(goals[b].vr);
      tables.delta.push_back(goals[b].delta);
      tables.max_velocity.insert(tables.max_velocity.end(), goals[b].vmax.begin(), goals[b].vmax.end());
      tables.max_acceleration.insert(tables.max_acceleration.end(), goals[b].amax.begin(), goals[b].amax.end());
    }
    const double t_w_ik = now() - t0;
    PathTimingTrajectorySet whole(opt, B, CartesianTableCapacity{(size_t)longest});
    PathTimingTrajectorySet stream(opt, B, CartesianTableCapacity{(size_t)N});
    if (!whole.status().ok() || !stream.status().ok()) { std::printf("{\"error\": \"no set\"}\n"); return 1; }
    t0 = now();
    if (!whole.SetIkTables(all, tables).ok()) { std::printf("{\"error\": \"SetIkTables\"}\n"); return 1; }
    const double t_w_up = now() - t0;
    t0 = now();
    whole.Plan(FromUnixNanos(0), horizon);
    const double t_w_plan = now() - t0;
    // ---- (b) streaming: rows 0 .. N-1 (callbacks + upload in one call), then the first Plan
    t0 = now();
    if (!stream.SetCartesianPaths(sp, /*streaming=*/true).ok()) { std::printf("{\"error\": \"SetCartesianPaths\"}\n"); return 1; }
    const double t_s_set = now() - t0, t_s_ik = stream.HostCallbackSecondsOfLastCall();
    t0 = now();
    stream.PlanStreaming(FromUnixNanos(0), horizon);
    const double t_s_plan = now() - t0, t_s_plan_ik = stream.HostCallbackSecondsOfLastCall();
    differences += Differences(whole, stream, all);
    compared += B;
    if (rep > 0) {
      w_ik.push_back(1e3 * t_w_ik); w_up.push_back(1e3 * t_w_up); w_plan.push_back(1e3 * t_w_plan);
      s_ik.push_back(1e3 * t_s_ik); s_up.push_back(1e3 * (t_s_set - t_s_ik)); s_plan.push_back(1e3 * t_s_plan);
      s_plan_ik.push_back(1e3 * t_s_plan_ik);
    }
    if (rep != 1) continue;
    // ---- one walk to the target (the first measured repeat): every replan of both sets, compared
    w_bytes_first = TableBytes(whole, B);
    s_bytes_first = TableBytes(stream, B);
    for (int k = 1; k <= 400; k++) {
      std::vector<tpamd::compat::Time> starts(B);
      bool done = true;
      for (int b = 0; b < B; b++) {
        starts[b] = whole.GetNextPlanStartTime(b, FromUnixNanos(k * 200 * kMs));
        done = done && whole.IsTrajectoryAtEnd(b);
      }
      if (done) break;
      const std::vector<tpamd::compat::Duration> hz(B, horizon);
      t0 = now();
      whole.Plan(starts, hz);
      const double tw = now() - t0;
      w_pcie = std::max(w_pcie, whole.LastPlanBytesOverPcie());
      t0 = now();
      stream.PlanStreaming(starts, hz);
      const double ts = now() - t0;
      const int waited = stream.SuspensionsOfLastPlan();
      suspensions += waited;
      if (waited) {
        w_busy.push_back(1e3 * tw); s_busy.push_back(1e3 * ts); s_busy_ik.push_back(1e3 * stream.HostCallbackSecondsOfLastCall());
        s_pcie_resume = std::max(s_pcie_resume, stream.LastPlanBytesOverPcie());
      } else {
        w_steady.push_back(1e3 * tw); s_steady.push_back(1e3 * ts);
        s_pcie_steady = std::max(s_pcie_steady, stream.LastPlanBytesOverPcie());
      }
      differences += Differences(whole, stream, all);
      compared += B;
      walk_plans++;
    }
    for (int b = 0; b < B; b++) at_target += whole.IsTrajectoryAtEnd(b) && stream.IsTrajectoryAtEnd(b);
    w_bytes_end = TableBytes(whole, B);
    s_bytes_end = TableBytes(stream, B);
  }
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"time_step_ms\": 4, \"horizon_ms\": 750, "
              "\"replan_every_ms\": 200, \"reps\": %d, \"trajectories_compared\": %ld, \"trajectories_different\": %ld, "
              "\"walk_plan_calls\": %d, \"planners_at_target\": %d, \"walk_suspensions\": %ld, "
              "\"whole_host_callbacks_ms\": %.1f, \"whole_upload_ms\": %.3f, \"whole_first_plan_ms\": %.3f, "
              "\"whole_time_to_first_trajectory_ms\": %.1f, "
              "\"streaming_host_callbacks_ms\": %.1f, \"streaming_upload_ms\": %.3f, \"streaming_first_plan_ms\": %.3f, "
              "\"streaming_first_plan_host_callbacks_ms\": %.1f, \"streaming_time_to_first_trajectory_ms\": %.1f, "
              "\"whole_replan_no_rows_ms\": %.3f, \"streaming_replan_no_rows_ms\": %.3f, \"replans_no_rows\": %zu, "
              "\"whole_replan_same_calls_ms\": %.3f, \"streaming_replan_with_waiting_ms\": %.3f, "
              "\"streaming_replan_with_waiting_host_callbacks_ms\": %.3f, \"replans_with_waiting\": %zu, "
              "\"whole_table_bytes_after_first_plan\": %zu, \"whole_table_bytes_at_target\": %zu, "
              "\"streaming_table_bytes_after_first_plan\": %zu, \"streaming_table_bytes_at_target\": %zu, "
              "\"whole_pcie_bytes_per_plan_call\": %zu, \"streaming_pcie_bytes_per_plan_call_no_rows\": %zu, "
              "\"streaming_pcie_bytes_last_resume\": %zu}\n",
              B, D, N, reps, compared, differences, walk_plans, at_target, suspensions, median(w_ik), median(w_up),
              median(w_plan), median(w_ik) + median(w_up) + median(w_plan), median(s_ik), median(s_up), median(s_plan),
              median(s_plan_ik), median(s_ik) + median(s_up) + median(s_plan), median(w_steady), median(s_steady),
              s_steady.size(), median(w_busy), median(s_busy), median(s_busy_ik), s_busy.size(), w_bytes_first, w_bytes_end,
              s_bytes_first, s_bytes_end, w_pcie, s_pcie_steady, s_pcie_resume);
  return differences == 0 && at_target == B ? 0 : 1;
}

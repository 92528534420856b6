// Cartesian planning throughput (run on the GPU): 1024 planners x 7 joints, N = 1000 path samples,
// 4 ms time step, 750 ms horizon, a replan every 200 ms. The paths are TimeableCartesianSplinePaths
// over W in 3..6 random waypoints (joint waypoints uniform in [-1, 1]^7, the pose translation follows
// the first three joints) with delta = f kend / (N - 1), f in {0.4, 0.25} mixed; the IK callback
// returns the joint targets (a per-sample, closed-form solver), the Jacobian callback is
// J[c][d] = 0.2 sin(q_d (c + 1) + 0.31 d) + (c == d). Three ways:
//   (a) set     a Cartesian PathTimingTrajectorySet: the IK tables are uploaded once
//               (SetCartesianPaths), a Plan call reads its windows out of the resident tables
//   (b) batch   PathTimingTrajectory::PlanBatch with the same paths, whose callbacks LOOK the rows of
//               (a)'s tables UP (a hash of the joint target / the joint position finds the row), so
//               that (b) times the route and not the callbacks: per window and planner SamplePath,
//               the packing and N D + N 6 D doubles up (the route that existed before Cartesian
//               sets; not the code under test)
//   (c) joint   a joint-space set of the same size over the same joint waypoints, for scale
// The tables of (a) are built once with the computing callbacks above (table_build_on_host_ms: what
// the user's IK and Jacobian cost, paid once per path by (a) and spread over the windows by a real
// (b)); set_time_to_first_trajectory_ms adds build, upload and the first Plan.
// Medians of `reps` after a warm-up. One JSON line.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <memory>
#include <unordered_map>
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

// The rows of one planner's table by the bits of the joint position.
struct Lookup {
  const double *q = nullptr, *J = nullptr;     // [rows][D], [rows][6][D]
  std::unordered_map<uint64_t, int> row;
  long misses = 0;
  static uint64_t Key(const double *v) {
    uint64_t h = 1469598103934665603ULL;
    for (int d = 0; d < D; d++) {
      uint64_t b;
      std::memcpy(&b, v + d, 8);
      h = (h ^ b) * 1099511628211ULL;
    }
    return h;
  }
  int Find(const double *v) const {
    const auto it = row.find(Key(v));
    return it != row.end() && std::memcmp(q + (size_t)it->second * D, v, D * 8) == 0 ? it->second : -1;
  }
};

struct Goal {
  std::vector<Pose3d> poses;
  std::vector<VectorXd> joints;
  std::vector<double> vmax, amax;
  double vt, vr, delta;
};

// lookup null: the computing callbacks; else both callbacks look the table up (a miss computes and is counted)
static std::shared_ptr<TimeableCartesianSplinePath> MakePath(const Goal &g, int N, std::shared_ptr<Lookup> lookup = nullptr) {
  CartesianPathOptions opt;
  opt.set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(g.delta);
  if (!lookup) {
    opt.set_path_ik_func(PassThroughIk).set_jacobian_func(FakeJacobian);
  } else {
    opt.set_path_ik_func([lookup](const VectorXd &, const std::vector<Pose3d> &, const std::vector<VectorXd> &joints,
                                  std::vector<VectorXd> *result) -> Status {
      result->clear();
      for (const VectorXd &t : joints) {
        const int r = lookup->Find(t.data());
        if (r < 0) { lookup->misses++; result->push_back(t); continue; }
        result->push_back(VectorXd(lookup->q + (size_t)r * D, D));
      }
      return tpamd::compat::OkStatus();
    });
    opt.set_jacobian_func([lookup](const VectorXd &q, Matrix6Xd *J) -> Status {
      const int r = lookup->Find(q.data());
      if (r < 0) { lookup->misses++; return FakeJacobian(q, J); }
      std::memcpy(J->data(), lookup->J + (size_t)r * 6 * D, 6 * D * 8);
      return tpamd::compat::OkStatus();
    });
  }
  auto path = std::make_shared<TimeableCartesianSplinePath>(opt);
  path->SetMaxJointVelocity({g.vmax.data(), g.vmax.size()});
  path->SetMaxJointAcceleration({g.amax.data(), g.amax.size()});
  path->SetMaxCartesianVelocity(g.vt, g.vr);
  path->SetWaypoints({g.poses.data(), g.poses.size()}, {g.joints.data(), g.joints.size()});
  return path;
}

int main(int argc, char **argv) {
  const int B = argc > 1 ? std::atoi(argv[1]) : 1024;
  const int N = argc > 2 ? std::atoi(argv[2]) : 1000;
  const int reps = argc > 3 ? std::atoi(argv[3]) : 5;
  const bool run_batch = argc > 4 ? std::atoi(argv[4]) != 0 : true;
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
  // ---- (a) the Cartesian set. The tables are built once (the callbacks' time), then uploaded
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> paths(B);
  for (int b = 0; b < B; b++) paths[b] = MakePath(goals[b], N);
  IkTables tables;
  std::vector<size_t> all(B);
  double t0 = now();
  tables.row_offsets.assign(1, 0);
  for (int b = 0; b < B; b++) {
    all[b] = b;
    if (!paths[b]->BuildIkTable(&tables.ik_positions, &tables.jacobians).ok()) { std::printf("{\"error\": \"BuildIkTable\"}\n"); return 1; }
    tables.row_offsets.push_back((int32_t)(tables.ik_positions.size() / D));
    tables.path_end.push_back(paths[b]->knots().back());
    tables.max_translational_velocity.push_back(goals[b].vt);
    tables.max_rotational_velocity.push_back(goals[b].vr);
    tables.delta.push_back(goals[b].delta);
    tables.max_velocity.insert(tables.max_velocity.end(), goals[b].vmax.begin(), goals[b].vmax.end());
    tables.max_acceleration.insert(tables.max_acceleration.end(), goals[b].amax.begin(), goals[b].amax.end());
  }
  const double t_build = now() - t0;
  const size_t table_bytes = (tables.ik_positions.size() + tables.jacobians.size()) * 8;
  int longest = 0;
  for (int b = 0; b < B; b++) longest = std::max(longest, tables.row_offsets[b + 1] - tables.row_offsets[b]);
  std::vector<double> first_ms, replan_ms, upload_ms;
  size_t set_bytes = 0, set_device_bytes = 0;
  int at_end_checks = 0;
  for (int rep = 0; rep < reps + 1; rep++) {        // rep 0 is the warm-up
    PathTimingTrajectorySet set(opt, B, CartesianTableCapacity{(size_t)longest});
    if (!set.status().ok()) { std::printf("{\"error\": \"%s\"}\n", set.status().ToString().c_str()); return 1; }
    t0 = now();
    if (!set.SetIkTables(all, tables).ok()) { std::printf("{\"error\": \"SetIkTables\"}\n"); return 1; }
    const double t_up = now() - t0;
    t0 = now();
    const auto st = set.Plan(FromUnixNanos(0), horizon);
    const double t_first = now() - t0;
    for (int b = 0; b < B; b++) at_end_checks += st[b].ok();
    std::vector<double> re;
    for (int k = 1; k <= 5; k++) {
      std::vector<tpamd::compat::Time> starts(B);
      for (int b = 0; b < B; b++) starts[b] = set.GetNextPlanStartTime(b, FromUnixNanos(k * 200 * kMs));
      t0 = now();
      set.Plan(starts, std::vector<tpamd::compat::Duration>(B, horizon));
      re.push_back(now() - t0);
      set_bytes = std::max(set_bytes, set.LastPlanBytesOverPcie());
    }
    if (rep == 0) continue;
    upload_ms.push_back(1e3 * t_up);
    first_ms.push_back(1e3 * t_first);
    replan_ms.push_back(1e3 * median(re));
    set_device_bytes = set.DeviceBytes();
  }
  // ---- (b) PlanBatch over the same paths (fresh path objects: their IK tables start empty); the
  // callbacks look (a)'s tables up
  std::vector<double> batch_first_ms, batch_replan_ms;
  std::vector<std::shared_ptr<Lookup>> lookups(B);
  long lookup_misses = 0;
  if (run_batch) {
    for (int b = 0; b < B; b++) {
      auto l = std::make_shared<Lookup>();
      l->q = tables.ik_positions.data() + (size_t)tables.row_offsets[b] * D;
      l->J = tables.jacobians.data() + (size_t)tables.row_offsets[b] * 6 * D;
      const int rows = tables.row_offsets[b + 1] - tables.row_offsets[b];
      for (int r = 0; r < rows; r++) l->row.emplace(Lookup::Key(l->q + (size_t)r * D), r);
      lookups[b] = l;
    }
    for (int rep = 0; rep < reps + 1; rep++) {      // rep 0 is the warm-up
      std::vector<std::unique_ptr<PathTimingTrajectory>> planners;
      std::vector<PathTimingTrajectory *> ptrs;
      for (int b = 0; b < B; b++) {
        planners.push_back(std::make_unique<PathTimingTrajectory>(opt));
        planners.back()->SetPath(MakePath(goals[b], N, lookups[b]));
        ptrs.push_back(planners.back().get());
      }
      t0 = now();
      PathTimingTrajectory::PlanBatch(ptrs, FromUnixNanos(0), horizon);
      const double t_first = now() - t0;
      std::vector<double> re;
      for (int k = 1; k <= reps; k++) {
        int64_t s = k * 200 * kMs;
        for (int b = 0; b < B; b++)
          if (planners[b]->GetNumTimeSamples()) s = std::min<int64_t>(s, tpamd::compat::ToUnixNanos(planners[b]->GetEndTime()));
        t0 = now();
        PathTimingTrajectory::PlanBatch(ptrs, FromUnixNanos(s), horizon);
        re.push_back(now() - t0);
      }
      if (rep == 0) continue;
      batch_first_ms.push_back(1e3 * t_first);
      batch_replan_ms.push_back(1e3 * median(re));
    }
  }
  // ---- (c) a joint set over the same joint waypoints
  std::vector<double> joint_first_ms, joint_replan_ms;
  size_t joint_bytes = 0;
  {
    std::vector<std::shared_ptr<TimeableJointSplinePath>> jp(B);
    for (int b = 0; b < B; b++) {
      const Goal &g = goals[b];
      auto probe = std::make_shared<TimeableJointSplinePath>(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
      probe->SetWaypoints({g.joints.data(), g.joints.size()});
      const double delta = ((b % 2) ? 0.25 : 0.4) * probe->knots().back() / (N - 1);
      jp[b] = std::make_shared<TimeableJointSplinePath>(
          JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta));
      jp[b]->SetMaxJointVelocity({g.vmax.data(), g.vmax.size()});
      jp[b]->SetMaxJointAcceleration({g.amax.data(), g.amax.size()});
      jp[b]->SetWaypoints({g.joints.data(), g.joints.size()});
    }
    for (int rep = 0; rep < reps + 1; rep++) {
      PathTimingTrajectorySet set(opt, B, 16);
      set.SetPaths(jp);
      t0 = now();
      set.Plan(FromUnixNanos(0), horizon);
      const double t_first = now() - t0;
      std::vector<double> re;
      for (int k = 1; k <= 5; k++) {
        std::vector<tpamd::compat::Time> starts(B);
        for (int b = 0; b < B; b++) starts[b] = set.GetNextPlanStartTime(b, FromUnixNanos(k * 200 * kMs));
        t0 = now();
        set.Plan(starts, std::vector<tpamd::compat::Duration>(B, horizon));
        re.push_back(now() - t0);
        joint_bytes = std::max(joint_bytes, set.LastPlanBytesOverPcie());
      }
      if (rep == 0) continue;
      joint_first_ms.push_back(1e3 * t_first);
      joint_replan_ms.push_back(1e3 * median(re));
    }
  }
  for (int b = 0; b < B && run_batch; b++) lookup_misses += lookups[b]->misses;
  // what PlanBatch ships per window iteration: N D + N 6 D doubles per planner up, the window down
  const size_t batch_up = (size_t)B * ((size_t)N * D + (size_t)N * 6 * D) * 8;
  std::printf("{\"planners\": %d, \"dofs\": %d, \"path_samples\": %d, \"time_step_ms\": 4, \"horizon_ms\": 750, "
              "\"replan_every_ms\": 200, \"reps\": %d, \"planner_plans_ok_first_call\": %d, "
              "\"table_rows_total\": %d, \"table_upload_bytes\": %zu, \"table_upload_ms\": %.3f, \"table_build_on_host_ms\": %.1f, "
              "\"set_time_to_first_trajectory_ms\": %.1f, \"batch_callbacks\": \"table look-ups\", \"batch_lookup_misses\": %ld, "
              "\"set_first_plan_ms\": %.3f, \"set_replan_ms\": %.3f, \"set_pcie_bytes_per_plan_call\": %zu, \"set_device_MB\": %.1f, "
              "\"batch_first_plan_ms\": %.3f, \"batch_replan_ms\": %.3f, \"batch_upload_bytes_per_window_iteration\": %zu, "
              "\"joint_set_first_plan_ms\": %.3f, \"joint_set_replan_ms\": %.3f, \"joint_set_pcie_bytes_per_plan_call\": %zu}\n",
              B, D, N, reps, at_end_checks / (reps + 1), tables.row_offsets.back(), table_bytes, median(upload_ms), 1e3 * t_build,
              1e3 * t_build + median(upload_ms) + median(first_ms), lookup_misses,
              median(first_ms), median(replan_ms), set_bytes, set_device_bytes / 1e6, median(batch_first_ms),
              median(batch_replan_ms), batch_up, median(joint_first_ms), median(joint_replan_ms), joint_bytes);
  return 0;
}

// GPU test of CheckSolutions on the three batch classes (run by tests/test_gpu_check_mirror.py):
// BatchPathTiming, BatchWaypointTiming and BatchCartesianTiming on 16 paths of the shapes (joints,
// samples, waypoints) = (7, 65, 4) and (16, 33, 3), each timed with the option off and on.
//   * with the option off the check fields stay empty, and every timing result is bit-equal to the
//     one with it on;
//   * violations[b] == 0  <=>  the mirror's own TimeOptimalPathProfile::SolutionSatisfiesConstraints()
//     is ok on that path's constraints (the joint path's SamplePath + ConstraintSetup; for Cartesian
//     paths the oracle's ComputePathDerivatives + ConstraintSetup on the same IK rows); a path
//     without a solution has -1;
//   * the waypoint batch, which times the same splines, reports the same records as the path batch.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_cartesian_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_path_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_waypoint_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/time_optimal_path_timing.h"
#include "test_support.h"

using namespace trajectory_planning;

template <class T>
static bool Same(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

static const size_t kPaths = 16;
static const double kTimeStart = 0.5;

static bool SameTiming(const BatchTimingResult &a, const BatchTimingResult &b) {
  return Same(a.status, b.status) && Same(a.last_extremal_index, b.last_extremal_index) &&
         Same(a.samples_per_path, b.samples_per_path) && Same(a.dofs_per_path, b.dofs_per_path) &&
         Same(a.sample_offset, b.sample_offset) && Same(a.joint_offset, b.joint_offset) && Same(a.time, b.time) &&
         Same(a.s, b.s) && Same(a.sd, b.sd) && Same(a.sdd, b.sdd) && Same(a.q, b.q) && Same(a.qd, b.qd) &&
         Same(a.qdd, b.qdd);
}
static bool NoCheckFields(const BatchTimingResult &r) {
  return r.violations.empty() && r.worst_sample.empty() && r.worst_row.empty() && r.worst_excess.empty();
}
static bool CheckFieldsSized(const BatchTimingResult &r, size_t B) {
  return r.violations.size() == B && r.worst_sample.size() == B && r.worst_row.size() == B && r.worst_excess.size() == B;
}

// SolutionSatisfiesConstraints of the mirror's own profile on `rows`; -1 if it has no solution
static int MirrorSatisfied(const std::vector<TimeOptimalPathProfile::Constraint> &rows, int N, int C, double s_end,
                           double sd_start) {
  TimeOptimalPathProfile opt;
  if (!opt.InitSolver(N, C)) return -1;
  opt.SetMaxNumSolverLoops(std::max(100, 10 * N));
  if (!opt.SetupProblem(rows, 0.0, s_end, sd_start, 0.0, kTimeStart)) return -1;
  if (!opt.OptimizePathParameter()) return -1;
  return opt.SolutionSatisfiesConstraints().ok() ? 1 : 0;
}

// violations against the mirror's answer, path by path; returns the number of paths with violated rows
static int Compare(const char *what, const BatchTimingResult &r, const std::vector<int> &satisfied) {
  int solved = 0, violated = 0;
  for (size_t b = 0; b < satisfied.size(); b++) {
    if (r.status[b] != 0) {
      CHECK(r.violations[b] == -1 && r.worst_sample[b] == -1 && r.worst_row[b] == -1 && std::isnan(r.worst_excess[b]));
      CHECK(satisfied[b] == -1);
      continue;
    }
    solved++;
    CHECK(satisfied[b] != -1);
    CHECK(r.violations[b] >= 0);
    CHECK((r.violations[b] == 0) == (satisfied[b] == 1));
    CHECK(r.worst_sample[b] >= 0 && r.worst_sample[b] < r.samples_per_path[b]);
    CHECK(r.worst_row[b] >= 0);
    // a violated row exceeds its bound by more than kTiny; without one no row does
    CHECK((r.worst_excess[b] > 2.220446049250313e-11) == (r.violations[b] > 0));
    violated += r.violations[b] > 0;
  }
  std::printf("%s: %d of %zu paths solved, %d of them with violated rows\n", what, solved, satisfied.size(), violated);
  return violated;
}

static void RunShape(size_t D, size_t N, size_t W, unsigned long long seed) {
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  char name[96];
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths;
  BatchWaypointTiming wt;
  std::vector<CartesianPathSamples> cart(kPaths);
  std::vector<int> joint_ok(kPaths), cart_ok(kPaths);
  for (size_t b = 0; b < kPaths; b++) {
    std::vector<VectorXd> wps;
    for (size_t w = 0; w < W; w++) {
      VectorXd q(D);
      for (size_t d = 0; d < D; d++) q[d] = 4.0 * rnd() - 2.0;
      wps.push_back(q);
    }
    std::vector<double> vmax(D), amax(D);
    for (size_t d = 0; d < D; d++) { vmax[d] = 1.0 + rnd(); amax[d] = 2.0 + 2.0 * rnd(); }
    auto options = [&](double delta) {
      return JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_rounding(0.2).set_constraint_safety(0.8)
          .set_delta_parameter(delta);
    };
    TimeableJointSplinePath probe(options(0.01));
    CHECK(probe.SetWaypoints({wps.data(), wps.size()}).ok());
    const double delta = probe.knots().back() / (double)(N - 1);
    auto p = std::make_shared<TimeableJointSplinePath>(options(delta));
    CHECK(p->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
    CHECK(p->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
    CHECK(p->SetWaypoints({wps.data(), wps.size()}).ok());
    paths.push_back(p);
    CHECK(wt.AddPath(wps, options(delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
    // the mirror's own profile on the joint path's constraints
    CHECK(p->SamplePath(0.0).ok());
    CHECK(p->ConstraintSetup().ok());
    joint_ok[b] = MirrorSatisfied(p->GetConstraints(), (int)N, (int)(2 * D), delta * (double)(N - 1), 0.0);
    // a Cartesian path on the same joint positions
    CartesianPathSamples &c = cart[b];
    for (size_t i = 0; i < N; i++) c.ik_positions.push_back(p->GetPathPositionAt(i));
    c.jacobian = [D](const VectorXd &q, double *J) {
      for (size_t r = 0; r < 6; r++)
        for (size_t d = 0; d < D; d++)
          J[r * D + d] = 0.25 * std::sin(q[d] * (r + 1.0) + 0.37 * d) + ((r == d % 6) ? 1.0 : 0.0);
      return ::tpamd::compat::OkStatus();
    };
    c.max_joint_velocity = VectorXd(D);
    c.max_joint_acceleration = VectorXd(D);
    for (size_t d = 0; d < D; d++) { c.max_joint_velocity[d] = vmax[d]; c.max_joint_acceleration[d] = amax[d]; }
    c.max_translational_velocity = 0.6 + 0.9 * rnd();
    c.max_rotational_velocity = 0.8 + 1.2 * rnd();
    c.delta_parameter = delta;
    {
      const size_t C = 2 * D + 2;
      std::vector<double> q(N * D), J(N * 6 * D), q1(N * D), q2(N * D), jq1(N * 6), A(N * C), Bm(N * C), lo(N * C), hi(N * C);
      for (size_t i = 0; i < N; i++) {
        for (size_t d = 0; d < D; d++) q[i * D + d] = c.ik_positions[i][d];
        CHECK(c.jacobian(c.ik_positions[i], &J[i * 6 * D]).ok());
      }
      tpo_cartesian_path_derivatives(q.data(), (int)N, (int)D, delta, q1.data(), q2.data());
      tpo_cartesian_jacobian_times_q1(J.data(), q1.data(), (int)N, (int)D, jq1.data());
      tpo_cartesian_constraint_setup(q1.data(), q2.data(), jq1.data(), (int)N, (int)D, vmax.data(), amax.data(),
                                     c.max_translational_velocity, c.max_rotational_velocity, 0.8, A.data(), Bm.data(),
                                     lo.data(), hi.data());
      std::vector<TimeOptimalPathProfile::Constraint> rows(N);
      for (size_t i = 0; i < N; i++) {
        rows[i].resize((int)C);
        for (size_t k = 0; k < C; k++) {
          rows[i].a_coefficient((int)k) = A[i * C + k]; rows[i].b_coefficient((int)k) = Bm[i * C + k];
          rows[i].lower((int)k) = lo[i * C + k]; rows[i].upper((int)k) = hi[i * C + k];
        }
      }
      cart_ok[b] = MirrorSatisfied(rows, (int)N, (int)C, delta * (double)(N - 1), 0.0);
    }
  }

  BatchTimingResult off, on;
  BatchPathTiming pt;
  CHECK(pt.SetPaths(paths).ok());
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &off).ok());
  pt.CheckSolutions();
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &on).ok());
  CHECK(NoCheckFields(off) && CheckFieldsSized(on, kPaths) && SameTiming(off, on));
  std::snprintf(name, sizeof name, "BatchPathTiming (%zu, %zu, %zu)", D, N, W);
  const int joint_violated = Compare(name, on, joint_ok);
  pt.CheckSolutions(false);
  BatchTimingResult again;
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &again).ok());
  CHECK(NoCheckFields(again) && SameTiming(off, again));

  BatchTimingResult woff, won;
  wt.CoverWholePath(true);
  CHECK(wt.ComputeTimingProfiles(kTimeStart, &woff).ok());
  wt.CheckSolutions();
  CHECK(wt.ComputeTimingProfiles(kTimeStart, &won).ok());
  CHECK(NoCheckFields(woff) && CheckFieldsSized(won, kPaths) && SameTiming(woff, won));
  CHECK(SameTiming(on, won));                      // the same splines, the same solutions
  std::snprintf(name, sizeof name, "BatchWaypointTiming (%zu, %zu, %zu)", D, N, W);
  CHECK(Compare(name, won, joint_ok) == joint_violated);
  CHECK(Same(on.violations, won.violations) && Same(on.worst_sample, won.worst_sample) &&
        Same(on.worst_row, won.worst_row) && Same(on.worst_excess, won.worst_excess));

  BatchTimingResult coff, con;
  BatchCartesianTiming ct;
  CHECK(ct.SetPaths(cart).ok());
  CHECK(ct.ComputeTimingProfiles(kTimeStart, &coff).ok());
  const int calls = ct.EngineCallsOfLastCompute();
  ct.CheckSolutions();
  CHECK(ct.ComputeTimingProfiles(kTimeStart, &con).ok());
  CHECK(ct.EngineCallsOfLastCompute() == calls);
  CHECK(NoCheckFields(coff) && CheckFieldsSized(con, kPaths) && SameTiming(coff, con));
  std::snprintf(name, sizeof name, "BatchCartesianTiming (%zu, %zu, %zu)", D, N, W);
  Compare(name, con, cart_ok);
}

int main() {
  RunShape(7, 65, 4, 20261);
  RunShape(16, 33, 3, 20262);
  if (g_fail == 0) std::printf("ALL OK\n");
  return g_fail ? 1 : 0;
}

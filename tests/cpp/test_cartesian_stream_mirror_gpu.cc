// GPU test of streaming IK tables through the host mirror (run by tests/test_gpu_cartesian_stream.py):
// a PathTimingTrajectorySet loaded through SetCartesianPaths(paths, streaming) and planned with
// PlanStreaming equals one mirror PathTimingTrajectory per planner planning the same path window by
// window through the unchanged SamplePath, bit for bit at every step -- with an IK callback whose
// result depends on the split into calls (q_i = joint_target_i + 1e-3 sin(seed)). A whole-table set
// built with the same callback (BuildIkTable: one call over the whole path) is shown to DIFFER: the
// streaming route does on the device what the reference's lazy extension does on the host, and the
// whole-table caveat is what it removes.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/engine_handle.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_cartesian_spline.h"

#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::AngleAxisd;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Matrix6Xd;
using tpamd::compat::Milliseconds;
using tpamd::compat::Pose3d;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using tpamd::compat::Vector3d;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static const int D = 7, N = 64;
static int g_ik_calls = 0;

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

// An IK whose result depends on how the samples were split into calls, as a warm-started solver's
// does: q_i = joint_target_i + 1e-3 sin(seed), the call's seed applied to all of its rows.
static Status SeededIk(const VectorXd &seed, const std::vector<Pose3d> &poses, const std::vector<VectorXd> &joints,
                       std::vector<VectorXd> *result) {
  g_ik_calls++;
  result->clear();
  for (size_t i = 0; i < poses.size(); i++) {
    VectorXd q(D);
    for (int d = 0; d < D; d++) q[d] = joints[i][d] + 1e-3 * std::sin(seed[d]);
    result->push_back(q);
  }
  return tpamd::compat::OkStatus();
}
static Status FakeJacobian(const VectorXd &q, Matrix6Xd *J) {
  for (int r = 0; r < 6; r++)
    for (int d = 0; d < D; d++) (*J)(r, d) = 0.2 * std::sin(q[d] * (r + 1.0) + 0.31 * d) + (r == d ? 1.0 : 0.0);
  return tpamd::compat::OkStatus();
}
static Pose3d MakePose(double x, double y, double z, double ax, double ay, double az, double angle) {
  AngleAxisd aa;
  const double n = std::sqrt(ax * ax + ay * ay + az * az);
  aa.axis = Vector3d(ax / n, ay / n, az / n);
  aa.angle = angle;
  return Pose3d(aa.toQuaternion(), Vector3d(x, y, z));
}

static std::vector<Pose3d> Shape(int k) {
  if (k == 0)   // test_host_api.cc:656-657
    return {MakePose(0.3, 0.0, 0.4, 0, 0, 1, 0.1), MakePose(0.5, 0.25, 0.6, 0, 1, 0, 0.7),
            MakePose(0.2, 0.5, 0.3, 1, 0, 0, 0.4), MakePose(0.45, 0.1, 0.5, 0, 0, 1, 1.0)};
  if (k == 1)
    return {MakePose(0.1, 0.2, 0.3, 1, 1, 0, 0.3), MakePose(0.4, 0.2, 0.35, 0, 1, 1, 0.5), MakePose(0.4, 0.5, 0.6, 1, 0, 1, 0.2)};
  return {MakePose(0.6, -0.1, 0.2, 0, 0, 1, 0.8), MakePose(0.3, 0.1, 0.4, 0, 1, 0, 0.2), MakePose(0.5, 0.4, 0.5, 1, 0, 0, 0.6),
          MakePose(0.2, 0.3, 0.7, 0, 1, 1, 0.9), MakePose(0.1, 0.0, 0.4, 1, 1, 1, 0.3)};
}
static std::vector<VectorXd> JointsOf(const std::vector<Pose3d> &poses) {
  std::vector<VectorXd> joints;
  for (size_t i = 0; i < poses.size(); i++) {
    VectorXd q(D);
    for (int d = 0; d < 3; d++) q[d] = poses[i].translation()[d];
    const AngleAxisd aa(poses[i].quaternion());
    for (int d = 0; d < 3; d++) q[3 + d] = aa.axis[d] * aa.angle;
    q[6] = 0.2 * (double)i - 0.3;
    joints.push_back(q);
  }
  return joints;
}

static std::shared_ptr<TimeableCartesianSplinePath> MakePath(int shape, double frac) {
  const std::vector<Pose3d> poses = Shape(shape);
  const std::vector<VectorXd> joints = JointsOf(poses);
  CartesianPathOptions probe_opt;
  probe_opt.set_num_dofs(D).set_num_path_samples(N);
  probe_opt.set_path_ik_func(SeededIk).set_jacobian_func(FakeJacobian);
  TimeableCartesianSplinePath probe(probe_opt);
  CHECK(probe.SetWaypoints({poses.data(), poses.size()}, {joints.data(), joints.size()}).ok());
  const double delta = frac * probe.knots().back() / (N - 1);
  CartesianPathOptions opt;
  opt.set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta);
  opt.set_path_ik_func(SeededIk).set_jacobian_func(FakeJacobian);
  auto path = std::make_shared<TimeableCartesianSplinePath>(opt);
  const std::vector<double> vmax = {0.6, 0.5, 0.7, 1.0, 0.9, 1.1, 0.8}, amax = {1.5, 1.2, 1.8, 2.5, 2.0, 3.0, 2.2};
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  CHECK(path->SetMaxCartesianVelocity(0.35 + 0.05 * shape, 0.9).ok());
  CHECK(path->SetWaypoints({poses.data(), poses.size()}, {joints.data(), joints.size()}).ok());
  return path;
}


static void TestStreamingFamily(Method method) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 6;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet set(opt, B, CartesianTableCapacity{(size_t)N}), whole(opt, B, CartesianTableCapacity{(size_t)N});
  CHECK(set.status().ok() && whole.status().ok());
  if (!set.status().ok() || !whole.status().ok()) return;
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> set_paths(B), whole_paths(B), mirror_paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) {
    const double frac = (b % 2) ? 0.25 : 0.4;
    set_paths[b] = MakePath(b / 2, frac);
    whole_paths[b] = MakePath(b / 2, frac);
    mirror_paths[b] = MakePath(b / 2, frac);
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(mirror_paths[b]).ok());
  }
  CHECK(set.SetCartesianPaths(set_paths, /*streaming=*/true).ok());
  CHECK(whole.SetCartesianPaths(whole_paths).ok());
  for (int b = 0; b < B; b++) {
    std::vector<double> q, J;
    CHECK(set.GetIkTable(b, &q, &J).ok() && q.size() == (size_t)N * D);       // rows 0 .. N-1 only
    CHECK(set_paths[b]->GetState() == TimeablePath::State::kNewPath);
  }
  std::vector<int64_t> start(B, 0);
  std::vector<PlannedTrajectory> tr(B), tw(B);
  int plans = 0, compared = 0, reported = 0, suspensions = 0, whole_differs = 0;
  for (int step = 0; step < 300; step++) {
    std::vector<Time> st(B);
    for (int b = 0; b < B; b++) st[b] = FromUnixNanos(start[b]);
    const std::vector<tpamd::compat::Duration> hz(B, Milliseconds(750));
    const auto sd = set.PlanStreaming(st, hz);
    suspensions += set.SuspensionsOfLastPlan();
    const auto sw = whole.Plan(st, hz);
    plans++;
    bool all_done = true;
    for (int b = 0; b < B; b++) {
      const Status ms = mirrors[b]->Plan(st[b], Milliseconds(750));
      CHECK(ms.ok() && sd[b].ok());
      const int bad = CompareOne(set, b, *mirrors[b], nullptr, &tr[b]);
      CHECK(bad == 0);
      if (bad && ++reported <= 10) std::printf("  %s step %d planner %d: differences 0x%x\n", skip ? "skip" : "uniform", step, b, bad);
      compared++;
      // the streamed table is the mirror path's own IK solution, row for row
      std::vector<double> q, J;
      CHECK(set.GetIkTable(b, &q, &J).ok() && SameBits(q, Flatten(set_paths[b]->GetSplineIKPosition())) &&
            SameBits(q, Flatten(mirror_paths[b]->GetSplineIKPosition())));
      if (sw[b].ok() && whole.GetTrajectory(b, &tw[b]).ok())
        whole_differs += !(SameBits(tw[b].time, tr[b].time) && SameBits(tw[b].positions, tr[b].positions));
      else
        whole_differs++;
    }
    for (int b = 0; b < B; b++)
      if (!mirrors[b]->IsTrajectoryAtEnd()) {
        start[b] = std::min<int64_t>(ToUnixNanos(mirrors[b]->GetEndTime()), start[b] + 200 * kMs);
        all_done = false;
      }
    if (all_done) break;
  }
  for (int b = 0; b < B; b++) CHECK(mirrors[b]->IsTrajectoryAtEnd() && set.IsTrajectoryAtEnd(b));
  CHECK(plans > 4 && suspensions >= B);
  CHECK(whole_differs > 0);        // otherwise this test would prove nothing
  std::printf("streaming mirror family (%s): %d Plan calls, %d planner-plans compared, %d suspensions; the whole-table set "
              "differs in %d planner-plans\n", skip ? "skip" : "uniform", plans, compared, suspensions, whole_differs);
}

int main() {
  TestStreamingFamily(Method::kUniformlyInTime);
  TestStreamingFamily(Method::kSkipSamplesCloserThanTimeStep);
  {
    // PlanStreaming on a joint set
    PathTimingTrajectoryOptions opt;
    opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
    PathTimingTrajectorySet joint(opt, 2, 8);
    CHECK(joint.status().ok());
    const auto st = joint.PlanStreaming(FromUnixNanos(0), Milliseconds(750));
    CHECK(st.size() == 2 && st[0].code() == StatusCode::kFailedPrecondition);
    std::printf("PlanStreaming on a joint set: refused\n");
  }
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

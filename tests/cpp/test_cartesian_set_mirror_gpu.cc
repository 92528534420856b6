// GPU test of Cartesian planner sets through the host mirror (run by tests/test_gpu_cartesian_set.py):
//   3. a PathTimingTrajectorySet loaded through SetCartesianPaths with real
//      TimeableCartesianSplinePaths (the closed-form fake IK and Jacobian of test_host_api.cc, its
//      pose and joint waypoints plus two more shapes, two sampling distances each) equals one mirror
//      PathTimingTrajectory per planner planning the same path window by window, at every step, for
//      both sampling methods; BuildIkTable runs the IK callback once, leaves GetState() alone and
//      gives GetSplineIKPosition()
//   7. downstream on that set, against the existing host flows on the downloaded trajectory:
//      GetSetpoints against the mirror planner's Get*AtTime, GetTrajectories against GetTrajectory,
//      GetPathStopParameters against tpamd_fastest_stop_host, StopTrajectoriesBeforeTime against a
//      mirror TrajectoryBuffer's StopBeforeTime, TrajectoryBufferSet::InsertFromPlannerSet against
//      the trajectory
//   8. the joint-only methods return FailedPrecondition on a Cartesian set, the Cartesian ones on a
//      joint set
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
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer_set.h"

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

static const int D = 7, N = 400;
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

// test_host_api.cc:630-647: a pure function of the targets
static Status FakeIk(const VectorXd &, const std::vector<Pose3d> &poses, const std::vector<VectorXd> &joints,
                     std::vector<VectorXd> *result) {
  g_ik_calls++;
  result->clear();
  for (size_t i = 0; i < poses.size(); i++) {
    VectorXd q(D);
    for (int d = 0; d < 3; d++) q[d] = poses[i].translation()[d];
    const AngleAxisd aa(poses[i].quaternion());
    for (int d = 0; d < 3; d++) q[3 + d] = aa.axis[d] * aa.angle;
    q[6] = joints[i][6];
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
  probe_opt.set_path_ik_func(FakeIk).set_jacobian_func(FakeJacobian);
  TimeableCartesianSplinePath probe(probe_opt);
  CHECK(probe.SetWaypoints({poses.data(), poses.size()}, {joints.data(), joints.size()}).ok());
  const double delta = frac * probe.knots().back() / (N - 1);
  CartesianPathOptions opt;
  opt.set_num_dofs(D).set_num_path_samples(N).set_delta_parameter(delta);
  opt.set_path_ik_func(FakeIk).set_jacobian_func(FakeJacobian);
  auto path = std::make_shared<TimeableCartesianSplinePath>(opt);
  const std::vector<double> vmax = {0.6, 0.5, 0.7, 1.0, 0.9, 1.1, 0.8}, amax = {1.5, 1.2, 1.8, 2.5, 2.0, 3.0, 2.2};
  CHECK(path->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
  CHECK(path->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
  CHECK(path->SetMaxCartesianVelocity(0.35 + 0.05 * shape, 0.9).ok());
  CHECK(path->SetWaypoints({poses.data(), poses.size()}, {joints.data(), joints.size()}).ok());
  return path;
}

// test 7 on the set as it stands after a Plan
static void Downstream(const PathTimingTrajectorySet &set, const std::vector<std::unique_ptr<PathTimingTrajectory>> &mirrors,
                       const std::vector<PlannedTrajectory> &tr, const std::vector<int64_t> &start, int round,
                       long *ticks_ok, long *stops_ok, long *params_ok, long *inserted) {
  const int B = (int)tr.size();
  std::vector<size_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  // the packed download against the one-planner download
  std::vector<PlannedTrajectory> packed;
  CHECK(set.GetTrajectories(all, &packed).ok() && packed.size() == (size_t)B);
  for (int b = 0; b < B && packed.size() == (size_t)B; b++)
    CHECK(SameBits(packed[b].time, tr[b].time) && SameBits(packed[b].positions, tr[b].positions) &&
          SameBits(packed[b].velocities, tr[b].velocities) && SameBits(packed[b].accelerations, tr[b].accelerations) &&
          SameBits(packed[b].path_parameter, tr[b].path_parameter));
  // setpoints at control ticks: from before the first sample, past the last
  const int T = 40;
  std::vector<Time> starts(B);
  std::vector<int64_t> s0(B);
  for (int b = 0; b < B; b++) {
    const int64_t last = (int64_t)llround(tr[b].time.back() * 1e9);
    s0[b] = (b + round) % 3 == 0 ? start[b] - 5 * kMs : ((b + round) % 3 == 1 ? start[b] + 13 * kMs : last - 30 * kMs);
    starts[b] = FromUnixNanos(s0[b]);
  }
  const auto step = tpamd::compat::Nanoseconds(kMs + 1);
  TrajectorySetpoints sp;
  CHECK(set.GetSetpoints(all, starts, step, T, &sp).ok());
  if (sp.status.size() == (size_t)B * T)
    for (int b = 0; b < B; b++)
      for (int j = 0; j < T; j++) {
        const int64_t ns = s0[b] + j * step.nanos();
        const TrajectoryPlanner &R = *mirrors[b];
        const auto wq = R.GetPositionAtTime(FromUnixNanos(ns)), wqd = R.GetVelocityAtTime(FromUnixNanos(ns)),
                   wqdd = R.GetAccelerationAtTime(FromUnixNanos(ns));
        const size_t i = (size_t)b * T + j;
        const int got = Code(sp.status[i]);
        CHECK(got == Code(wq.status()) && got == Code(wqd.status()) && got == Code(wqdd.status()));
        if (got == TPAMD_PLAN_OK && wq.ok() && wqd.ok() && wqdd.ok()) {
          CHECK(SameBits(sp.positions.data() + i * D, (*wq).data(), D) && SameBits(sp.velocities.data() + i * D, (*wqd).data(), D) &&
                SameBits(sp.accelerations.data() + i * D, (*wqdd).data(), D));
          (*ticks_ok)++;
        }
      }
  // the fastest-stop parameter against tpamd_fastest_stop_host on the downloaded trajectory
  std::vector<Time> qt(B);
  for (int b = 0; b < B; b++) qt[b] = FromUnixNanos(start[b] + (30 + 17 * b) * kMs);
  const auto stop = set.GetPathStopParameters(qt);
  CHECK(stop.size() == (size_t)B);
  {
    tpamd::EngineLease lease = tpamd::acquire_engine();
    CHECK((bool)lease);
    for (int b = 0; b < B && lease && stop.size() == (size_t)B; b++) {
      const PlannedTrajectory &p = tr[b];
      const std::vector<double> amax = {1.5, 1.2, 1.8, 2.5, 2.0, 3.0, 2.2};
      const double query = (double)ToUnixNanos(qt[b]) / 1e9;
      double sp_out = -1, dur = -1;
      int32_t idx = -1, st = -1;
      tpamd_fastest_stop_args a{};
      a.num_paths = 1; a.stride = (int32_t)p.time.size(); a.num_dofs = D;
      a.time = p.time.data(); a.s = p.path_parameter.data(); a.qd = p.velocities.data(); a.qdd = p.accelerations.data();
      a.max_acceleration = amax.data(); a.query_time = &query;
      a.stop_parameter = &sp_out; a.stop_index = &idx; a.duration = &dur; a.status = &st;
      CHECK(tpamd_fastest_stop_host(lease.get(), &a) == 0);
      CHECK(Code(stop[b].status()) == st);
      if (stop[b].ok() && st == TPAMD_PLAN_OK) {
        const double got = *stop[b];
        CHECK(SameBits(&got, &sp_out, 1));
        (*params_ok)++;
      }
    }
  }
  // stopping trajectories against a mirror TrajectoryBuffer
  std::vector<VectorXd> am(B, VectorXd(std::vector<double>{1.5, 1.2, 1.8, 2.5, 2.0, 3.0, 2.2}.data(), D));
  std::vector<StoppingSegment> segs;
  CHECK(set.StopTrajectoriesBeforeTime(all, qt, am, 1e-3, &segs).ok());
  for (int b = 0; b < B && segs.size() == (size_t)B; b++) {
    const PlannedTrajectory &p = tr[b];
    const int n = (int)p.time.size();
    std::vector<VectorXd> Q(n), V(n), A(n);
    for (int i = 0; i < n; i++) {
      Q[i] = VectorXd(p.positions.data() + (size_t)i * D, D);
      V[i] = VectorXd(p.velocities.data() + (size_t)i * D, D);
      A[i] = VectorXd(p.accelerations.data() + (size_t)i * D, D);
    }
    auto buf = *TrajectoryBuffer::Create();
    CHECK(buf->InsertSegment(Span<const double>(p.time.data(), n), Span<const VectorXd>(Q.data(), n),
                             Span<const VectorXd>(V.data(), n), Span<const VectorXd>(A.data(), n)).ok());
    const int ms = Code(buf->StopBeforeTime((double)ToUnixNanos(qt[b]) / 1e9, am[b], 1e-3));
    const StoppingSegment &s = segs[b];
    CHECK(Code(s.status) == ms);
    const size_t keep = s.keep, seg = s.time.size();
    CHECK(keep + seg == buf->GetNumSamples());
    if (keep + seg != buf->GetNumSamples()) continue;
    bool same = true;
    for (size_t i = 0; i < keep + seg; i++) {
      const double *t = i < keep ? &p.time[i] : &s.time[i - keep];
      const double *q = i < keep ? &p.positions[i * D] : &s.positions[(i - keep) * D];
      const double *v = i < keep ? &p.velocities[i * D] : &s.velocities[(i - keep) * D];
      const double *a = i < keep ? &p.accelerations[i * D] : &s.accelerations[(i - keep) * D];
      same = same && SameBits(t, &buf->GetTimes()[i], 1) && SameBits(q, buf->GetPositions()[i].data(), D) &&
             SameBits(v, buf->GetVelocities()[i].data(), D) && SameBits(a, buf->GetAccelerations()[i].data(), D);
    }
    CHECK(same);
    if (ms == TPAMD_PLAN_OK && same) (*stops_ok)++;
  }
  // a buffer set fed by the planner set, device to device
  {
    TrajectoryBufferSet bufs(set, B, D);
    CHECK(bufs.status().ok());
    const auto st = bufs.InsertFromPlannerSet(set, all, all);
    std::vector<SampledTrajectory> got;
    CHECK(bufs.GetSamples(all, &got).ok() && got.size() == (size_t)B);
    for (int b = 0; b < B && got.size() == (size_t)B && st.size() == (size_t)B; b++) {
      CHECK(st[b].ok());
      const bool same = SameBits(got[b].times, tr[b].time) && SameBits(Flatten(got[b].positions), tr[b].positions) &&
                        SameBits(Flatten(got[b].velocities), tr[b].velocities) &&
                        SameBits(Flatten(got[b].accelerations), tr[b].accelerations);
      CHECK(same);
      (*inserted) += same;
    }
  }
}

static void TestMirrorFamily(Method method) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 6;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(method);
  PathTimingTrajectorySet set(opt, B, CartesianTableCapacity{(size_t)N});
  CHECK(set.status().ok() && set.is_cartesian());
  if (!set.status().ok()) return;
  std::vector<std::shared_ptr<TimeableCartesianSplinePath>> set_paths(B), mirror_paths(B);
  std::vector<std::unique_ptr<PathTimingTrajectory>> mirrors(B);
  for (int b = 0; b < B; b++) {
    const double frac = (b % 2) ? 0.25 : 0.4;
    set_paths[b] = MakePath(b / 2, frac);
    mirror_paths[b] = MakePath(b / 2, frac);
    mirrors[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(mirrors[b]->SetPath(mirror_paths[b]).ok());
  }
  // BuildIkTable: one IK call, the state stays, the table is GetSplineIKPosition()
  {
    const int calls = g_ik_calls;
    std::vector<double> q, J;
    CHECK(set_paths[0]->GetState() == TimeablePath::State::kNewPath);
    CHECK(set_paths[0]->BuildIkTable(&q, &J).ok());
    CHECK(g_ik_calls == calls + 1);
    CHECK(set_paths[0]->GetState() == TimeablePath::State::kNewPath);
    const auto &table = set_paths[0]->GetSplineIKPosition();
    CHECK((int)table.size() == set_paths[0]->PathIkIndex(set_paths[0]->knots().back()) + N + 1);
    CHECK(SameBits(q, Flatten(table)) && J.size() == q.size() * 6);
  }
  CHECK(set.SetCartesianPaths(set_paths).ok());
  {
    std::vector<double> q, J;
    CHECK(set.GetIkTable(1, &q, &J).ok());
    CHECK(SameBits(q, Flatten(set_paths[1]->GetSplineIKPosition())));
  }
  // 8. the joint-only methods on this set
  {
    std::vector<double> k, c;
    CHECK(set.GetPath(0, &k, &c).code() == StatusCode::kFailedPrecondition);
    TimeableJointSplinePath jp(JointPathOptions().set_num_dofs(D).set_num_path_samples(N));
    CHECK(set.SetPath(0, jp).code() == StatusCode::kFailedPrecondition);
    CHECK(set.SetPaths({}).code() == StatusCode::kFailedPrecondition);
    const auto s1 = set.SetWaypointPaths({0}, {{VectorXd(D, 0.0), VectorXd(D, 1.0)}}, {VectorXd(D, 1.0)}, {VectorXd(D, 1.0)}, {});
    CHECK(s1.size() == 1 && s1[0].code() == StatusCode::kFailedPrecondition);
    const auto s2 = set.SwitchToWaypointPaths({0}, {FromUnixNanos(0)}, {{VectorXd(D, 0.0)}});
    CHECK(s2.size() == 1 && s2[0].code() == StatusCode::kFailedPrecondition);
  }
  std::vector<int64_t> start(B, 0);
  std::vector<PlannedTrajectory> tr(B);
  int plans = 0, compared = 0, reported = 0;
  long ticks_ok = 0, stops_ok = 0, params_ok = 0, inserted = 0;
  for (int step = 0; step < 120; step++) {
    std::vector<Time> st(B);
    for (int b = 0; b < B; b++) st[b] = FromUnixNanos(start[b]);
    const auto sd = set.Plan(st, std::vector<tpamd::compat::Duration>(B, Milliseconds(750)));
    plans++;
    bool all_done = true;
    for (int b = 0; b < B; b++) {
      const Status ms = mirrors[b]->Plan(st[b], Milliseconds(750));
      CHECK(ms.ok() && sd[b].ok());
      const int bad = CompareOne(set, b, *mirrors[b], nullptr, &tr[b]);
      CHECK(bad == 0);
      if (bad && ++reported <= 10) std::printf("  %s step %d planner %d: differences 0x%x\n", skip ? "skip" : "uniform", step, b, bad);
      compared++;
    }
    if (step % 4 == 1) Downstream(set, mirrors, tr, start, step, &ticks_ok, &stops_ok, &params_ok, &inserted);
    for (int b = 0; b < B; b++)
      if (!mirrors[b]->IsTrajectoryAtEnd()) {
        start[b] = std::min<int64_t>(ToUnixNanos(mirrors[b]->GetEndTime()), start[b] + 200 * kMs);
        all_done = false;
      }
    if (all_done) break;
  }
  for (int b = 0; b < B; b++) CHECK(mirrors[b]->IsTrajectoryAtEnd() && set.IsTrajectoryAtEnd(b));
  CHECK(plans > 4 && ticks_ok > 100 && stops_ok > 5 && params_ok > 5 && inserted > 5);
  std::printf("mirror family (%s): %d Plan calls, %d planner-plans compared; downstream: %ld ticks, %ld stops, %ld stop "
              "parameters, %ld buffers\n", skip ? "skip" : "uniform", plans, compared, ticks_ok, stops_ok, params_ok, inserted);
}

// 8. the Cartesian methods on a joint set
static void TestJointSetRefusesTables() {
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(N).SetTimeStep(Milliseconds(4));
  PathTimingTrajectorySet set(opt, 2, 8);
  CHECK(set.status().ok() && !set.is_cartesian());
  if (!set.status().ok()) return;
  auto path = MakePath(0, 0.4);
  CHECK(set.SetCartesianPath(0, *path).code() == StatusCode::kFailedPrecondition);
  CHECK(set.SetCartesianPaths({path}).code() == StatusCode::kFailedPrecondition);
  CHECK(set.SetIkTables({0}, IkTables{}).code() == StatusCode::kFailedPrecondition);
  std::vector<double> q, J;
  CHECK(set.GetIkTable(0, &q, &J).code() == StatusCode::kFailedPrecondition);
  std::printf("Cartesian methods on a joint set: refused\n");
}

int main() {
  TestMirrorFamily(Method::kUniformlyInTime);
  TestMirrorFamily(Method::kSkipSamplesCloserThanTimeStep);
  TestJointSetRefusesTables();
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

// GPU test of moving planners between sets through the C++ mirror (run by
// tests/test_gpu_set_state_mirror.py): PathTimingTrajectorySet::ExportPlanners / ImportPlanners /
// CopyPlanners. For D = 3 and 7 and both sampling methods (N = 65, delta 0.01, 12 planners, 2-5
// waypoints each) every planner of a set is followed by one host PathTimingTrajectory given the
// same waypoints and Plans. After three Plans the planners move
//   1. into a set of other capacities (14 planners, 4 control points to start with) in reversed
//      order through ExportPlanners + ImportPlanners,
//   2. into a third set through CopyPlanners,
//   3. onto themselves, rotated by five, through CopyPlanners(dst == src),
// and in each case the receiver's getters answer from the records at once (summary refreshed
// without a Plan), equal to the host planners', and three more Plans of the receiver stay bit-equal
// to the host planners continuing on the host: summaries, trajectories and resident splines. The
// refused calls (a planner listed twice or out of range, a blob that does not match, a set of
// another shape) change nothing.
// The bridge from the reference-named class (host/planner_state.h, AdoptPlanner / ReleasePlanner):
//   4. a host PathTimingTrajectory plans three steps; PlannerStateFromHost of it equals, byte for
//      byte, the record the device exports for a set planner that was given the same calls;
//      AdoptPlanner takes it into another set, whose export gives the same bytes again, and that
//      set continues three steps bit-equal to a twin host planner continuing on the host;
//   5. ReleasePlanner hands the planner to a fresh host PathTimingTrajectory (the slot is reset),
//      which continues three steps bit-equal to the twin, down to equal records at the end.
// Prints "ALL OK" when everything holds.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/planner_state.h"
#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_state.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

#define TEST_SUPPORT_MIRROR
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::FromUnixNanos;
using tpamd::compat::Milliseconds;
using tpamd::compat::Nanoseconds;
using tpamd::compat::StatusCode;
using tpamd::compat::ToUnixNanos;
using Method = PathTimingTrajectoryOptions::TimeSamplingMethod;

static VectorXd RandomVec(int D, double lo, double hi) {
  VectorXd v(D);
  for (int d = 0; d < D; d++) v[d] = lo + (hi - lo) * Rnd();
  return v;
}

// planner `slot` of the set against the host planner: getters, trajectory and resident spline
static int CompareOne(const PathTimingTrajectorySet &set, size_t slot, const PathTimingTrajectory &m,
                      const TimeableJointSplinePath &path) {
  int bad = 0;
  if (set.GetNumTimeSamples(slot) != m.GetNumTimeSamples()) return 1;
  bad |= (ToUnixNanos(set.GetEndTime(slot)) != ToUnixNanos(m.GetEndTime())) << 1;
  bad |= (ToUnixNanos(set.GetStartTime(slot)) != ToUnixNanos(m.GetStartTime())) << 2;
  bad |= (ToUnixNanos(set.GetFinalDecelStart(slot)) != ToUnixNanos(m.GetFinalDecelStart())) << 3;
  bad |= (set.IsTrajectoryAtEnd(slot) != m.IsTrajectoryAtEnd()) << 4;
  PlannedTrajectory t;
  if (!set.GetTrajectory(slot, &t).ok()) return bad | (1 << 5);
  bad |= !SameBits(t.time, m.GetTime()) << 6;
  bad |= !SameBits(t.path_parameter, m.GetPathParameters()) << 7;
  bad |= !SameBits(t.positions, Flatten(m.GetPositions())) << 9;
  bad |= !SameBits(t.velocities, Flatten(m.GetVelocities())) << 10;
  bad |= !SameBits(t.accelerations, Flatten(m.GetAccelerations())) << 11;
  std::vector<double> k, c;
  bad |= !set.GetPath(slot, &k, &c).ok() << 12;
  bad |= (!SameBits(k, path.knots()) || !SameBits(c, path.packed_control_points())) << 13;
  return bad;
}

struct Fleet {
  int B, D;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths;
  std::vector<std::unique_ptr<PathTimingTrajectory>> host;
  std::vector<std::vector<VectorXd>> wps;
  std::vector<VectorXd> vmax, amax;
  std::vector<size_t> all;
};

static const int kN = 65;
static const double kDelta = 0.01, kRounding = 0.2;

// a fleet and a set holding it, planned three times (host planners alongside)
static void MakeFleet(const PathTimingTrajectoryOptions &opt, int B, int D, Fleet *f) {
  f->B = B; f->D = D;
  f->paths.resize(B); f->host.resize(B); f->wps.resize(B); f->vmax.resize(B); f->amax.resize(B);
  for (int b = 0; b < B; b++) {
    f->all.push_back(b);
    f->vmax[b] = RandomVec(D, 1.0, 2.0);
    f->amax[b] = RandomVec(D, 2.0, 5.0);
    const int W = 2 + b % 4;
    for (int i = 0; i < W; i++) f->wps[b].push_back(RandomVec(D, -1.5, 1.5));
    auto path = std::make_shared<TimeableJointSplinePath>(
        JointPathOptions().set_num_dofs(D).set_num_path_samples(kN).set_delta_parameter(kDelta).set_rounding(kRounding));
    CHECK(path->SetWaypoints({f->wps[b].data(), f->wps[b].size()}).ok());
    CHECK(path->SetMaxJointVelocity({f->vmax[b].data(), f->vmax[b].size()}).ok());
    CHECK(path->SetMaxJointAcceleration({f->amax[b].data(), f->amax[b].size()}).ok());
    f->paths[b] = path;
    f->host[b] = std::make_unique<PathTimingTrajectory>(opt);
    CHECK(f->host[b]->SetPath(path).ok());
  }
}

// One Plan of the set (planner slot[b] holds fleet planner b) and of the host planners named in
// `follow`; returns how many planners were compared equal.
static int PlanBoth(PathTimingTrajectorySet *set, const std::vector<size_t> &slot, Fleet *f, int64_t start_ns,
                    bool plan_host) {
  const size_t nset = set->size();
  std::vector<Time> starts(nset, FromUnixNanos(start_ns));
  std::vector<Duration> horizons(nset, Nanoseconds(300 * kMs));
  const auto st = set->Plan(starts, horizons);
  int equal = 0;
  for (int b = 0; b < f->B; b++) {
    if (plan_host) CHECK(f->host[b]->Plan(FromUnixNanos(start_ns), Nanoseconds(300 * kMs)).ok());
    CHECK(st[slot[b]].ok());
    const int bad = CompareOne(*set, slot[b], *f->host[b], *f->paths[b]);
    if (bad) std::printf("  planner %d in slot %zu differs: %#x\n", b, slot[b], bad);
    CHECK(bad == 0);
    equal += bad == 0;
  }
  return equal;
}

static void TestFamily(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  const int B = 12;
  g_seed = 5300 + 17 * D + (skip ? 1 : 0);
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(method);
  int equal = 0;
  for (int route = 0; route < 3; route++) {
    Fleet f;
    MakeFleet(opt, B, D, &f);
    PathTimingTrajectorySet a(opt, B, 16), other(opt, B + 2, 4);
    CHECK(a.status().ok() && other.status().ok());
    if (!a.status().ok() || !other.status().ok()) return;
    for (const auto &x : a.SetWaypointPaths(f.all, f.wps, f.vmax, f.amax, {}, kRounding, kDelta)) CHECK(x.ok());
    int64_t t = 1000 * kMs;
    for (int step = 0; step < 3; step++, t += 60 * kMs) equal += PlanBoth(&a, f.all, &f, t, true);
    // the hand-over
    PathTimingTrajectorySet *to = route == 2 ? &a : &other;
    std::vector<size_t> slot(B);
    for (int b = 0; b < B; b++) slot[b] = route == 2 ? (size_t)((b + 5) % B) : (size_t)(B + 1 - b);
    std::vector<Status> st;
    if (route == 0) {
      PathTimingTrajectorySet::PlannerStateBlob blob;
      CHECK(a.ExportPlanners(f.all, &blob).ok());
      CHECK(blob.offsets.size() == (size_t)B + 1 && blob.bytes.size() == (size_t)blob.offsets[B]);
      for (const auto &x : blob.status) CHECK(x.ok());
      // refused imports change nothing: a planner listed twice, one out of range, a short blob
      std::vector<size_t> twice = slot, outside = slot;
      twice[1] = twice[0];
      outside[2] = B + 2;
      PathTimingTrajectorySet::PlannerStateBlob cut = blob;
      cut.bytes.resize(cut.bytes.size() - 16);
      for (const auto &x : other.ImportPlanners(twice, blob)) CHECK(x.code() == StatusCode::kInvalidArgument);
      for (const auto &x : other.ImportPlanners(outside, blob)) CHECK(x.code() == StatusCode::kInvalidArgument);
      for (const auto &x : other.ImportPlanners(slot, cut)) CHECK(x.code() == StatusCode::kInvalidArgument);
      for (size_t s = 0; s < other.size(); s++) CHECK(other.GetNumTimeSamples(s) == 0);
      st = other.ImportPlanners(slot, blob);
      // export(import(r)) == r through the mirror
      PathTimingTrajectorySet::PlannerStateBlob again;
      CHECK(other.ExportPlanners(slot, &again).ok());
      CHECK(again.offsets == blob.offsets && again.bytes == blob.bytes);
    } else {
      st = PathTimingTrajectorySet::CopyPlanners(to, slot, &a, f.all);
    }
    CHECK(st.size() == (size_t)B);
    for (const auto &x : st) CHECK(x.ok());
    // the getters answer from the records at once
    for (int b = 0; b < B; b++) CHECK(CompareOne(*to, slot[b], *f.host[b], *f.paths[b]) == 0);
    for (int step = 0; step < 3; step++, t += 60 * kMs) equal += PlanBoth(to, slot, &f, t, true);
  }
  // a set of another shape takes nothing
  {
    Fleet f;
    MakeFleet(opt, 2, D, &f);
    PathTimingTrajectoryOptions opt2 = opt;
    opt2.SetNumPathSamples(kN + 1);
    PathTimingTrajectorySet a(opt, 2, 16), wrong(opt2, 2, 16);
    for (const auto &x : a.SetWaypointPaths(f.all, f.wps, f.vmax, f.amax, {}, kRounding, kDelta)) CHECK(x.ok());
    PlanBoth(&a, f.all, &f, 1000 * kMs, true);
    for (const auto &x : PathTimingTrajectorySet::CopyPlanners(&wrong, f.all, &a, f.all))
      CHECK(x.code() == StatusCode::kInvalidArgument);
    PathTimingTrajectorySet::PlannerStateBlob blob;
    CHECK(a.ExportPlanners(f.all, &blob).ok());
    for (const auto &x : wrong.ImportPlanners(f.all, blob)) CHECK(x.code() == StatusCode::kInvalidArgument);
    CHECK(wrong.GetNumTimeSamples(0) == 0 && wrong.GetNumTimeSamples(1) == 0);
  }
  std::printf("set state vs host planners: D %d, %s: %d planner-plans bit-equal over three routes\n", D,
              skip ? "skip" : "uniform", equal);
  CHECK(equal == 3 * 6 * B);
}

// where two records differ: the header byte, or the section and word
static void PrintDifference(const char *what, const std::vector<unsigned char> &a, const std::vector<unsigned char> &b) {
  if (a == b) return;
  std::printf("  %s: records differ (%zu and %zu bytes)", what, a.size(), b.size());
  const size_t n = std::min(a.size(), b.size());
  size_t at = 0;
  while (at < n && a[at] == b[at]) at++;
  if (at < sizeof(tpamd::StateRecordHeader) || a.size() < sizeof(tpamd::StateRecordHeader)) {
    std::printf(", first at header byte %zu\n", at);
    return;
  }
  const tpamd::StateLayout L = tpamd::state_record_layout(tpamd::state_record_header(a.data()));
  int sec = 0;
  for (int s = 0; s < tpamd::kStateSections; s++)
    if (L.off[s] <= at) sec = s;
  double x, y;
  std::memcpy(&x, a.data() + (at & ~(size_t)7), 8);
  std::memcpy(&y, b.data() + (at & ~(size_t)7), 8);
  std::printf(", first in section %d word %zu: %.17g against %.17g\n", sec, (size_t)((at - L.off[sec]) / 8), x, y);
}

static bool HostEqual(const PathTimingTrajectory &a, const PathTimingTrajectory &b) {
  return a.GetNumTimeSamples() == b.GetNumTimeSamples() && ToUnixNanos(a.GetEndTime()) == ToUnixNanos(b.GetEndTime()) &&
         ToUnixNanos(a.GetStartTime()) == ToUnixNanos(b.GetStartTime()) &&
         ToUnixNanos(a.GetFinalDecelStart()) == ToUnixNanos(b.GetFinalDecelStart()) &&
         a.IsTrajectoryAtEnd() == b.IsTrajectoryAtEnd() && SameBits(a.GetTime(), b.GetTime()) &&
         SameBits(a.GetPathParameters(), b.GetPathParameters()) &&
         SameBits(a.GetPathParameterDerivatives(), b.GetPathParameterDerivatives()) &&
         SameBits(a.GetSecondPathParameterDerivatives(), b.GetSecondPathParameterDerivatives()) &&
         SameBits(Flatten(a.GetPositions()), Flatten(b.GetPositions())) &&
         SameBits(Flatten(a.GetVelocities()), Flatten(b.GetVelocities())) &&
         SameBits(Flatten(a.GetAccelerations()), Flatten(b.GetAccelerations()));
}

static void TestBridge(Method method, int D) {
  const bool skip = method == Method::kSkipSamplesCloserThanTimeStep;
  PathTimingTrajectoryOptions opt;
  opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(4)).SetTimeSamplingMethod(method);
  // the host planner and its twin: the same waypoints and limits
  Fleet f, g;
  g_seed = 6100 + 31 * D + (skip ? 1 : 0);
  MakeFleet(opt, 1, D, &f);
  g_seed = 6100 + 31 * D + (skip ? 1 : 0);
  MakeFleet(opt, 1, D, &g);
  PathTimingTrajectory &host = *f.host[0], &twin = *g.host[0];
  PathTimingTrajectorySet same(opt, 3, 16), set(opt, 3, 4);
  CHECK(same.status().ok() && set.status().ok());
  if (!same.status().ok() || !set.status().ok()) return;
  for (const auto &x : same.SetWaypointPaths({2}, {f.wps[0]}, {f.vmax[0]}, {f.amax[0]}, {}, kRounding, kDelta)) CHECK(x.ok());
  int64_t t = 1000 * kMs;
  for (int step = 0; step < 3; step++, t += 60 * kMs) {
    CHECK(host.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs)).ok());
    CHECK(twin.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs)).ok());
    CHECK(same.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs))[2].ok());
  }
  // 4. the host encoder against the device export of a set planner that did the same calls
  std::vector<unsigned char> record;
  CHECK(PlannerStateFromHost(host, &record).ok());
  PathTimingTrajectorySet::PlannerStateBlob blob;
  CHECK(same.ExportPlanners({2}, &blob).ok());
  PrintDifference("host encoder against the device export", record, blob.bytes);
  CHECK(record == blob.bytes);
  CHECK(set.AdoptPlanner(1, host).ok());
  CHECK(HostEqual(host, twin));                       // the host planner is unchanged
  CHECK(set.ExportPlanners({1}, &blob).ok());
  PrintDifference("host encoder against the adopted planner's export", record, blob.bytes);
  CHECK(record == blob.bytes);
  CHECK(CompareOne(set, 1, twin, *g.paths[0]) == 0);  // the getters answer at once
  int equal = 0;
  for (int step = 0; step < 3; step++, t += 60 * kMs) {
    CHECK(twin.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs)).ok());
    CHECK(set.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs))[1].ok());
    const int bad = CompareOne(set, 1, twin, *g.paths[0]);
    if (bad) std::printf("  adopted planner differs at step %d: %#x\n", step, bad);
    CHECK(bad == 0);
    equal += bad == 0;
  }
  // 5. back into a fresh host planner
  PathTimingTrajectory fresh(opt);
  CHECK(set.ReleasePlanner(1, &fresh).ok());
  CHECK(set.GetNumTimeSamples(1) == 0);               // the slot is reset
  CHECK(HostEqual(fresh, twin));
  std::vector<unsigned char> ra, rb;
  CHECK(PlannerStateFromHost(fresh, &ra).ok() && PlannerStateFromHost(twin, &rb).ok());
  PrintDifference("released planner against the twin", ra, rb);
  CHECK(ra == rb);
  for (int step = 0; step < 3; step++, t += 60 * kMs) {
    const Status sa = fresh.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs));
    const Status sb = twin.Plan(FromUnixNanos(t), Nanoseconds(300 * kMs));
    CHECK(sa.ok() && sb.ok());
    const bool ok = HostEqual(fresh, twin);
    CHECK(ok);
    equal += ok;
  }
  CHECK(PlannerStateFromHost(fresh, &ra).ok() && PlannerStateFromHost(twin, &rb).ok());
  PrintDifference("released planner against the twin after three Plans", ra, rb);
  CHECK(ra == rb);
  // refused: options that differ, a slot outside the set
  PathTimingTrajectoryOptions other = opt;
  other.SetNumPathSamples(kN + 2);
  PathTimingTrajectory wrong(other);
  CHECK(set.AdoptPlanner(0, wrong).code() == StatusCode::kInvalidArgument);
  CHECK(set.AdoptPlanner(3, host).code() == StatusCode::kInvalidArgument);
  CHECK(set.ReleasePlanner(0, &wrong).code() == StatusCode::kInvalidArgument);
  CHECK(PlannerStateToHost(record.data(), record.size() - 8, &wrong).code() == StatusCode::kInvalidArgument);
  std::printf("bridge: D %d, %s: record of %zu bytes equal to the device export, %d of 6 continued Plans bit-equal\n", D,
              skip ? "skip" : "uniform", record.size(), equal);
  CHECK(equal == 6);
}

int main() {
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) TestFamily(m, D);
  for (int D : {3, 7})
    for (Method m : {Method::kUniformlyInTime, Method::kSkipSamplesCloserThanTimeStep}) TestBridge(m, D);
  if (g_fail) {
    std::printf("%d check(s) FAILED\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

// GPU test of BatchWaypointTiming (run by tests/test_gpu_batch_waypoint_timing.py): 14 paths with 6
// and 7 joints alternating, 1 .. 9 waypoints, three sample counts, two roundings and two constraint
// safeties, timed by BatchWaypointTiming -- waypoints in, the fit on the device -- and by
// BatchPathTiming fed with TimeableJointSplinePath::SetWaypoints paths of the same waypoints and
// options. Every packed result array must be bit-equal, with the options' delta_parameter and with
// CoverWholePath (where the comparison path gets delta = knots.back() / (N - 1), one division, from a
// probe fit on the host). AddPath rejects a waypoint or a limit of the wrong dimension and leaves the
// batch as it was; a path without waypoints comes back as TPAMD_PATH_NO_WAYPOINTS beside solved paths.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_path_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_waypoint_timing.h"
#include "test_support.h"

using namespace trajectory_planning;

template <class T>
static bool Same(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Case {
  size_t D, N;
  double rounding, safety, delta;
  std::vector<VectorXd> wps;
  std::vector<double> vmax, amax;
};

static std::vector<Case> MakeCases() {
  unsigned long long seed = 20251;
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  const size_t counts[14] = {2, 9, 1, 3, 5, 2, 7, 4, 3, 6, 2, 8, 5, 3};
  const size_t samples[3] = {200, 64, 333};
  std::vector<Case> cases(14);
  for (size_t b = 0; b < cases.size(); b++) {
    Case &c = cases[b];
    c.D = (b % 2) ? 7 : 6;
    c.N = samples[b % 3];
    c.rounding = (b % 4 == 1) ? 0.0 : 0.2;
    c.safety = (b % 5 == 4) ? 0.6 : 0.8;
    c.delta = 0.004 + 0.004 * rnd();
    for (size_t w = 0; w < counts[b]; w++) {
      VectorXd q(c.D);
      for (size_t d = 0; d < c.D; d++) q[d] = 2.0 * rnd() - 1.0;
      c.wps.push_back(q);
    }
    for (size_t d = 0; d < c.D; d++) {
      c.vmax.push_back(0.5 + 1.5 * rnd());
      c.amax.push_back(0.5 + 1.5 * rnd());
    }
  }
  return cases;
}

static JointPathOptions Options(const Case &c, double delta) {
  return JointPathOptions().set_num_dofs(c.D).set_num_path_samples(c.N).set_rounding(c.rounding)
      .set_constraint_safety(c.safety).set_delta_parameter(delta);
}

static void Compare(const std::vector<Case> &cases, bool whole) {
  BatchWaypointTiming wt;
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths;
  std::vector<double> want_delta, want_end;
  std::vector<int32_t> want_points;
  for (const Case &c : cases) {
    std::vector<double> vmax = c.vmax, amax = c.amax;
    std::vector<VectorXd> wps = c.wps;
    CHECK(wt.AddPath(wps, Options(c, c.delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
    TimeableJointSplinePath probe(Options(c, c.delta));
    CHECK(probe.SetWaypoints({wps.data(), wps.size()}).ok());
    const double end = probe.knots().back();
    const double delta = whole ? end / (double)(c.N - 1) : c.delta;
    auto p = std::make_shared<TimeableJointSplinePath>(Options(c, delta));
    CHECK(p->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
    CHECK(p->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
    CHECK(p->SetWaypoints({wps.data(), wps.size()}).ok());
    paths.push_back(p);
    want_delta.push_back(delta); want_end.push_back(end); want_points.push_back(p->num_control_points());
  }
  wt.CoverWholePath(whole);
  BatchTimingResult a, b;
  CHECK(wt.ComputeTimingProfiles(1.5, &a).ok());
  BatchPathTiming pt;
  CHECK(pt.SetPaths(paths).ok());
  CHECK(pt.ComputeTimingProfiles(1.5, &b).ok());
  int solved = 0;
  for (int32_t s : b.status) solved += s == 0;
  CHECK(solved >= 12);
  CHECK(Same(a.status, b.status));
  CHECK(Same(a.last_extremal_index, b.last_extremal_index));
  CHECK(Same(a.samples_per_path, b.samples_per_path));
  CHECK(Same(a.dofs_per_path, b.dofs_per_path));
  CHECK(Same(a.sample_offset, b.sample_offset));
  CHECK(Same(a.joint_offset, b.joint_offset));
  CHECK(a.num_samples == b.num_samples && a.num_dofs == b.num_dofs);
  CHECK(Same(a.time, b.time)); CHECK(Same(a.s, b.s)); CHECK(Same(a.sd, b.sd)); CHECK(Same(a.sdd, b.sdd));
  CHECK(Same(a.q, b.q)); CHECK(Same(a.qd, b.qd)); CHECK(Same(a.qdd, b.qdd));
  CHECK(Same(wt.delta_used(), want_delta));
  CHECK(Same(wt.path_end(), want_end));
  CHECK(Same(wt.num_control_points(), want_points));
  CHECK(wt.EngineCallsOfLastCompute() == 4);     // 6 and 7 joints, each at safety 0.8 and (paths 4 and 9) 0.6
  std::printf("%s: %d of %zu paths solved, engine calls %d, end time of path 0 %.17g\n",
              whole ? "whole path" : "delta_parameter", solved, cases.size(), wt.EngineCallsOfLastCompute(),
              a.time[a.sample_offset[1] - 1]);
}

int main() {
  const std::vector<Case> cases = MakeCases();
  Compare(cases, false);
  Compare(cases, true);
  {  // what AddPath refuses, and the path without waypoints
    BatchWaypointTiming wt;
    const Case &c = cases[3];
    std::vector<double> vmax = c.vmax, amax = c.amax, shortv(c.D - 1, 1.0);
    std::vector<VectorXd> bad = c.wps;
    bad[1] = VectorXd(c.D + 1, 0.5);
    CHECK(!wt.AddPath(bad, Options(c, c.delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
    CHECK(!wt.AddPath(c.wps, Options(c, c.delta), {shortv.data(), shortv.size()}, {amax.data(), amax.size()}).ok());
    CHECK(!wt.AddPath(c.wps, Options(c, c.delta).set_num_path_samples(2), {vmax.data(), vmax.size()},
                      {amax.data(), amax.size()}).ok());
    CHECK(wt.NumPaths() == 0);
    BatchTimingResult r;
    CHECK(!wt.ComputeTimingProfiles(0.0, &r).ok());
    CHECK(wt.AddPath(c.wps, Options(c, c.delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
    CHECK(wt.AddPath({}, Options(c, c.delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
    CHECK(wt.ComputeTimingProfiles(0.0, &r).ok());
    CHECK(r.status.size() == 2 && r.status[0] == 0 && r.status[1] == TPAMD_PATH_NO_WAYPOINTS);
    CHECK(wt.num_control_points()[1] == 0 && wt.path_end()[1] == 0.0);
  }
  if (g_fail == 0) std::printf("ALL OK\n");
  return g_fail ? 1 : 0;
}

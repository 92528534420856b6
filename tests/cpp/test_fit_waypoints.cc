// CPU test of the planner-set waypoint fit (run by tests/test_fit_waypoints_cpu.py): fit_waypoints of
// csrc/tpamd_fit.h, compiled here for the host, against the mirror's
// TimeableJointSplinePath::SetWaypoints (knots and control points, bit for bit) and the oracle's
// tpo_joint_fit_spline (the C function behind tpo.joint_fit_spline).
//
// Seeded cases for D = 1, 3, 7, 14, 16 and W = 1..40 with rounding 0, the default 0.2, and large
// radii; random waypoints, repeated consecutive waypoints, collinear runs and polygons shorter than
// 0.1 (the minimum final knot). Also: no waypoints is an error on both sides, and the mirror rejects
// a waypoint of the wrong dimension. Prints one line per category and "ALL OK".
// With an argument FILE it also writes a few hundred cases (W, D, rounding, waypoints, knots,
// control points of fit_waypoints) for the Python side to compare with tpo.joint_fit_spline.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_fit.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

#define TEST_SUPPORT_SEED 20261016ULL
#include "test_support.h"

using namespace trajectory_planning;

static std::map<std::string, int> g_seen;
static FILE *g_dump = nullptr;
static int g_dumped = 0;

// Waypoints of one case: kind 0 random, 1 repeated consecutive waypoints, 2 collinear runs,
// 3 a polygon shorter than 0.1, 4 all waypoints equal.
static std::vector<VectorXd> MakeWaypoints(int kind, int W, int D) {
  std::vector<VectorXd> w;
  const double scale = kind == 3 ? 0.1 / (3.0 * W * std::sqrt((double)D)) : 2.5;
  for (int i = 0; i < W; i++) {
    VectorXd v(D);
    for (int d = 0; d < D; d++) v[d] = scale * (2.0 * Rnd() - 1.0);
    if (kind == 1 && i > 0 && Rnd() < 0.4) v = w.back();                       // a repeat
    if (kind == 2 && i >= 2 && Rnd() < 0.7) {                                  // on the line of the last two
      const double t = 0.2 + 1.5 * Rnd();
      for (int d = 0; d < D; d++) v[d] = w[i - 1][d] + t * (w[i - 1][d] - w[i - 2][d]);
    }
    if (kind == 4 && i > 0) v = w.front();
    w.push_back(v);
  }
  return w;
}

static void OneCase(int kind, int W, int D, double rounding, const char *category) {
  const std::vector<VectorXd> wps = MakeWaypoints(kind, W, D);
  std::vector<double> flat;
  for (const auto &w : wps) flat.insert(flat.end(), w.begin(), w.end());
  const int P = tpamd::fit_points(W);
  std::vector<double> k(P + 3, -1.0), c((size_t)P * D, -1.0);
  const int got = tpamd::fit_waypoints(flat.data(), W, D, rounding, k.data(), c.data());
  CHECK(got == P);
  // the mirror
  TimeableJointSplinePath path(JointPathOptions().set_num_dofs(D).set_num_path_samples(3).set_rounding(rounding));
  CHECK(path.SetWaypoints({wps.data(), wps.size()}).ok());
  CHECK(path.num_control_points() == P);
  const bool mirror_same = SameBits(path.knots(), k.data(), (size_t)P + 3) &&
                           SameBits(path.packed_control_points(), c.data(), (size_t)P * D);
  CHECK(mirror_same);
  // the oracle
  std::vector<double> ok(P + 3, -2.0), oc((size_t)P * D, -2.0);
  tpo_joint_fit_spline(flat.data(), W, D, rounding, oc.data(), ok.data());
  const bool oracle_same = std::memcmp(ok.data(), k.data(), ok.size() * 8) == 0 &&
                           std::memcmp(oc.data(), c.data(), oc.size() * 8) == 0;
  CHECK(oracle_same);
  if (!mirror_same || !oracle_same)
    std::printf("  %s: differs (D %d W %d rounding %.17g, mirror %d oracle %d)\n", category, D, W, rounding,
                (int)mirror_same, (int)oracle_same);
  const double last = k[P + 2];
  g_seen[category]++;
  if (last == 0.1) g_seen["final knot 0.1 (polygon shorter than 0.1)"]++;
  if (g_dump && g_dumped < 400 && (W + D + (int)g_seen[category]) % 13 == 0) {
    const int hdr[2] = {W, D};
    std::fwrite(hdr, 4, 2, g_dump);
    std::fwrite(&rounding, 8, 1, g_dump);
    std::fwrite(flat.data(), 8, flat.size(), g_dump);
    std::fwrite(k.data(), 8, k.size(), g_dump);
    std::fwrite(c.data(), 8, c.size(), g_dump);
    g_dumped++;
  }
}

int main(int argc, char **argv) {
  if (argc > 1) g_dump = std::fopen(argv[1], "wb");
  const int dofs[] = {1, 3, 7, 14, 16};
  const double radii[] = {0.0, 0.2, 1.5, 50.0};
  const char *kinds[] = {"random", "repeated waypoints", "collinear runs", "polygon shorter than 0.1",
                         "all waypoints equal"};
  int cases = 0;
  for (int D : dofs) {
    for (int W = 1; W <= 40; W++) {
      for (int kind = 0; kind < 5; kind++) {
        for (double r : radii) {
          std::string cat = std::string(kinds[kind]) + (r == 0.0 ? ", rounding 0" : r == 0.2 ? ", rounding 0.2"
                                                                                         : ", large rounding");
          OneCase(kind, W, D, r, cat.c_str());
          cases++;
        }
        // a seeded radius as well
        OneCase(kind, W, D, 0.5 * Rnd(), kinds[kind]);
        cases++;
      }
    }
  }
  // no waypoints: an error on both sides, nothing written
  for (int D : dofs) {
    double k[4] = {7, 7, 7, 7}, c[2] = {7, 7};
    CHECK(tpamd::fit_waypoints(nullptr, 0, D, 0.2, k, c) == 0);
    CHECK(k[0] == 7 && c[0] == 7);
    TimeableJointSplinePath path(JointPathOptions().set_num_dofs(D).set_num_path_samples(3));
    CHECK(path.SetWaypoints({}).code() == tpamd::compat::StatusCode::kInvalidArgument);
    std::vector<VectorXd> bad = {VectorXd(D + 1)};
    CHECK(path.SetWaypoints({bad.data(), bad.size()}).code() == tpamd::compat::StatusCode::kInvalidArgument);
    g_seen["no waypoints / wrong dimension"]++;
  }
  if (g_dump) std::fclose(g_dump);
  for (const auto &kv : g_seen) std::printf("category %s: %d\n", kv.first.c_str(), kv.second);
  std::printf("fit cases: %d\n", cases);
  std::printf("dumped: %d\n", g_dumped);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

// Stand-alone host program around joint_fit_path (csrc/tpamd_joint_fit.h), the body of
// k_fit_joint_waypoints, run by tests/test_waypoint_batch_cpu.py. It links nothing of the project, so
// it is built with -fsanitize=address,undefined and run directly: every buffer has exactly the size
// its layout needs, and a fit that leaves its slot is an error of the run.
//
// stdin (text, doubles as C99 hex floats):
//   D B S N
//   offsets[B + 1]  point_offsets[B]  knot_offsets[B]  total_points total_knots
//   samples[B]  rounding[B]  delta_in[B]  waypoints[rows * D]
// It fits the batch three times -- packed (the fit entry: every status written, no timing fields),
// strided with the whole-path delta, strided with delta_in -- and prints every array. Buffers start
// as -7 so that the caller sees what was not written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_joint_fit.h"

static double rd() {
  double v = 0;
  if (std::scanf("%la", &v) != 1) std::exit(2);
  return v;
}
static int ri() {
  int v = 0;
  if (std::scanf("%d", &v) != 1) std::exit(2);
  return v;
}
static void pd(const char *name, const std::vector<double> &v) {
  std::printf("%s %zu", name, v.size());
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}
static void pi(const char *name, const std::vector<int32_t> &v) {
  std::printf("%s %zu", name, v.size());
  for (int32_t x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main() {
  const int D = ri(), B = ri(), S = ri(), N = ri();
  std::vector<int32_t> off(B + 1), poff(B), koff(B), ns(B);
  for (auto &x : off) x = ri();
  for (auto &x : poff) x = ri();
  for (auto &x : koff) x = ri();
  const int total_points = ri(), total_knots = ri();
  for (auto &x : ns) x = ri();
  std::vector<double> rounding(B), delta_in(B), wps((size_t)off[B] * D);
  for (auto &x : rounding) x = rd();
  for (auto &x : delta_in) x = rd();
  for (auto &x : wps) x = rd();

  {  // packed, as tpamd_fit_joint_waypoints_* runs it
    std::vector<double> knots(total_knots, -7.0), cps((size_t)total_points * D, -7.0), end(B, -7.0);
    std::vector<int32_t> np(B, -7), status(B, -7);
    tpamd::JointFitParams p{};
    p.Q = B; p.D = D; p.offsets = off.data(); p.wps = wps.data(); p.rounding = rounding.data();
    p.point_offsets = poff.data(); p.knot_offsets = koff.data();
    p.knots = knots.data(); p.cps = cps.data();
    p.num_points = np.data(); p.path_end = end.data(); p.status = status.data();
    p.status_empty = 3; p.status_all = 1;
    for (int k = 0; k < B; k++) tpamd::joint_fit_path(p, k);
    pd("packed_knots", knots); pd("packed_cps", cps); pd("packed_end", end);
    pi("packed_np", np); pi("packed_status", status);
  }
  for (int given = 0; given < 2; given++) {  // strided, as tpamd_time_waypoint_paths_* runs it
    std::vector<double> knots((size_t)B * (S + 3), -7.0), cps((size_t)B * S * D, -7.0), end(B, -7.0), delta(B, -7.0),
        zero(B, -7.0);
    std::vector<int32_t> np(B, -7), status(B, -7), samples(B, -7);
    tpamd::JointFitParams p{};
    p.Q = B; p.D = D; p.offsets = off.data(); p.wps = wps.data();
    p.rounding = given ? rounding.data() : nullptr;          // null: 0.2
    p.p_stride = S; p.knots = knots.data(); p.cps = cps.data();
    p.num_points = np.data(); p.path_end = end.data(); p.status = status.data();
    p.status_empty = 11; p.status_all = 0;
    p.N = N; p.samples_in = given ? ns.data() : nullptr; p.delta_in = given ? delta_in.data() : nullptr;
    p.delta = delta.data(); p.samples = samples.data(); p.zero = zero.data();
    for (int k = 0; k < B; k++) tpamd::joint_fit_path(p, k);
    const char *tag = given ? "given" : "whole";
    char name[64];
#define OUT(fn, what, v) std::snprintf(name, sizeof name, "%s_%s", tag, what), fn(name, v)
    OUT(pd, "knots", knots); OUT(pd, "cps", cps); OUT(pd, "end", end); OUT(pd, "delta", delta); OUT(pd, "zero", zero);
    OUT(pi, "np", np); OUT(pi, "status", status); OUT(pi, "samples", samples);
#undef OUT
  }
  return 0;
}

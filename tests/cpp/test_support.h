// What the stand-alone drivers in this directory share: the failure counter and CHECK, the seeded
// 64-bit LCG their random cases come from, and bit-for-bit comparisons. A driver ends with
//   if (g_fail) { std::printf("%d checks failed\n", g_fail); return 1; }  std::printf("ALL OK\n");
// or its own equivalent; tests/native_driver.py holds the other half of that contract.
//
// Two macros, defined before the include, select what a driver needs:
//   TEST_SUPPORT_SEED    the LCG's first state (default 1); a driver may also assign g_seed later
//   TEST_SUPPORT_MIRROR  also include the host mirror's headers and define Flatten and CompareOne,
//                        for drivers that link libtp_host.so
#ifndef TESTS_CPP_TEST_SUPPORT_H_
#define TESTS_CPP_TEST_SUPPORT_H_

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

// Failed checks are counted without limit; only the first 40 are printed.
__attribute__((unused)) static int g_fail = 0;
#define CHECK(cond)                                                                  \
  do {                                                                               \
    if (!(cond)) {                                                                   \
      if (g_fail < 40) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fail++;                                                                      \
    }                                                                                \
  } while (0)

// Expands where it is used, so it needs the HIP runtime header only in drivers that call it.
#define HIP_OK(expr) CHECK((expr) == hipSuccess)

static const int64_t kMs = 1000000;

#ifndef TEST_SUPPORT_SEED
#define TEST_SUPPORT_SEED 1
#endif
__attribute__((unused)) static unsigned long long g_seed = TEST_SUPPORT_SEED;
static inline double Rnd() {
  g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL;
  return (double)(g_seed >> 11) / 9007199254740992.0;
}
static inline int RndInt(int lo, int hi) { return lo + (int)(Rnd() * (hi - lo + 1)) % (hi - lo + 1); }

static inline bool SameBits(const std::vector<double> &a, const std::vector<double> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * 8) == 0);
}
static inline bool SameBits(const double *a, const double *b, size_t n) { return n == 0 || std::memcmp(a, b, n * 8) == 0; }
static inline bool SameBits(const std::vector<double> &a, const double *b, size_t n) {
  return a.size() == n && (n == 0 || std::memcmp(a.data(), b, n * 8) == 0);
}

#ifdef TEST_SUPPORT_MIRROR
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "../../x-edr-trajectory-planning_amd/host/timeable_path_joint_spline.h"

static inline std::vector<double> Flatten(const std::vector<trajectory_planning::VectorXd> &v) {
  std::vector<double> r;
  for (const auto &x : v) r.insert(r.end(), x.begin(), x.end());
  return r;
}

// Planner b of the set against its mirror: summary and trajectory, bit for bit; with a path, the
// set's resident spline against it as well. Bit k of the result set: check k differs. The
// trajectory read from the set is left in *out where the caller wants it.
static inline int CompareOne(const trajectory_planning::PathTimingTrajectorySet &set, int b,
                             const trajectory_planning::PathTimingTrajectory &m,
                             const trajectory_planning::TimeableJointSplinePath *path = nullptr,
                             trajectory_planning::PlannedTrajectory *out = nullptr) {
  using tpamd::compat::ToUnixNanos;
  trajectory_planning::PlannedTrajectory own;
  trajectory_planning::PlannedTrajectory &t = out ? *out : own;
  int bad = 0;
  if (set.GetNumTimeSamples(b) != m.GetNumTimeSamples()) return 1;
  bad |= (ToUnixNanos(set.GetEndTime(b)) != ToUnixNanos(m.GetEndTime())) << 1;
  bad |= (ToUnixNanos(set.GetStartTime(b)) != ToUnixNanos(m.GetStartTime())) << 2;
  bad |= (ToUnixNanos(set.GetFinalDecelStart(b)) != ToUnixNanos(m.GetFinalDecelStart())) << 3;
  bad |= (set.IsTrajectoryAtEnd(b) != m.IsTrajectoryAtEnd()) << 4;
  if (!set.GetTrajectory(b, &t).ok()) return bad | (1 << 5);
  bad |= !SameBits(t.time, m.GetTime()) << 6;
  bad |= !SameBits(t.path_parameter, m.GetPathParameters()) << 7;
  bad |= !SameBits(t.path_parameter_derivative, m.GetPathParameterDerivatives()) << 8;
  bad |= !SameBits(t.positions, Flatten(m.GetPositions())) << 9;
  bad |= !SameBits(t.velocities, Flatten(m.GetVelocities())) << 10;
  bad |= !SameBits(t.accelerations, Flatten(m.GetAccelerations())) << 11;
  if (path) {
    std::vector<double> k, c;
    bad |= !set.GetPath(b, &k, &c).ok() << 12;
    bad |= (!SameBits(k, path->knots()) || !SameBits(c, path->packed_control_points())) << 13;
  }
  return bad;
}
#endif  // TEST_SUPPORT_MIRROR

#endif  // TESTS_CPP_TEST_SUPPORT_H_

// CPU test of the stopping trajectories (run by tests/test_stop_buffer_cpu.py):
//   1. the mirror's TrajectoryBuffer::StopAtIndex / StopBeforeTime and
//      RescaleTrajectoryBackwardToStop (host/trajectory_buffer.cc, host/rescale_to_stop.cc) on the
//      cases of the reference's tests, restated as data generated here;
//   2. the host/device core of csrc/tpamd_rescale.h, compiled here for the host and composed by
//      rs_stop_serial, against the mirror bit for bit on seeded trajectories: the buffer after the
//      stop (input[0, keep) ++ segment) and the status. Every outcome category must be reached.
// Prints one line per category and "ALL OK".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_rescale.h"
#include "../../x-edr-trajectory-planning_amd/host/rescale_to_stop.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_buffer.h"

#define TEST_SUPPORT_SEED 20261016ULL
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::StatusCode;

static int Code(const Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return tpamd::kRsOk;
    case StatusCode::kFailedPrecondition: return 1;
    case StatusCode::kOutOfRange: return tpamd::kRsOutOfRange;
    case StatusCode::kInvalidArgument: return tpamd::kRsInvalidArgument;
    case StatusCode::kInternal: return tpamd::kRsInternal;
    case StatusCode::kNotFound: return tpamd::kRsNotFound;
    default: return 99;
  }
}

static std::shared_ptr<TrajectoryBuffer> Load(const SampledTrajectory &t) {
  auto b = TrajectoryBuffer::Create();
  CHECK(b.ok());
  auto buf = *b;
  CHECK(buf->InsertSegment(t.times, t.positions, t.velocities, t.accelerations).ok());
  return buf;
}

static VectorXd Constant(int n, double v) { return VectorXd((size_t)n, v); }

// GetQuadraticTestTrajectory of trajectory_buffer_test.cc: q = 0.5 (t - T)^2, v = t - T, a = 1
static SampledTrajectory Quadratic(int sample_count, double dt, int joints) {
  const double final_time = (sample_count - 1) * dt;
  SampledTrajectory t;
  for (int i = 0; i < sample_count; ++i) {
    const double time = dt * i, trel = time - final_time;
    t.times.push_back(time);
    t.positions.push_back(Constant(joints, 0.5 * trel * trel));
    t.velocities.push_back(Constant(joints, trel));
    t.accelerations.push_back(Constant(joints, 1.0));
  }
  return t;
}

static bool AccelerationsWithin(const TrajectoryBuffer &b, double amax) {
  for (const VectorXd &a : b.GetAccelerations())
    for (size_t j = 0; j < a.size(); j++)
      if (!(std::fabs(a[j]) <= amax + 1e-8)) return false;
  return true;
}

static void ReferenceCases() {
  // rescale_to_stop_test.cc SucceedsForConstantVelocity
  for (double velocity : {-1.0, 1.0}) {
    const int n = 200, J = 4;
    const double dt = 8e-3, amax = 2.0;
    SampledTrajectory t;
    for (int i = 0; i < n; ++i) {
      t.times.push_back(i * dt);
      t.positions.push_back(Constant(J, velocity * t.times[i]));
      t.velocities.push_back(Constant(J, velocity));
      t.accelerations.push_back(Constant(J, 0.0));
    }
    const auto r = RescaleTrajectoryBackwardToStop(Constant(J, amax), t.times, t.positions, t.velocities,
                                                   t.accelerations);
    CHECK(r.ok());
    const SampledTrajectory &s = *r;
    CHECK(!s.times.empty() && s.times.size() == s.positions.size() && s.times.size() == s.velocities.size() &&
          s.times.size() == s.accelerations.size());
    if (s.times.empty()) continue;
    CHECK(std::fabs((s.times.back() - s.times.front()) - std::fabs(velocity) / amax) <= dt);
    CHECK(s.velocities.back().maxAbs() == 0.0 && s.accelerations.back().maxAbs() == 0.0);
    const double travel = velocity * velocity / (2.0 * amax) * (velocity < 0 ? -1.0 : 1.0);
    for (int j = 0; j < J; j++)
      CHECK(std::fabs(s.positions.back()[j] - s.positions.front()[j] - travel) <= std::fabs(velocity * dt));
  }
  const int J = 9, n = 1001;
  const double dt = 1e-3;
  const SampledTrajectory quad = Quadratic(n, dt, J);
  {  // StopAtIndexSucceedsIfFeasible
    auto b = Load(quad);
    CHECK(b->StopAtIndex(n / 2, Constant(J, 5.0), dt).ok());
    CHECK(b->GetNumSamples() >= (size_t)(n / 2 + 1));
    CHECK(b->GetVelocities()[b->GetNumSamples() - 1].maxAbs() == 0.0);
    CHECK(AccelerationsWithin(*b, 5.0));
  }
  {  // StopAtIndexFailsIfInfeasible
    auto b = Load(quad);
    CHECK(b->StopAtIndex(2, Constant(J, 1.0), dt).code() == StatusCode::kNotFound);
    CHECK(b->GetNumSamples() == (size_t)n);
  }
  {  // StopBeforeTimeFailsIfInfeasible
    auto b = Load(quad);
    CHECK(b->StopBeforeTime(dt * 2, Constant(J, 1.0), dt).code() == StatusCode::kNotFound);
    CHECK(b->StopBeforeTime(dt * 3.1415, Constant(J, 1.0), dt).code() == StatusCode::kNotFound);
  }
  {  // StopBeforeTimeSucceedsIfFeasible: on a sample, then halfway between two
    auto b = Load(quad);
    const double on = b->GetTimes()[n / 2];
    CHECK(b->StopBeforeTime(on, Constant(J, 5.0), dt).ok());
    CHECK(b->GetNumSamples() >= (size_t)(n / 2 + 1));
    CHECK(b->GetVelocities()[b->GetNumSamples() - 1].maxAbs() == 0.0);
    CHECK(AccelerationsWithin(*b, 5.0));
    b->Clear();
    CHECK(b->InsertSegment(quad.times, quad.positions, quad.velocities, quad.accelerations).ok());
    const double half = 0.5 * (b->GetTimes()[n / 2] + b->GetTimes()[n / 2 + 1]);
    CHECK(b->StopBeforeTime(half, Constant(J, 5.0), dt).ok());
    CHECK(b->GetNumSamples() >= (size_t)(n / 2 + 1));
  }
  {  // StopBeforeTimeSucceedsIfCutoffTimeBeyondFinalTimestep
    SampledTrajectory t;
    for (int i = 0; i < 50; ++i) {
      t.times.push_back(i * 0.01);
      t.positions.push_back(Constant(3, 1.0 * 0.01 * i));
      t.velocities.push_back(Constant(3, 1.0));
      t.accelerations.push_back(Constant(3, 0.0));
    }
    auto b = Load(t);
    CHECK(b->StopBeforeTime(t.times.back() + 12.0, Constant(3, 2.0), 0.01).ok());
    CHECK(b->GetVelocities()[b->GetNumSamples() - 1].maxAbs() == 0.0);
  }
  {  // DetectsErrors: GetTestTrajectory(1.0, 5), v = 10 i, a = 100 i
    auto eb = TrajectoryBuffer::Create();
    auto b = *eb;
    const VectorXd amax = Constant(J, 4.0);
    CHECK(b->StopAtIndex(-1, amax, 8e-3).code() == StatusCode::kOutOfRange);
    CHECK(b->StopAtIndex(0, amax, 8e-3).code() == StatusCode::kOutOfRange);
    SampledTrajectory t;
    for (int i = 0; i < 5; ++i) {
      t.times.push_back(i * 8e-3 + 1.0);
      t.positions.push_back(Constant(J, i));
      t.velocities.push_back(Constant(J, 10.0 * i));
      t.accelerations.push_back(Constant(J, 100.0 * i));
    }
    CHECK(b->InsertSegment(t.times, t.positions, t.velocities, t.accelerations).ok());
    CHECK(b->StopAtIndex(5, amax, 8e-3).code() == StatusCode::kOutOfRange);
    CHECK(b->StopAtIndex(2, amax, -0.1).code() == StatusCode::kInvalidArgument);
    CHECK(b->StopAtIndex(2, Constant(J, 0.0), 8e-3).code() == StatusCode::kInvalidArgument);
    CHECK(b->StopBeforeTime(0.5, amax, 8e-3).code() == StatusCode::kOutOfRange);
    CHECK(b->GetNumSamples() == 5);
    // CreateChecksOptions; an empty buffer stops OK and stays empty
    CHECK(TrajectoryBuffer::Create(TrajectoryBufferOptions{0.0}).status().code() == StatusCode::kFailedPrecondition);
    auto e = *TrajectoryBuffer::Create();
    CHECK(e->StopBeforeTime(1.0, amax, 8e-3).ok() && e->GetNumSamples() == 0);
  }
  {  // the deviation: at rest before the end is InternalError, buffer unchanged
    SampledTrajectory t = Quadratic(20, 1e-2, 2);
    t.velocities[10] = Constant(2, 0.0);
    auto b = Load(t);
    CHECK(b->StopAtIndex(10, Constant(2, 5.0), 1e-2).code() == StatusCode::kInternal);
    CHECK(b->GetNumSamples() == 20 && b->GetVelocities()[10].maxAbs() == 0.0);
  }
  std::printf("reference cases: done\n");
}

// One seeded case: the mirror buffer against rs_stop_serial; returns the category.
static std::string FuzzOne(int c, std::map<std::string, long> *counts) {
  const int dofs[4] = {1, 3, 7, 16};
  const int D = dofs[RndInt(0, 3)];
  int n = RndInt(0, 9) == 0 ? RndInt(0, 2) : RndInt(3, 80);
  // times: regular, jittered, or with steps below the 1e-6 tolerance
  std::vector<double> t(n);
  const double dt = RndInt(0, 1) ? 1e-3 * RndInt(1, 8) : 1e-3 * (0.5 + Rnd());
  const int tiny = RndInt(0, 5) == 0;
  for (int i = 0; i < n; i++) {
    const double step = tiny && RndInt(0, 3) == 0 ? 1e-7 * (1 + Rnd()) : dt * (RndInt(0, 1) ? 1.0 : 0.5 + Rnd());
    t[i] = i == 0 ? 3.0 * Rnd() - 1.0 : t[i - 1] + step;
  }
  if (n > 2 && RndInt(0, 20) == 0) t[RndInt(1, n - 1)] = t[0];          // not increasing
  // velocities: a smooth profile decelerating towards the end, or random; at rest rows
  std::vector<double> q((size_t)n * D), qd((size_t)n * D), qdd((size_t)n * D), amax(D);
  const int shape = RndInt(0, 2);
  for (int j = 0; j < D; j++) amax[j] = 0.5 + 5.0 * Rnd();
  if (RndInt(0, 40) == 0) amax[RndInt(0, D - 1)] = RndInt(0, 1) ? 0.0 : -1.0;
  for (int j = 0; j < D; j++) {
    const double v0 = (2.0 * Rnd() - 1.0) * (shape == 2 ? 3.0 : 1.0);
    for (int i = 0; i < n; i++) {
      const double f = n > 1 ? (double)i / (n - 1) : 0.0;
      double v = shape == 0 ? v0 : shape == 1 ? v0 * (1.0 - f) : v0 * (0.5 + Rnd());
      qd[(size_t)i * D + j] = v;
      qdd[(size_t)i * D + j] = shape == 1 ? -v0 / std::max(1e-3, t[n - 1] - t[0]) : (2.0 * Rnd() - 1.0);
      q[(size_t)i * D + j] = 10.0 * Rnd();
    }
  }
  if (n > 0 && RndInt(0, 6) == 0)                                          // last sample nearly at rest
    for (int j = 0; j < D; j++) qd[(size_t)(n - 1) * D + j] = RndInt(0, 1) ? 0.0 : 5e-5 * (2.0 * Rnd() - 1.0);
  if (n > 2 && RndInt(0, 8) == 0) {                                        // a sample at rest mid-way
    const int r = RndInt(1, n - 2);
    for (int j = 0; j < D; j++) qd[(size_t)r * D + j] = RndInt(0, 1) ? 0.0 : 5e-9;
  }
  const double time_step = RndInt(0, 40) == 0 ? (RndInt(0, 1) ? 0.0 : -1e-3) : 1e-3;
  // the stop: by index (any, out of range included) or by time
  const bool by_index = RndInt(0, 3) == 0;
  int stop_index = 0;
  double time_sec = 0.0;
  if (by_index) {
    stop_index = RndInt(-1, n);
  } else if (n > 0) {
    const int kind = RndInt(0, 5);
    const int i = RndInt(0, n - 1);
    time_sec = kind == 0 ? t[0] - 1e-3 * Rnd() - 1e-9          // before the front
               : kind == 1 ? t[i]                              // on a sample
               : kind == 2 ? t[n - 1] + 0.5 * Rnd()            // past the end
               : kind == 3 ? t[n - 1]                          // on the last sample
                           : (i + 1 < n ? t[i] + (t[i + 1] - t[i]) * Rnd() : t[i]);
  } else {
    time_sec = Rnd();
  }

  // the mirror
  std::vector<VectorXd> Q(n), V(n), A(n);
  for (int i = 0; i < n; i++) {
    Q[i] = VectorXd(&q[(size_t)i * D], D);
    V[i] = VectorXd(&qd[(size_t)i * D], D);
    A[i] = VectorXd(&qdd[(size_t)i * D], D);
  }
  auto buf = *TrajectoryBuffer::Create();
  // InsertSegment does not check the times; a buffer with a repeated time stamp is loaded as is
  CHECK(buf->InsertSegment(Span<const double>(t.data(), n), Span<const VectorXd>(Q.data(), n),
                           Span<const VectorXd>(V.data(), n), Span<const VectorXd>(A.data(), n))
            .ok());
  const VectorXd am(amax.data(), D);
  const Status ms = by_index ? buf->StopAtIndex(stop_index, am, time_step) : buf->StopBeforeTime(time_sec, am, time_step);

  // the core
  const double nan = std::nan("");
  std::vector<double> ot(n, nan), oqd((size_t)n * D, nan), oqdd((size_t)n * D, nan);
  int keep = -7, first = -7, last = -7;
  const int st = tpamd::rs_stop_serial(t.data(), qd.data(), qdd.data(), n, D, amax.data(), time_step, by_index,
                                       stop_index, time_sec, &keep, &first, &last, ot.data(), oqd.data(), oqdd.data());
  CHECK(st == Code(ms));
  // rows outside [first, last] untouched
  for (int i = 0; i < n; i++)
    if (i < first || i > last) CHECK(std::isnan(ot[i]));
  // input[0, keep) ++ segment == the buffer
  std::vector<double> et, eq, ev, ea;
  for (int i = 0; i < keep && i < n; i++) {
    et.push_back(t[i]);
    eq.insert(eq.end(), q.begin() + (size_t)i * D, q.begin() + (size_t)(i + 1) * D);
    ev.insert(ev.end(), qd.begin() + (size_t)i * D, qd.begin() + (size_t)(i + 1) * D);
    ea.insert(ea.end(), qdd.begin() + (size_t)i * D, qdd.begin() + (size_t)(i + 1) * D);
  }
  for (int i = first; i <= last; i++) {
    et.push_back(ot[i]);
    eq.insert(eq.end(), q.begin() + (size_t)i * D, q.begin() + (size_t)(i + 1) * D);
    ev.insert(ev.end(), oqd.begin() + (size_t)i * D, oqd.begin() + (size_t)(i + 1) * D);
    ea.insert(ea.end(), oqdd.begin() + (size_t)i * D, oqdd.begin() + (size_t)(i + 1) * D);
  }
  const size_t bn = buf->GetNumSamples();
  bool same = et.size() == bn && SameBits(et.data(), buf->GetTimes().data(), bn);
  for (size_t i = 0; same && i < bn; i++)
    same = SameBits(&eq[i * D], buf->GetPositions()[i].data(), D) &&
           SameBits(&ev[i * D], buf->GetVelocities()[i].data(), D) &&
           SameBits(&ea[i * D], buf->GetAccelerations()[i].data(), D);
  CHECK(same);
  if (!same && g_fail < 25)
    std::printf("  case %d: n %d D %d by_index %d index %d time %.17g status %d keep %d first %d last %d buffer %zu\n", c,
                n, D, by_index, stop_index, time_sec, st, keep, first, last, bn);

  // category
  std::string cat;
  int index = stop_index, lower = -1;
  if (!by_index && n > 0 && time_sec >= t[0]) {
    tpamd::rs_index_for_time(t.data(), n, time_sec, &index);
    lower = (int)(std::lower_bound(t.begin(), t.end(), time_sec) - t.begin());
  }
  if (n == 0) cat = by_index ? "empty/by index" : "empty";
  else if (n == 1) cat = "one sample";
  else if (!by_index && time_sec < t[0]) cat = "before the front";
  else if (st == tpamd::kRsOutOfRange) cat = "index out of range";
  else if (std::fabs(amax[0]) >= 0 && [&] { for (double a : amax) if (a <= 0) return true; return false; }()) cat = "bad max_acceleration";
  else if (time_step <= 0) cat = "bad time_step";
  else if (st == tpamd::kRsOk && tpamd::rs_last_at_rest(index, n, &qd[(size_t)(n - 1) * D], D)) cat = "last-sample early return";
  else if (st == tpamd::kRsInvalidArgument) cat = "non-increasing times";
  else if (st == tpamd::kRsInternal) cat = "at-rest mid (Internal)";
  else if (st == tpamd::kRsNotFound) cat = "NotFound";
  else if (st == tpamd::kRsOk) {
    const int m = last - first + 1;
    cat = m == index ? "used all samples and matched" : "broke at rate >= 1";
    const double front = ot[first];
    const int lo = (int)(std::lower_bound(t.begin(), t.end(), front) - t.begin());
    (*counts)[lo > 0 && front - t[lo - 1] < tpamd::kRsTolerance ? "kept count decremented" : "kept count not decremented"]++;
  } else cat = "other status " + std::to_string(st);
  if (!by_index && lower + 1 > n - 1 && n > 1 && time_sec >= t[0]) (*counts)["clamped beyond the end"]++;
  return cat;
}

int main() {
  ReferenceCases();
  std::map<std::string, long> counts;
  const int kCases = 24000;
  for (int c = 0; c < kCases; c++) counts[FuzzOne(c, &counts)]++;
  std::printf("stop cases: %d\n", kCases);
  for (const auto &kv : counts) std::printf("category %s: %ld\n", kv.first.c_str(), kv.second);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

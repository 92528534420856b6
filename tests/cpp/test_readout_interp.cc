// CPU test of the planner-set readout's bracket and interpolation (run by
// tests/test_set_readout_cpu.py): the host/device functions of csrc/tpamd_readout.h, compiled here
// for the host, against the mirror's TrajectoryPlanner::Get{Position,Velocity,Acceleration}AtTime
// bit for bit, and the switch's sw_velocity_at_time (csrc/tpamd_switch.h), which now takes the same
// bracket, against GetVelocityAtTime.
//
// Seeded trajectories for D = 1, 3, 7, 16: times exactly on samples, between samples, on the first
// and the last sample, 1 ns outside both ends, anywhere inside; one-sample and empty trajectories;
// runs of repeated time stamps. Prints one line per category and "ALL OK".
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_readout.h"
#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_switch.h"
#include "../../x-edr-trajectory-planning_amd/host/trajectory_planner.h"

#define TEST_SUPPORT_SEED 20261016ULL
#include "test_support.h"

using namespace trajectory_planning;
using tpamd::compat::StatusCode;

static int PlanCode(const tpamd::compat::Status &s) {
  switch (s.code()) {
    case StatusCode::kOk: return tpamd::kRdOk;
    case StatusCode::kFailedPrecondition: return tpamd::kRdFailedPrecondition;
    case StatusCode::kOutOfRange: return tpamd::kRdOutOfRange;
    case StatusCode::kInvalidArgument: return tpamd::kRdInvalidArgument;
    default: return 4;
  }
}

// TrajectoryPlanner's getters on a filled buffer
struct BufferProbe : TrajectoryPlanner {
  Status Plan(Time, tpamd::compat::Duration) override { return Status(); }
  Status SetPath(std::shared_ptr<TimeablePath>) override { return Status(); }
  void ResetDerived() override {}
  void Fill(const std::vector<double> &t, const std::vector<VectorXd> &q, const std::vector<VectorXd> &qd,
            const std::vector<VectorXd> &qdd) {
    time_ = t; positions_ = q; velocities_ = qd; accelerations_ = qdd;
  }
};

static std::map<std::string, int> g_seen;

static void TestInterpolation() {
  const char *kinds[] = {"on a sample", "between samples", "first sample", "last sample", "1 ns before the first",
                         "1 ns after the last", "inside", "on a repeated stamp"};
  int cases = 0;
  for (int c = 0; c < 4000; c++) {
    const int D = (int[]){1, 3, 7, 16}[c % 4];
    const int shape = c % 23;                       // 0: empty, 1: one sample, 2..3: repeated stamps
    const int n = shape == 0 ? 0 : shape == 1 ? 1 : RndInt(2, 80);
    std::vector<double> t(n), fq, fqd, fqdd;
    std::vector<VectorXd> q(n, VectorXd(D)), qd(n, VectorXd(D)), qdd(n, VectorXd(D));
    double now = 1.0 + 5.0 * Rnd();
    for (int i = 0; i < n; i++) {
      const bool repeat = (shape == 2 || shape == 3) && i > 0 && Rnd() < 0.3;
      if (!repeat) now += (c % 5 == 0) ? 0.004 : 0.0005 + 0.01 * Rnd();
      t[i] = (double)(long long)(now * 1e9) / 1e9;  // on the nanosecond grid, as resampled times are
      for (int d = 0; d < D; d++) {
        q[i][d] = 4.0 * Rnd() - 2.0;
        qd[i][d] = 3.0 * Rnd() - 1.5;
        qdd[i][d] = 10.0 * Rnd() - 5.0;
      }
      fq.insert(fq.end(), q[i].begin(), q[i].end());
      fqd.insert(fqd.end(), qd[i].begin(), qd[i].end());
      fqdd.insert(fqdd.end(), qdd[i].begin(), qdd[i].end());
    }
    BufferProbe probe;
    probe.Fill(t, q, qd, qdd);
    for (int kind = 0; kind < 8; kind++) {
      long long ns = 3000000000LL;
      if (n > 0) {
        const int i = RndInt(0, n - 1);
        if (kind == 0) ns = (long long)llround(t[i] * 1e9);
        else if (kind == 1 && i + 1 < n) ns = (long long)((0.5 * (t[i] + t[i + 1])) * 1e9);
        else if (kind == 2) ns = (long long)llround(t[0] * 1e9);
        else if (kind == 3) ns = (long long)llround(t[n - 1] * 1e9);
        else if (kind == 4) ns = (long long)llround(t[0] * 1e9) - 1;
        else if (kind == 5) ns = (long long)llround(t[n - 1] * 1e9) + 1;
        else if (kind == 7) {
          int r = -1;
          for (int k = 0; k + 1 < n; k++)
            if (t[k] == t[k + 1]) { r = k; break; }
          if (r < 0) continue;
          ns = (long long)llround(t[r] * 1e9);
        } else ns = (long long)((t[0] + Rnd() * (t[n - 1] - t[0])) * 1e9);
      }
      const auto time = tpamd::compat::FromUnixNanos(ns);
      const double time_sec = (double)ns / 1e9;
      const auto wq = probe.GetPositionAtTime(time), wqd = probe.GetVelocityAtTime(time),
                 wqdd = probe.GetAccelerationAtTime(time);
      int l = -1, u = -1;
      const int st = tpamd::tb_bracket(t.data(), n, time_sec, &l, &u);
      CHECK(st == PlanCode(wq.status()) && st == PlanCode(wqd.status()) && st == PlanCode(wqdd.status()));
      std::vector<double> gq(D, -7.0), gqd(D, -7.0), gqdd(D, -7.0), sv(D, -9.0);
      const int sst = tpamd::sw_velocity_at_time(t.data(), fqd.data(), n, D, time_sec, sv.data());
      CHECK(sst == st);
      cases++;
      if (st == tpamd::kRdOk && wq.ok() && wqd.ok() && wqdd.ok()) {
        const double at = tpamd::tb_fraction(t.data(), l, u, time_sec);
        tpamd::tb_interpolate(fq.data(), l, u, D, at, gq.data());
        tpamd::tb_interpolate(fqd.data(), l, u, D, at, gqd.data());
        tpamd::tb_interpolate(fqdd.data(), l, u, D, at, gqdd.data());
        CHECK(std::memcmp(gq.data(), (*wq).data(), D * 8) == 0);
        CHECK(std::memcmp(gqd.data(), (*wqd).data(), D * 8) == 0);
        CHECK(std::memcmp(gqdd.data(), (*wqdd).data(), D * 8) == 0);
        CHECK(std::memcmp(sv.data(), (*wqd).data(), D * 8) == 0);
        CHECK(t[l] <= time_sec && (l == u ? l == n - 1 : time_sec < t[u]));
        if (kind == 3) CHECK(std::memcmp(gq.data(), q[n - 1].data(), D * 8) == 0);
      } else {
        CHECK(sv[0] == -9.0);                        // nothing written on failure
      }
      if (n == 0) CHECK(st == tpamd::kRdFailedPrecondition);
      if (n > 0 && (kind == 4 || kind == 5)) CHECK(st == tpamd::kRdOutOfRange);
      const std::string cat = std::string(n == 0 ? "empty" : n == 1 ? "one sample" : kinds[kind]) + "/" +
                              (st == 0 ? "ok" : "status " + std::to_string(st));
      g_seen[cat]++;
    }
  }
  std::printf("interpolation cases: %d\n", cases);
}

// the tick times: start + j step, and an overflow is reported instead of wrapping
static void TestTickTimes() {
  int64_t out = 0;
  CHECK(tpamd::tb_tick_time(1000, 4000000, 49, &out) && out == 1000 + 49 * 4000000LL);
  CHECK(tpamd::tb_tick_time(-5000000, 4000000, 2, &out) && out == 3000000);
  CHECK(!tpamd::tb_tick_time(LLONG_MAX - 10, 4, 3, &out));
  CHECK(tpamd::tb_tick_time(LLONG_MAX - 12, 4, 3, &out) && out == LLONG_MAX);
  CHECK(!tpamd::tb_tick_time(0, LLONG_MAX / 2 + 1, 2, &out));
  CHECK(tpamd::tb_tick_time(LLONG_MIN, 1, 0, &out) && out == LLONG_MIN);
  std::printf("tick times: ok\n");
}

int main() {
  TestInterpolation();
  TestTickTimes();
  for (const auto &kv : g_seen) std::printf("category %s: %d\n", kv.first.c_str(), kv.second);
  if (g_fail == 0) std::printf("ALL OK\n");
  else std::printf("%d CHECKS FAILED\n", g_fail);
  return g_fail == 0 ? 0 : 1;
}

// CPU test of the host/device arithmetic behind tpamd_planner_set_discard_ik_rows
// (csrc/tpamd_cartesian_window.h), run by tests/test_cartesian_discard_cpu.py, also stand-alone under
// AddressSanitizer / UndefinedBehaviorSanitizer:
//   cw_window_need_from  equals cw_window_need for first_row = 0 (random and tie-rounding cases);
//                        malformed exactly when the window's first row lies below first_row
//   cw_discard_floor     random non-decreasing histories: the first row k_plan_begin's rule picks for
//                        any start >= start_time_ is >= the floor, and the floor is attained at
//                        start == start_time_; states 1, 2, 3; count 0 and 1
//   cw_compact_*         the compaction schedule replayed sequentially (per chunk: all loads, then
//                        all stores) equals memmove for lengths 1..40, chunk sizes 1..8, all shifts
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_cartesian_window.h"
#include "test_support.h"

using namespace tpamd;

struct Rng {
  unsigned long long s;
  explicit Rng(unsigned long long seed) : s(seed * 2862933555777941757ULL + 3037000493ULL) { next(); next(); }
  double next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) / 9007199254740992.0;
  }
  double uniform(double lo, double hi) { return lo + (hi - lo) * next(); }
  int below(int n) { return std::min(n - 1, (int)(next() * n)); }
};

// k_plan_begin's rule (csrc/tpamd_kernels.h), restated: the first table row of a window that starts at
// start_sec, for path states 2 and 3 and a history of count >= 1 samples
static int PlanBeginFirstRow(const std::vector<double> &ht, const std::vector<double> &hs, double start_sec, double delta) {
  const int num = (int)ht.size();
  const int lo = (int)(std::lower_bound(ht.begin(), ht.end(), start_sec) - ht.begin());
  const int offset = std::min(std::max(lo - 1, 0), num - 1);
  return (int)std::round(hs[offset] / delta);
}

static void TestNeedFrom() {
  Rng rng(11);
  long same = 0, below = 0, kept = 0, ties = 0, malformed_both = 0;
  for (int i = 0; i < 6000; i++) {
    const int N = 3 + rng.below(200);
    double delta = rng.uniform(1e-3, 0.5);
    int k = rng.below(3000) - 20;                        // some negative starts
    double path_start = k * delta;
    if (i % 3 == 0) { path_start = (k + 0.5) * delta; ties++; }       // rounding ties
    if (i % 5 == 0) path_start += rng.uniform(-0.49, 0.49) * delta;
    double path_horizon = path_start + delta * (N - 1);
    if (i % 17 == 0) path_horizon += delta * (1 + rng.below(3));      // malformed: not N rows
    if (i % 41 == 0) delta = i % 82 ? 0.0 : -delta;                    // malformed: delta
    const int rows = rng.below(4000);
    int f0, l0, nf0, nc0, f1, l1, nf1, nc1;
    const int r0 = cw_window_need(path_start, path_horizon, delta, N, rows, &f0, &l0, &nf0, &nc0);
    const int r1 = cw_window_need_from(path_start, path_horizon, delta, N, rows, 0, &f1, &l1, &nf1, &nc1);
    CHECK(r0 == r1 && f0 == f1 && l0 == l1 && nf0 == nf1 && nc0 == nc1);
    same += r0 == r1;
    // a first resident row around the window's first row
    for (int first_row : {f0 - 1, f0, f0 + 1, f0 + N, rows - 1, rows + 3, 1}) {
      if (first_row < 0) continue;
      const int r2 = cw_window_need_from(path_start, path_horizon, delta, N, rows, first_row, &f1, &l1, &nf1, &nc1);
      CHECK(f1 == f0 && l1 == l0);
      if (r0 == kCwMalformed) {
        CHECK(r2 == kCwMalformed && nf1 == 0 && nc1 == 0);
        malformed_both++;
      } else if (f0 < first_row) {
        CHECK(r2 == kCwMalformed && nf1 == 0 && nc1 == 0);
        below++;
      } else {
        CHECK(r2 == r0 && nf1 == nf0 && nc1 == nc0);
        kept++;
      }
    }
  }
  std::printf("need_from equal at first_row 0: %ld\nrounding ties: %ld\nbelow first_row: %ld\nat or above first_row: %ld\n"
              "malformed either way: %ld\n", same, ties, below, kept, malformed_both);
}

static void TestFloor() {
  Rng rng(12);
  long later = 0, attained = 0, zero_cases = 0, positive = 0;
  for (int i = 0; i < 3000; i++) {
    const int count = i % 50 == 0 ? 0 : (i % 50 == 1 ? 1 : 1 + rng.below(300));
    const double delta = rng.uniform(1e-3, 0.2);
    std::vector<double> ht(count), hs(count);
    double t = rng.uniform(0.0, 5.0), s = rng.uniform(0.0, 3.0);
    for (int k = 0; k < count; k++) {
      ht[k] = t; hs[k] = s;
      if (rng.next() < 0.8) t += rng.uniform(0.0, 0.05);        // repeated time stamps stay in
      if (rng.next() < 0.8) s += rng.uniform(0.0, 2.0) * delta;  // non-decreasing, flat stretches stay in
      if (i % 7 == 0 && rng.next() < 0.3) s = (std::floor(s / delta) + 1.5) * delta;   // rounding ties
    }
    const double t0 = count ? ht[0] : 0.0, t1 = count ? ht[count - 1] : 1.0;
    const double start_time = rng.uniform(t0 - 0.1, t1 + 0.1);
    for (int state : {1, 2, 3}) {
      const int floor_row = cw_discard_floor(ht.data(), hs.data(), count, start_time, state, delta);
      CHECK(floor_row >= 0);
      if (state == 1 || count == 0) {
        CHECK(floor_row == 0);
        zero_cases++;
        continue;
      }
      CHECK(PlanBeginFirstRow(ht, hs, start_time, delta) == floor_row);       // attained at start == start_time_
      attained++;
      positive += floor_row > 0;
      for (int j = 0; j < 20; j++) {
        double start = start_time + (j < 3 ? 0.0 : rng.uniform(0.0, t1 - t0 + 0.3));
        if (j == 1 && count > 1) start = std::max(start_time, ht[rng.below(count)]);   // exactly on a sample
        CHECK(PlanBeginFirstRow(ht, hs, start, delta) >= floor_row);
        later++;
      }
    }
    // a delta that is not positive has no rows to speak of
    CHECK(cw_discard_floor(ht.data(), hs.data(), count, start_time, 3, 0.0) == 0);
  }
  std::printf("floor attained: %ld\nlater starts: %ld\nfloor zero by rule: %ld\nfloor positive: %ld\n", attained, later,
              zero_cases, positive);
}

static void TestCompactionSchedule() {
  long runs = 0, overlapping = 0;
  for (int len = 1; len <= 40; len++)
    for (int T = 1; T <= 8; T++)
      for (int threads = 1; threads <= T; threads++) {
        if (T % threads) continue;
        const int unroll = T / threads;
        for (int shift = 0; shift < len; shift++) {
          // a table of len elements loses its first `shift`: n = len - shift elements move down
          std::vector<int> a(len), ref(len);
          for (int i = 0; i < len; i++) a[i] = ref[i] = 1000 + i;
          const int n = len - shift;
          std::memmove(ref.data(), ref.data() + shift, (size_t)n * sizeof(int));
          if (shift > 0) {          // the kernel does not run for a shift of 0
            const long long chunks = cw_compact_chunks(n, threads, unroll);
            CHECK(chunks == (n + T - 1) / T);
            std::vector<char> visited(n, 0);
            for (long long c = 0; c < chunks; c++) {
              std::vector<int> reg((size_t)T);
              for (int tid = 0; tid < threads; tid++)          // all loads of the chunk
                for (int u = 0; u < unroll; u++) {
                  const long long e = cw_compact_index(c, threads, unroll, tid, u);
                  CHECK(e >= c * T && e < (c + 1) * T);
                  if (e < n) reg[(size_t)tid * unroll + u] = a[e + shift];
                }
              for (int tid = 0; tid < threads; tid++)          // the barrier, then all stores
                for (int u = 0; u < unroll; u++) {
                  const long long e = cw_compact_index(c, threads, unroll, tid, u);
                  if (e < n) { a[e] = reg[(size_t)tid * unroll + u]; visited[e]++; }
                }
            }
            for (int e = 0; e < n; e++) CHECK(visited[e] == 1);
            overlapping += shift < n;
          }
          CHECK(std::memcmp(a.data(), ref.data(), (size_t)n * sizeof(int)) == 0);
          runs++;
        }
      }
  std::printf("compaction schedules: %ld\noverlapping moves: %ld\n", runs, overlapping);
}

int main() {
  TestNeedFrom();
  TestFloor();
  TestCompactionSchedule();
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

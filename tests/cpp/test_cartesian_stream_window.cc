// CPU test of cw_window_need (csrc/tpamd_cartesian_window.h), run by tests/test_cartesian_stream_cpu.py
// as a plain build and as a stand-alone -fsanitize=address,undefined build. Host code only; it needs
// no library.
//   grid     cw_window_need on a grid of (path_start, delta, N, rows) against a restatement of
//            TimeableCartesianSplinePath::SamplePath's index arithmetic
//            (timeable_path_cartesian_spline.cc:464-476, :527-530, :671-674) written here: the
//            resident / needs rows / malformed split, first / last, need_first / need_count. The grid
//            holds the rounding ties of round(path_start / delta), rows = last, last + 1 and
//            last + 2, negative starts, and non-positive and NaN delta. cw_window's answer is
//            unchanged by it.
//   machine  "suspend at window w, append exactly the need, resume" simulated on the host over the
//            window starts of a receding-horizon run: the growing table visits the same
//            (first, last) sequence as the full-table index rule of the oracle's IK-table planner
//            (oracle/tp_oracle_plan.c:308-310, restated), never holds more than last + 1 rows, and
//            ends with the size SamplePath leaves path_ik_positions_ with.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_cartesian_window.h"
#include "test_support.h"

// :671-674
static int PathIkIndex(double parameter, double delta) { return (int)std::round(parameter / delta); }

// SamplePath on a table of `rows` rows. :464-476: rows horizon_ik_upper_index .. are appended when
// the horizon's index is not below the table's last index; the first new sample re-evaluates the
// last row, so indices current + 1 .. horizon are what the table gains (:516-517). :527-530: the
// CHECK_EQ on the window's width. Returns 0 resident (nothing appended), 1 rows appended, 2 a window
// the copy cannot take (first < 0 or the width is not N - 1; the reference aborts or reads before
// the table).
struct RefAnswer { int kind, first, last, appended_first, appended_count, rows_after; };
static RefAnswer ReferenceSamplePath(double path_start, double delta, int N, int rows) {
  RefAnswer r{};
  const double path_horizon = path_start + delta * (N - 1);
  const int horizon = PathIkIndex(path_horizon, delta);
  const int current = rows - 1;
  r.first = PathIkIndex(path_start, delta);
  r.last = horizon;
  r.rows_after = rows;
  if (r.first < 0 || horizon - r.first != N - 1) { r.kind = 2; return r; }
  if (horizon >= current) {
    const int num_new_samples = horizon - current + 1;     // the first one is not appended
    r.appended_first = current + 1;
    r.appended_count = num_new_samples - 1;
    r.rows_after = rows + r.appended_count;
  }
  r.kind = r.appended_count > 0 ? 1 : 0;
  return r;
}

// oracle/tp_oracle_plan.c:308-310 on the full table
static bool OracleWindow(double path_start, double path_horizon, double delta, int N, int table_len, int *first,
                         int *last) {
  *first = (int)round(path_start / delta);
  *last = (int)round(path_horizon / delta);
  return !(*first < 0 || *last - *first != N - 1 || *last >= table_len);
}

int main() {
  long cases = 0, resident = 0, needs = 0, malformed = 0, ties = 0, rows_last = 0, rows_last1 = 0, rows_last2 = 0,
       negative = 0;
  for (int rep = 0; rep < 40; rep++) {
    g_seed = 91000 + rep;
    const int N = 3 + (int)(Rnd() * 70);
    // deltas that are and are not exactly representable: ties of round() occur with the former
    const double delta = (rep % 4 == 0) ? 0.25 : (rep % 4 == 1) ? 0.0078125 : 0.001 + 0.05 * Rnd();
    std::vector<double> starts;
    for (int r = -3; r <= 40; r++) {
      const double s = r * delta;
      for (double x : {s, std::nextafter(s, 1e300), std::nextafter(s, -1e300), s + 0.49 * delta, s - 0.49 * delta,
                       s + 0.5 * delta, s - 0.5 * delta, std::nextafter(s + 0.5 * delta, 1e300),
                       std::nextafter(s + 0.5 * delta, -1e300), s + (0.98 * Rnd() - 0.49) * delta})
        starts.push_back(x);
    }
    for (double s : starts) {
      const double horizon = s + delta * (N - 1);
      const double frac = s / delta - std::floor(s / delta);
      const bool tie = frac == 0.5;
      const int l = PathIkIndex(horizon, delta);
      for (int rows : {l, l + 1, l + 2, l - 5, l + 40, N, 1}) {
        if (rows < 1) continue;
        const RefAnswer ref = ReferenceSamplePath(s, delta, N, rows);
        int f1, l1, nf, nc, f0, l0;
        const int kind = tpamd::cw_window_need(s, horizon, delta, N, rows, &f1, &l1, &nf, &nc);
        const bool ok0 = tpamd::cw_window(s, horizon, delta, N, rows, &f0, &l0);
        CHECK(kind == ref.kind && f1 == ref.first && l1 == ref.last);
        CHECK(ok0 == (kind == tpamd::kCwResident) && f0 == f1 && l0 == l1);
        if (kind == tpamd::kCwNeedsRows) {
          CHECK(nf == ref.appended_first && nc == ref.appended_count && nf == rows && nc >= 1);
          CHECK(nf + nc == ref.rows_after && ref.rows_after == l1 + 1);
          // after exactly that append the window is resident and the table ends on its last row
          int f2, l2, nf2, nc2;
          CHECK(tpamd::cw_window_need(s, horizon, delta, N, nf + nc, &f2, &l2, &nf2, &nc2) == tpamd::kCwResident &&
                f2 == f1 && l2 == l1 && nf2 == 0 && nc2 == 0);
          // one row less and it still waits, for that one row
          if (nc > 1)
            CHECK(tpamd::cw_window_need(s, horizon, delta, N, nf + nc - 1, &f2, &l2, &nf2, &nc2) == tpamd::kCwNeedsRows &&
                  nf2 == nf + nc - 1 && nc2 == 1);
          needs++;
        } else {
          CHECK(nf == 0 && nc == 0);
          (kind == tpamd::kCwResident ? resident : malformed)++;
        }
        cases++;
        ties += tie;
        negative += s < 0.0;
        if (kind != tpamd::kCwMalformed) {
          rows_last += rows == l1;
          rows_last1 += rows == l1 + 1;
          rows_last2 += rows == l1 + 2;
        }
      }
    }
  }
  {
    // a sampling distance that is not positive has no window, whatever the table
    int f, l, nf = 7, nc = 7;
    for (double d : {0.0, -0.1, (double)std::nan("")}) {
      CHECK(tpamd::cw_window_need(0.0, d * 9, d, 10, 100, &f, &l, &nf, &nc) == tpamd::kCwMalformed && nf == 0 && nc == 0);
      CHECK(tpamd::cw_window_need(0.0, d * 9, d, 10, 5, &f, &l, &nf, &nc) == tpamd::kCwMalformed && nf == 0 && nc == 0);
      CHECK(!tpamd::cw_window(0.0, d * 9, d, 10, 100, &f, &l));
    }
  }
  std::printf("cases: %ld\nresident: %ld\nneeds rows: %ld\nmalformed: %ld\nrounding ties: %ld\nnegative starts: %ld\n",
              cases, resident, needs, malformed, ties, negative);
  std::printf("rows = last: %ld\nrows = last + 1: %ld\nrows = last + 2: %ld\n", rows_last, rows_last1, rows_last2);
  CHECK(resident > 1000 && needs > 1000 && malformed > 100 && ties > 0 && negative > 0 && rows_last > 0 &&
        rows_last1 > 0 && rows_last2 > 0);

  // the state machine: window starts as Plan produces them (a sample of the previous window: start +
  // i * delta for some i in N/2 .. N-1, :639-646 / :328-339), until the path's end is planned
  long machine_windows = 0, suspensions = 0, machines = 0;
  for (int rep = 0; rep < 200; rep++) {
    g_seed = 93000 + rep;
    const int N = 8 + (int)(Rnd() * 120);
    const double path_end = 0.5 + 3.0 * Rnd();
    const double delta = ((rep % 2) ? 0.25 : 0.4) * path_end / (N - 1);
    const int full_rows = (int)std::lround(path_end / delta) + N + 1;       // BuildIkTable
    int rows = N;                                                           // the first upload
    double start = 0.0;
    int max_last = -1;
    for (int w = 0; w < 10000; w++) {
      const double horizon = start + delta * (N - 1);
      int f0, l0;
      const bool ok0 = OracleWindow(start, horizon, delta, N, full_rows, &f0, &l0);
      CHECK(ok0);                                       // the full table holds every window of the run
      int f, l, nf, nc;
      int kind = tpamd::cw_window_need(start, horizon, delta, N, rows, &f, &l, &nf, &nc);
      if (kind == tpamd::kCwNeedsRows) {                // suspend, append exactly the need, resume
        CHECK(nf == rows && nc >= 1);
        rows = nf + nc;
        suspensions++;
        kind = tpamd::cw_window_need(start, horizon, delta, N, rows, &f, &l, &nf, &nc);
      }
      CHECK(kind == tpamd::kCwResident && f == f0 && l == l0);
      max_last = l > max_last ? l : max_last;
      CHECK(rows == max_last + 1 || (rows == N && max_last + 1 <= N));      // never more than the windows asked for
      CHECK(rows <= full_rows);
      machine_windows++;
      if (horizon >= path_end - 1e-4) break;            // CloseToEnd: planned to the end
      const int i = N / 2 + (int)(Rnd() * (N - N / 2));
      start = start + delta * i;                        // s of sample i of this window
    }
    CHECK(rows == max_last + 1 && rows < full_rows);    // the tail past the last window is never held
    machines++;
  }
  std::printf("state machines: %ld\nmachine windows: %ld\nsuspensions: %ld\n", machines, machine_windows, suspensions);
  CHECK(suspensions > machines);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

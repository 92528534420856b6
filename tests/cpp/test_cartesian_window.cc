// CPU test of csrc/tpamd_cartesian_window.h (run by tests/test_cartesian_set_cpu.py): the window
// rule of a Cartesian planner set, compiled for the host, against the oracle, bit for bit.
//   cw_window   first / last and the range verdict against the index rule of
//               oracle/tp_oracle_plan.c:308-310, for window starts on, and within +-1 ulp and
//               +-0.49 delta of, multiples of delta; windows that end exactly on, one row before and
//               one row past the table end included
//   cw_rows_at  q', q'', J q' (component by component) and the 2D+2 rows of every sample
//               against tpo_cartesian_path_derivatives, tpo_cartesian_jacobian_times_q1 and
//               tpo_cartesian_constraint_setup on the same table segment
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_cartesian_window.h"
#include "test_support.h"

static bool Same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * 8) == 0; }

// tp_oracle_plan.c:308-310
static bool OracleWindow(double path_start, double path_horizon, double delta, int N, int table_len, int *first,
                         int *last) {
  *first = (int)round(path_start / delta);
  *last = (int)round(path_horizon / delta);
  return !(*first < 0 || *last - *first != N - 1 || *last >= table_len);
}

int main() {
  long windows = 0, in_range = 0, out_of_range = 0, samples = 0, on_end = 0, before_end = 0, past_end = 0;
  for (int D : {1, 5, 6, 7, 16}) {
    for (int rep = 0; rep < 6; rep++) {
      g_seed = 77000 + 131 * D + rep;
      const int N = 3 + (int)(Rnd() * 60);
      const int rows = N + 1 + (int)(Rnd() * 150);
      const double delta = 0.001 + 0.05 * Rnd();
      const double safety = 0.8 + 0.2 * Rnd();
      std::vector<double> q((size_t)rows * D), J((size_t)rows * 6 * D), vmax(D), amax(D);
      for (auto &v : q) v = 2.0 * Rnd() - 1.0;
      for (auto &v : J) v = 2.0 * Rnd() - 1.0;
      for (int d = 0; d < D; d++) { vmax[d] = 0.5 + 0.6 * Rnd(); amax[d] = 1.2 + 1.8 * Rnd(); }
      const double vt = 0.3 + 0.3 * Rnd(), vr = 0.8 + 0.4 * Rnd();
      // window starts: every multiple of delta around the table (a row before it, rows past its end),
      // each exact, +-1 ulp, +-0.49 delta and a random offset inside the rounding cell
      std::vector<double> starts;
      for (int r = -1; r <= rows - N + 2; r++) {
        const double s = r * delta;
        starts.push_back(s);
        starts.push_back(std::nextafter(s, 1e300));
        starts.push_back(std::nextafter(s, -1e300));
        starts.push_back(s + 0.49 * delta);
        starts.push_back(s - 0.49 * delta);
        starts.push_back(s + (0.98 * Rnd() - 0.49) * delta);
      }
      std::vector<double> wq((size_t)N * D), q1((size_t)N * D), q2((size_t)N * D), jq1((size_t)6 * N);
      const int C = 2 * D + 2;
      std::vector<double> A((size_t)N * C), Bm(A.size()), LO(A.size()), HI(A.size());
      std::vector<double> rec(2 * D), a(C), bb(C), lo(C), hi(C);
      double jv[6];
      for (double s : starts) {
        const double horizon = s + delta * (N - 1);      // path_timing_trajectory.cc:340-341
        int f0, l0, f1, l1;
        const bool ok0 = OracleWindow(s, horizon, delta, N, rows, &f0, &l0);
        const bool ok1 = tpamd::cw_window(s, horizon, delta, N, rows, &f1, &l1);
        CHECK(ok0 == ok1 && f0 == f1 && l0 == l1);
        windows++;
        if (f0 >= 0 && l0 - f0 == N - 1) {
          on_end += l0 == rows - 1;
          before_end += l0 == rows - 2;
          past_end += l0 == rows;
        }
        if (!ok0) { out_of_range++; continue; }
        in_range++;
        // the oracle on the segment (tp_oracle_plan.c:311-316)
        std::memcpy(wq.data(), q.data() + (size_t)f0 * D, sizeof(double) * N * D);
        tpo_cartesian_path_derivatives(wq.data(), N, D, delta, q1.data(), q2.data());
        tpo_cartesian_jacobian_times_q1(J.data() + (size_t)f0 * 6 * D, q1.data(), N, D, jq1.data());
        tpo_cartesian_constraint_setup(q1.data(), q2.data(), jq1.data(), N, D, vmax.data(), amax.data(), vt, vr,
                                       safety, A.data(), Bm.data(), LO.data(), HI.data());
        const double inv = 1.0 / delta;
        for (int i = 0; i < N; i++) {
          tpamd::cw_rows_at(i, N, D, inv, q.data() + (size_t)(f1 + i) * D, J.data() + (size_t)(f1 + i) * 6 * D,
                            vmax.data(), amax.data(), safety, vt, vr, rec.data(), a.data(), bb.data(), lo.data(),
                            hi.data(), jv);
          bool same = true;
          for (int d = 0; d < D; d++)
            same = same && Same(&rec[2 * d], &q1[(size_t)i * D + d], 1) && Same(&rec[2 * d + 1], &q2[(size_t)i * D + d], 1);
          CHECK(same);
          // J q' component by component; the Cartesian B rows are its squared norms (3 + 3)
          const double *v6 = jq1.data() + (size_t)6 * i;
          CHECK(Same(jv, v6, 6));
          const double bt = (v6[0] * v6[0] + v6[1] * v6[1]) + v6[2] * v6[2];
          const double br = (v6[3] * v6[3] + v6[4] * v6[4]) + v6[5] * v6[5];
          CHECK(Same(&bb[2 * D], &bt, 1) && Same(&bb[2 * D + 1], &br, 1));
          CHECK(Same(a.data(), &A[(size_t)i * C], C) && Same(bb.data(), &Bm[(size_t)i * C], C) &&
                Same(lo.data(), &LO[(size_t)i * C], C) && Same(hi.data(), &HI[(size_t)i * C], C));
          samples++;
        }
      }
    }
  }
  std::printf("windows: %ld\nin range: %ld\nout of range: %ld\nsamples: %ld\n", windows, in_range, out_of_range, samples);
  std::printf("window ends on the last row: %ld\none row before: %ld\none row past: %ld\n", on_end, before_end, past_end);
  CHECK(in_range > 1000 && out_of_range > 100 && on_end > 0 && before_end > 0 && past_end > 0);
  {
    // a sampling distance that is not positive has no window, whatever the table
    int f, l;
    CHECK(!tpamd::cw_window(0.0, 0.0, 0.0, 10, 100, &f, &l) && !tpamd::cw_window(0.0, -0.9, -0.1, 10, 100, &f, &l) &&
          !tpamd::cw_window(0.0, 0.0, std::nan(""), 10, 100, &f, &l));
  }
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

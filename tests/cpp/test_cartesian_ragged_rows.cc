// CPU test of the ragged row arithmetic of csrc/tpamd_cartesian_window.h (run by
// tests/test_cartesian_ragged_cpu.py): cw_ragged_count, cw_ragged_first_row and cw_rows_ragged_at,
// compiled for the host, against the oracle's set-up of every path ALONE at N = n, bit for bit.
//   packed   the paths' rows lie shuffled in one table, each path directly followed by another
//            path's rows (or, for the last one, by rows of NaN): an end condition taken from the
//            stride instead of the path's count would read them and differ
//   strided  the same paths in a [B][stride] batch whose rows beyond n[b] are NaN
//   counts   n in {3, 4, 5, 64}; 0, 1, stride + 1 and a negative count give no sample at all
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../oracle/tp_oracle.h"
#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_cartesian_window.h"
#include "test_support.h"

static bool Same(const double *a, const double *b, size_t n) { return std::memcmp(a, b, n * 8) == 0; }

int main() {
  const int counts[] = {3, 4, 5, 64, 64, 5, 4, 3};     // two paths of every count
  const int order[] = {5, 2, 7, 0, 3, 6, 1, 4};        // where each path's rows lie in the table
  const int B = 8, stride = 70;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  long samples = 0, refused = 0;
  for (int D : {1, 5, 6, 7, 16}) {
    g_seed = 91000 + 17 * D;
    const int C = 2 * D + 2;
    // every path's own rows, limits and sampling distance
    std::vector<std::vector<double>> pq(B), pJ(B), vmax(B), amax(B);
    std::vector<double> delta(B), vt(B), vr(B), safety(B);
    int total = 0;
    for (int b = 0; b < B; b++) {
      const int n = counts[b];
      pq[b].resize((size_t)n * D); pJ[b].resize((size_t)n * 6 * D); vmax[b].resize(D); amax[b].resize(D);
      for (auto &v : pq[b]) v = 2.0 * Rnd() - 1.0;
      for (auto &v : pJ[b]) v = 2.0 * Rnd() - 1.0;
      for (int d = 0; d < D; d++) { vmax[b][d] = 0.5 + 0.6 * Rnd(); amax[b][d] = 1.2 + 1.8 * Rnd(); }
      delta[b] = 0.001 + 0.05 * Rnd(); vt[b] = 0.3 + 0.3 * Rnd(); vr[b] = 0.8 + 0.4 * Rnd();
      safety[b] = 0.8 + 0.2 * Rnd();
      total += n;
    }
    // packed table: the paths in `order`, then two rows of NaN
    std::vector<double> tq((size_t)(total + 2) * D, nan), tJ((size_t)(total + 2) * 6 * D, nan);
    std::vector<int32_t> ns(B), first(B);
    int row = 0;
    for (int k = 0; k < B; k++) {
      const int b = order[k];
      first[b] = row; ns[b] = counts[b];
      std::memcpy(&tq[(size_t)row * D], pq[b].data(), pq[b].size() * 8);
      std::memcpy(&tJ[(size_t)row * 6 * D], pJ[b].data(), pJ[b].size() * 8);
      row += counts[b];
    }
    // strided batch: rows beyond a path's count are NaN
    std::vector<double> sq((size_t)B * stride * D, nan), sJ((size_t)B * stride * 6 * D, nan);
    for (int b = 0; b < B; b++) {
      std::memcpy(&sq[(size_t)b * stride * D], pq[b].data(), pq[b].size() * 8);
      std::memcpy(&sJ[(size_t)b * stride * 6 * D], pJ[b].data(), pJ[b].size() * 8);
    }
    std::vector<double> rec(2 * D), a(C), bb(C), lo(C), hi(C);
    double jv[6];
    for (int b = 0; b < B; b++) {
      const int n = counts[b];
      // the oracle on the path alone (N = n)
      std::vector<double> q1((size_t)n * D), q2((size_t)n * D), jq1((size_t)6 * n);
      std::vector<double> A((size_t)n * C), Bm(A.size()), LO(A.size()), HI(A.size());
      tpo_cartesian_path_derivatives(pq[b].data(), n, D, delta[b], q1.data(), q2.data());
      tpo_cartesian_jacobian_times_q1(pJ[b].data(), q1.data(), n, D, jq1.data());
      tpo_cartesian_constraint_setup(q1.data(), q2.data(), jq1.data(), n, D, vmax[b].data(), amax[b].data(), vt[b],
                                     vr[b], safety[b], A.data(), Bm.data(), LO.data(), HI.data());
      CHECK(tpamd::cw_ragged_count(n, stride) == n);
      CHECK(tpamd::cw_ragged_first_row(first.data(), b, stride) == (size_t)first[b]);
      CHECK(tpamd::cw_ragged_first_row(nullptr, b, stride) == (size_t)b * stride);
      for (int layout = 0; layout < 2; layout++) {
        const int32_t *fr = layout == 0 ? first.data() : nullptr;
        const double *Q = layout == 0 ? tq.data() : sq.data(), *JJ = layout == 0 ? tJ.data() : sJ.data();
        for (int i = 0; i < stride; i++) {
          const bool did = tpamd::cw_rows_ragged_at(b, i, stride, D, ns.data(), fr, 1.0 / delta[b], Q, JJ,
                                                    vmax[b].data(), amax[b].data(), safety[b], vt[b], vr[b],
                                                    rec.data(), a.data(), bb.data(), lo.data(), hi.data(), jv);
          CHECK(did == (i < n));
          if (!did || i >= n) continue;
          bool same = true;
          for (int d = 0; d < D; d++)
            same = same && Same(&rec[2 * d], &q1[(size_t)i * D + d], 1) && Same(&rec[2 * d + 1], &q2[(size_t)i * D + d], 1);
          CHECK(same);
          CHECK(Same(jv, jq1.data() + (size_t)6 * i, 6));
          CHECK(Same(a.data(), &A[(size_t)i * C], C) && Same(bb.data(), &Bm[(size_t)i * C], C) &&
                Same(lo.data(), &LO[(size_t)i * C], C) && Same(hi.data(), &HI[(size_t)i * C], C));
          samples++;
        }
      }
    }
    // counts the set-up kernel refuses: no sample, nothing read (the table pointers are null)
    for (int bad : {0, 1, stride + 1, -5}) {
      std::vector<int32_t> nb(B, bad);
      CHECK(tpamd::cw_ragged_count(bad, stride) == 0);
      for (int i = 0; i < stride; i++) {
        CHECK(!tpamd::cw_rows_ragged_at(3, i, stride, D, nb.data(), first.data(), 1.0, nullptr, nullptr, nullptr,
                                        nullptr, 0.8, 1.0, 1.0, nullptr, nullptr, nullptr, nullptr, nullptr));
        refused++;
      }
    }
    CHECK(tpamd::cw_ragged_count(2, stride) == 2 && tpamd::cw_ragged_count(stride, stride) == stride);
  }
  std::printf("samples: %ld\nrefused: %ld\n", samples, refused);
  CHECK(samples == 5L * 2 * 2 * (3 + 4 + 5 + 64) && refused == 5L * 4 * 70);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

// CPU test of the mirror's bucketing (run by tests/test_cartesian_ragged_cpu.py):
// trajectory_planning::CartesianTimingBuckets on length lists with known buckets. The function is
// header-only, so this needs neither the engine library nor a GPU.
#include <cstdio>
#include <set>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/host/batch_cartesian_timing.h"
#include "test_support.h"

using trajectory_planning::CartesianTimingBuckets;
typedef std::vector<std::vector<size_t>> Buckets;

int main() {
  {
    // one joint count, one safety: the edges of the 512-sample buckets
    const std::vector<size_t> n = {3, 512, 513, 1024, 1025, 511, 600, 4000, 3585, 3584};
    const std::vector<size_t> d(n.size(), 6);
    const std::vector<double> sf(n.size(), 0.8);
    const Buckets b = CartesianTimingBuckets(d, n, sf, 0, n.size());
    const Buckets want = {{0, 1, 5}, {2, 3, 6}, {4}, {9}, {7, 8}};   // ceil(n / 512) = 1, 2, 3, 7, 8
    CHECK(b == want);
  }
  {
    // 40 paths of 40 distinct lengths 500 .. 890 in steps of 10, alternating 6 and 7 joints: lengths
    // up to 512 and above it, per joint count -- four buckets where the exact-count rule had 40
    std::vector<size_t> n, d;
    std::vector<double> sf;
    for (int k = 0; k < 40; k++) { n.push_back(500 + 10 * k); d.push_back(k % 2 ? 7 : 6); sf.push_back(0.8); }
    const Buckets b = CartesianTimingBuckets(d, n, sf, 0, 40);
    CHECK(b.size() == 4);
    CHECK((b[0] == std::vector<size_t>{0}) && (b[2] == std::vector<size_t>{1}));   // 500 (D 6), 510 (D 7)
    size_t total = 0;
    std::set<size_t> seen;
    for (const auto &ids : b) {
      total += ids.size();
      for (size_t k = 0; k < ids.size(); k++) {
        seen.insert(ids[k]);
        CHECK(d[ids[k]] == d[ids[0]] && (n[ids[k]] + 511) / 512 == (n[ids[0]] + 511) / 512);
        if (k) CHECK(ids[k] > ids[k - 1]);                 // index order inside a bucket
      }
    }
    CHECK(total == 40 && seen.size() == 40);
  }
  {
    // the safety factor and the joint count split buckets; [lo, hi) limits the paths
    const std::vector<size_t> n = {100, 100, 100, 100, 100, 100};
    const std::vector<size_t> d = {6, 6, 7, 6, 7, 6};
    const std::vector<double> sf = {0.8, 0.9, 0.8, 0.8, 0.8, 0.8};
    const Buckets all = CartesianTimingBuckets(d, n, sf, 0, 6);
    const Buckets want = {{0, 3, 5}, {1}, {2, 4}};
    CHECK(all == want);
    const Buckets part = CartesianTimingBuckets(d, n, sf, 2, 5);
    const Buckets want_part = {{3}, {2, 4}};
    CHECK(part == want_part);
    CHECK(CartesianTimingBuckets(d, n, sf, 3, 3).empty());
  }
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

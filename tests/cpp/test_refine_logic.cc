// The decisions of a refined call (csrc/tpamd_refine.h: refine_candidate, refine_slot_code,
// refine_first, refine_step and the continue rule inside it) run on the host, built with the address
// and undefined-behaviour sanitizers by tests/test_refine_cpu.py, which holds the output equal to a
// numpy restatement.
//
// The slot ranks are formed the way k_refine_select forms them: the paths in chunks of 256, a 64-bit
// vote mask per wave, the count of set bits below the lane, the waves' totals, and a running base
// across chunks.
//
// stdin:  B M N max_samples max_rounds tolerance
//         B lines: violations worst_excess n delta, then max_rounds pairs (violations worst_excess):
//                  the record of the path's solve in round r, should it make one
// stdout: "name count values...", doubles as hex floats.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../x-edr-trajectory-planning_amd/csrc/tpamd_refine.h"

using namespace tpamd;

static double read_double() {
  char buf[64];
  if (std::scanf("%63s", buf) != 1) std::exit(2);
  return std::strtod(buf, nullptr);
}
static int read_int() {
  int v;
  if (std::scanf("%d", &v) != 1) std::exit(2);
  return v;
}
static void print_ints(const char *name, const std::vector<int32_t> &v) {
  std::printf("%s %zu", name, v.size());
  for (int32_t x : v) std::printf(" %d", x);
  std::printf("\n");
}
static void print_doubles(const char *name, const std::vector<double> &v) {
  std::printf("%s %zu", name, v.size());
  for (double x : v) std::printf(" %a", x);
  std::printf("\n");
}

int main() {
  const int B = read_int(), M = read_int(), N = read_int(), max_samples = read_int(), max_rounds = read_int();
  const double tolerance = read_double();
  std::vector<int32_t> violations(B), n(B);
  std::vector<double> excess(B), delta(B);
  std::vector<std::vector<int32_t>> made_violations(B, std::vector<int32_t>(max_rounds));
  std::vector<std::vector<double>> made_excess(B, std::vector<double>(max_rounds));
  for (int b = 0; b < B; b++) {
    violations[b] = read_int();
    excess[b] = read_double();
    n[b] = read_int();
    delta[b] = read_double();
    for (int r = 0; r < max_rounds; r++) {
      made_violations[b][r] = read_int();
      made_excess[b][r] = read_double();
    }
  }
  (void)N;
  // k_refine_select's walk
  constexpr int kChunk = 256, kWaves = 4;
  std::vector<int32_t> slot(B), slot_path(M, -1);
  std::vector<RefineSlot> state(M, refine_unused());
  int running = 0;
  for (int base = 0; base < B; base += kChunk) {
    int cand[kChunk];
    uint64_t votes[kWaves] = {0, 0, 0, 0};
    for (int t = 0; t < kChunk; t++) {
      const int b = base + t;
      cand[t] = b < B ? refine_candidate(violations[b], excess[b], tolerance, n[b], max_samples) : kRefineNothing;
      if (cand[t] == 0) votes[t >> 6] |= (uint64_t)1 << (t & 63);
    }
    int total = 0;
    for (int w = 0; w < kWaves; w++) total += __builtin_popcountll(votes[w]);
    for (int t = 0; t < kChunk; t++) {
      const int b = base + t, wave = t >> 6, lane = t & 63;
      if (b >= B) break;
      int before = 0;
      for (int w = 0; w < wave; w++) before += __builtin_popcountll(votes[w]);
      const int below = __builtin_popcountll(votes[wave] & (((uint64_t)1 << lane) - 1));
      const int code = refine_slot_code(cand[t], running + before + below, M);
      slot[b] = code;
      if (code >= 0) {
        slot_path[code] = b;
        state[code] = refine_first(n[b], delta[b]);
      }
    }
    running += total;
  }
  const int used = running < M ? running : M;
  print_ints("slot", slot);
  print_ints("slot_path", slot_path);
  print_ints("num_refined", {used});
  std::vector<int32_t> first_samples(M);
  std::vector<double> first_delta(M);
  for (int k = 0; k < M; k++) {
    first_samples[k] = state[k].next_samples;
    first_delta[k] = state[k].next_delta;
  }
  print_ints("first_samples", first_samples);
  print_doubles("first_delta", first_delta);
  // the rounds: k_refine_step's trip for every slot
  std::vector<int32_t> live(1, used);
  for (int r = 1; r <= max_rounds; r++) {
    int count = 0;
    for (int k = 0; k < M; k++) {
      const int b = slot_path[k];
      const int v = b >= 0 ? made_violations[b][r - 1] : -1;
      const double x = b >= 0 ? made_excess[b][r - 1] : 0.0;
      if (!refine_step(state[k], v, x, tolerance, max_rounds, max_samples)) continue;
      if (state[k].next_samples > 0) count++;
    }
    live.push_back(count);
  }
  print_ints("live", live);
  std::vector<int32_t> rounds(M), num_samples(M), next_samples(M);
  std::vector<double> delta_out(M);
  for (int k = 0; k < M; k++) {
    rounds[k] = state[k].rounds;
    num_samples[k] = state[k].num_samples;
    delta_out[k] = state[k].delta;
    next_samples[k] = state[k].next_samples;
  }
  print_ints("rounds", rounds);
  print_ints("num_samples", num_samples);
  print_doubles("delta", delta_out);
  print_ints("next_samples", next_samples);
  return 0;
}

// tpamd_refine.h -- refinement of violating paths on the device (include/tpamd.h
// tpamd_time_joint_paths_refined_*, tpamd_time_waypoint_paths_refined_*): what lies between a check
// (tpamd_check.h) and the next solve, so that a caller who finds violated rows does not download
// the records, pick the violators, build a second batch and solve again from the host.
//
// Round 0 is the plain solve at the caller's stride and its check. k_refine_select turns the [B]
// check record into a slot map: the paths that need refinement and whose doubled grid fits the
// refined arrays take slots 0, 1, .. in ascending path index (a prefix count, no atomics: the map
// is the same in every run). k_refine_gather copies a slot's spline, limits and start values into
// the sub-batch of M slots. Rounds 1 .. max_rounds solve the sub-batch as a ragged joint batch of
// stride max_samples -- a slot's count is n_r = 2 n_{r-1} - 1 with delta_r = delta_{r-1} / 2 (exact:
// the old samples are every second new one), or 0 once the slot is settled, which with the skip
// mark (kErrSkip) leaves its outputs as they are -- and check it; k_refine_step, one thread per
// slot, keeps the record of the solve just made and decides the slot's next count.
//
// The decisions per path and per slot are TPAMD_HD inline functions, so that the host compiles
// them too (tests/cpp/test_refine_logic.cc, also under the address and undefined-behaviour
// sanitizers).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#ifndef TPAMD_HD
#define TPAMD_HD __host__ __device__
#endif
#else
#ifndef TPAMD_HD
#define TPAMD_HD
#endif
#endif

namespace tpamd {

// slot[b] below 0 (include/tpamd.h)
constexpr int kRefineNothing = -1;   // clean, within tolerance, or not checked
constexpr int kRefineNoSlot = -2;    // needs refinement, every slot is taken
constexpr int kRefineTooLong = -3;   // needs refinement, 2 n - 1 > max_samples

// A path (or a slot's last solve) needs refinement: it has violated rows and its worst excess lies
// above the tolerance. A path that was not checked (-1 / NaN) does not: both comparisons are false.
TPAMD_HD inline bool refine_needed(int violations, double worst_excess, double tolerance) {
  return violations > 0 && worst_excess > tolerance;
}

// n <= 8192: no overflow
TPAMD_HD inline int refine_next_samples(int n) { return 2 * n - 1; }
TPAMD_HD inline double refine_next_delta(double delta) { return delta / 2.0; }

// Round 0, path b with n samples: 0 if it is a candidate for a slot, otherwise its slot code.
TPAMD_HD inline int refine_candidate(int violations, double worst_excess, double tolerance, int n, int max_samples) {
  if (!refine_needed(violations, worst_excess, tolerance)) return kRefineNothing;
  if (refine_next_samples(n) > max_samples) return kRefineTooLong;
  return 0;
}

// The slot code of a path: `rank` = the number of candidates with a smaller path index.
TPAMD_HD inline int refine_slot_code(int candidate, int rank, int max_refined) {
  if (candidate < 0) return candidate;
  return rank < max_refined ? rank : kRefineNoSlot;
}

// A slot whose round r solve (n_r samples) has the record (violations, worst_excess) goes on to
// round r + 1.
TPAMD_HD inline bool refine_continues(int violations, double worst_excess, double tolerance, int r, int max_rounds,
                                      int n_r, int max_samples) {
  return refine_needed(violations, worst_excess, tolerance) && r < max_rounds &&
         refine_next_samples(n_r) <= max_samples;
}

// What a slot carries from round to round.
struct RefineSlot {
  int32_t rounds;        // solves made
  int32_t num_samples;   // of the last solve made
  double delta;          // of the last solve made
  int32_t next_samples;  // of the next solve; 0: settled (or unused)
  double next_delta;
};

// a used slot behind k_refine_select
TPAMD_HD inline RefineSlot refine_first(int n0, double delta0) {
  RefineSlot s;
  s.rounds = 0;
  s.num_samples = 0;
  s.delta = 0.0;
  s.next_samples = refine_next_samples(n0);
  s.next_delta = refine_next_delta(delta0);
  return s;
}
TPAMD_HD inline RefineSlot refine_unused() {
  RefineSlot s;
  s.rounds = 0;
  s.num_samples = 0;
  s.delta = 0.0;
  s.next_samples = 0;
  s.next_delta = 0.0;
  return s;
}

// Behind a round's check: (violations, worst_excess) is the record of the solve the slot just made
// with s.next_samples samples. Returns false, and leaves `s` alone, for a slot that made none.
TPAMD_HD inline bool refine_step(RefineSlot &s, int violations, double worst_excess, double tolerance, int max_rounds,
                                 int max_samples) {
  if (s.next_samples <= 0) return false;
  s.rounds += 1;
  s.num_samples = s.next_samples;
  s.delta = s.next_delta;
  if (refine_continues(violations, worst_excess, tolerance, s.rounds, max_rounds, s.num_samples, max_samples)) {
    s.next_samples = refine_next_samples(s.num_samples);
    s.next_delta = refine_next_delta(s.delta);
  } else {
    s.next_samples = 0;
  }
  return true;
}

#if defined(__HIPCC__) || defined(__HIP__)

// a check record on the device: violations required, the rest may be null (tpamd_check.h CheckOutputs)
struct RefineRecord {
  int32_t *violations;
  double *worst_excess;
  int32_t *worst_sample, *worst_row, *first_sample;
};

struct RefineSelectParams {
  int B, M, N;                       // paths; slots; round 0's stride
  int max_samples;
  double tolerance;
  const int32_t *violations;         // [B] round 0's record
  const double *worst_excess;        // [B]
  const int32_t *ns;                 // [B] round 0's counts, or null: N
  const double *delta;               // [B] round 0's
  int32_t *slot;                     // [B]
  int32_t *slot_path;                // [M]
  int32_t *num_refined;              // [1]
  int32_t *live;                     // [1] slots with a solve to make
  int32_t *rounds, *num_samples;     // [M]
  double *delta_out;                 // [M]
  int32_t *next_samples;             // [M] the sub-batch's num_samples_per_path
  double *next_delta;                // [M] the sub-batch's delta
  RefineRecord record;               // [M] the caller's refined_check, every array may be null: set to "not checked"
};

struct RefineGatherParams {
  int M, D;
  int knots_per_path, points_per_path;   // P + 3 and P of the source and of the sub-batch (the waypoint form: S)
  const int32_t *slot_path;              // [M]
  const double *knots, *cps, *vmax, *amax, *path_start, *sd_start, *sdd_start, *time_start;   // [B]..; the three
                                                                                              // start arrays may be null: 0
  const int32_t *np;                     // [B] or null (waypoint form: control points of path b)
  double *knots_out, *cps_out, *vmax_out, *amax_out, *path_start_out, *sd_start_out, *sdd_start_out, *time_start_out;
  int32_t *np_out;                       // [M] or null; 0 for an unused slot
};

struct RefineStepParams {
  int M, max_rounds, max_samples;
  double tolerance;
  RefineRecord made;                     // [M] the record the sub-batch's check just wrote
  RefineRecord out;                      // [M] the caller's refined_check: every array may be null
  int32_t *rounds, *num_samples;         // [M]
  double *delta_out;                     // [M]
  int32_t *next_samples;                 // [M]
  double *next_delta;                    // [M]
  int32_t *live;                         // [1] set to 0 in front of this kernel; counts the slots that go on
};

// Each enqueues one kernel on `st` (tpamd_refine.hip).
void launch_refine_select(const RefineSelectParams &p, hipStream_t st);
void launch_refine_gather(const RefineGatherParams &p, hipStream_t st);
void launch_refine_step(const RefineStepParams &p, hipStream_t st);
#endif

}  // namespace tpamd

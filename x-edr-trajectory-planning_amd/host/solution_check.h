// The arithmetic of the solution check on the host (no engine, no GPU): the five-number record of
// one solution on its constraint rows -- TimeOptimalPathProfile::SolutionSatisfiesConstraints
// (time_optimal_path_timing.cc:492-518) plus the excess and the tie rule of include/tpamd.h
// tpamd_check_* -- and the rule that merges the records of the windows of one Plan call into a
// planner's tpamd_planner_check. Compile with -ffp-contract=off: v is two products and one sum.
#ifndef TPAMD_HOST_SOLUTION_CHECK_H_
#define TPAMD_HOST_SOLUTION_CHECK_H_

#include <limits>

#include "../../include/tpamd.h"

namespace trajectory_planning {

struct SolutionCheckRecord {
  int violations = -1;            // violated rows; -1: not checked
  double worst_excess = std::numeric_limits<double>::quiet_NaN();   // NaN: no row with an excess
  int worst_sample = -1, worst_row = -1;
  int first_sample = -1;          // first sample with a violated row
};

// rows a, b, lower, upper [N][C]; sd2, sdd [N]. An excess is max(lower - v, v - upper), the second
// where both are equal, NaN (and then left out) if either difference is NaN; among equal excesses
// the smallest i * C + c keeps the place.
inline SolutionCheckRecord CheckSolutionRows(int N, int C, const double *a, const double *b, const double *lower,
                                             const double *upper, const double *sd2, const double *sdd) {
  constexpr double kTiny = std::numeric_limits<double>::epsilon() * 1e5;
  SolutionCheckRecord r;
  r.violations = 0;
  for (int i = 0; i < N; i++) {
    for (int c = 0; c < C; c++) {
      const size_t k = (size_t)i * C + c;
      const double v = a[k] * sdd[i] + b[k] * sd2[i];
      if ((v + kTiny < lower[k]) || (v - kTiny > upper[k])) {
        ++r.violations;
        if (r.first_sample < 0) r.first_sample = i;
      }
      const double e_lo = lower[k] - v, e_hi = v - upper[k];
      if (e_lo != e_lo || e_hi != e_hi) continue;
      const double e = e_lo > e_hi ? e_lo : e_hi;
      if (r.worst_sample < 0 || e > r.worst_excess) {
        r.worst_excess = e;
        r.worst_sample = i;
        r.worst_row = c;
      }
    }
  }
  return r;
}

// The record of a planner none of whose windows was checked.
inline tpamd_planner_check EmptyPlannerCheck() {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  return tpamd_planner_check{0, -1, -1, -1, -1, -1, -1, -1, nan, nan};
}

// Window `window` (numbered in solve order within the Plan call) into the planner's record: counts
// add, the larger excess wins and an equal one keeps the smaller (window, sample, row), the first
// violated (window, sample) stays. path_parameter: the window's s at w.worst_sample (not read
// without one). A window that was not checked (w.violations < 0) changes nothing.
inline void MergeWindowRecord(const SolutionCheckRecord &w, int window, double path_parameter,
                              tpamd_planner_check *record) {
  if (w.violations < 0) return;
  tpamd_planner_check &r = *record;
  r.windows += 1;
  r.violations = (r.violations < 0 ? 0 : r.violations) + w.violations;
  r.last_window_violations = w.violations;
  if (w.worst_sample >= 0) {
    const bool earlier = window < r.worst_window ||
                         (window == r.worst_window && (w.worst_sample < r.worst_sample ||
                                                       (w.worst_sample == r.worst_sample && w.worst_row < r.worst_row)));
    if (r.worst_window < 0 || w.worst_excess > r.worst_excess || (w.worst_excess == r.worst_excess && earlier)) {
      r.worst_excess = w.worst_excess;
      r.worst_window = window;
      r.worst_sample = w.worst_sample;
      r.worst_row = w.worst_row;
      r.worst_parameter = path_parameter;
    }
  }
  if (w.first_sample >= 0 &&
      (r.first_window < 0 || window < r.first_window || (window == r.first_window && w.first_sample < r.first_sample))) {
    r.first_window = window;
    r.first_sample = w.first_sample;
  }
}

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_SOLUTION_CHECK_H_

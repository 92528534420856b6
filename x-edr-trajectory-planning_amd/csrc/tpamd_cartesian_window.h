// tpamd_cartesian_window.h -- one timing window of a Cartesian path, read out of its IK table.
//
// TimeableCartesianSplinePath keeps its IK solution in path_ik_positions_, one row per multiple of
// delta_parameter (timeable_path_cartesian_spline.cc:464-549, PathIkIndex = round(parameter /
// delta) :671-674). A window is arithmetic on N consecutive rows of that table:
//   cw_window     which rows (SamplePath :527-542), and whether the table holds them
//   cw_window_need  the same, and which rows a growing table still lacks (streaming Plan)
//   cw_window_need_from / cw_discard_floor / cw_compact_*  the same for a table whose consumed
//                 front rows were discarded, which rows are safe to discard, and the in-place move
//   cw_rows_at    ComputePathDerivatives :39-68 (forward differences, q'[N-1] = 0, q''[0] =
//                 q''[N-1] = 0) and ConstraintSetup :551-595 (the 2D joint rows plus two rows
//                 bounding |(J q')_{1..3}|^2 and |(J q')_{4..6}|^2 with lower = -upper; J q' is
//                 accumulated over the dofs in index order)
//   cw_ragged_count / cw_ragged_first_row / cw_rows_ragged_at  the same arithmetic for a path of a
//                 ragged batch: its own sample count, its own first row (strided or packed)
// All compile for the host as well (TPAMD_HD): tests/cpp/test_cartesian_window.cc holds them
// against the CPU restatement of the reference, bit for bit. k_plan_begin and k_cartesian_rows
// (tpamd_kernels.h) call them.
#pragma once

#include <math.h>
#include <stddef.h>

#ifndef TPAMD_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define TPAMD_HD __host__ __device__
#else
#define TPAMD_HD
#endif
#endif

namespace tpamd {

// The table rows of the window [path_start, path_horizon]: first = PathIkIndex(path_start), last =
// PathIkIndex(path_horizon). False if the table (`rows` rows) does not hold N rows from `first` on.
TPAMD_HD inline bool cw_window(double path_start, double path_horizon, double delta, int N, int rows, int *first,
                               int *last) {
  *first = *last = -1;
  if (!(delta > 0.0)) return false;      // (also keeps the conversions below defined)
  const int f = (int)round(path_start / delta);
  const int l = (int)round(path_horizon / delta);
  *first = f;
  *last = l;
  return !(f < 0 || l - f != N - 1 || l >= rows);
}

// cw_window with a three-way answer, for tables that grow as SamplePath grows path_ik_positions_
// (:464-549: each call appends the rows between the table's last row and the window's last row).
//   kCwResident   as cw_window's true
//   kCwMalformed  as cw_window's false for a window no table can hold: delta not positive,
//                 first < 0 or last - first != N - 1
//   kCwNeedsRows  a well-formed window with last >= rows: rows need_first = rows .. need_first +
//                 need_count - 1 = last are missing; once they are appended the table has last + 1
//                 rows, the size SamplePath leaves it with (:516-517)
// need_first / need_count are 0 unless rows are needed.
enum { kCwResident = 0, kCwNeedsRows = 1, kCwMalformed = 2 };
TPAMD_HD inline int cw_window_need(double path_start, double path_horizon, double delta, int N, int rows, int *first,
                                   int *last, int *need_first, int *need_count) {
  *need_first = *need_count = 0;
  if (cw_window(path_start, path_horizon, delta, N, rows, first, last)) return kCwResident;
  if (!(delta > 0.0)) return kCwMalformed;
  if (*first < 0 || *last - *first != N - 1) return kCwMalformed;
  *need_first = rows;
  *need_count = *last + 1 - rows;
  return kCwNeedsRows;
}

// cw_window_need for a table whose front has been discarded (tpamd_planner_set_discard_ik_rows):
// the table holds path rows first_row .. rows - 1, row r in slot r - first_row. A well-formed window
// whose first row lies below first_row is kCwMalformed (need_first = need_count = 0): those rows are
// gone and cannot be supplied again, since an append only goes behind the last row. Every other
// answer, and first / last in every case, is cw_window_need's; first_row = 0 is cw_window_need.
TPAMD_HD inline int cw_window_need_from(double path_start, double path_horizon, double delta, int N, int rows,
                                        int first_row, int *first, int *last, int *need_first, int *need_count) {
  const int r = cw_window_need(path_start, path_horizon, delta, N, rows, first, last, need_first, need_count);
  if (r == kCwMalformed || *first >= first_row) return r;
  *need_first = *need_count = 0;
  return kCwMalformed;
}

// The lowest table row any later Plan of a planner can read: rows below it may be discarded.
//   * k_plan_begin starts a window at path_start = h_s[offset], offset = clamp(lower_bound(h_time,
//     start_sec) - 1, 0, count - 1), and reads rows round(path_start / delta) .. + N - 1.
//   * start_sec is the Plan's start, or a later loop start within the same Plan, and
//     HandleTimeArguments rejects a start before start_time_. lower_bound is monotone in start_sec,
//     so offset >= offset(start_time_).
//   * A window replaces the history from its own offset on (k_plan_append) and starts at the
//     parameter it found there; the samples below that offset stay. So the offset a later start
//     finds in a later history is not below the one start_time_ finds now, and h_s there is not
//     smaller: h_s is non-decreasing.
//   * round is monotone, so every later window's first row is >= round(h_s[offset(start_time_)] /
//     delta). A Plan that starts at start_time_ reads exactly that row: the floor is attained.
//   * A planner that waits for rows (streaming Plan) recomputes its window from the same history
//     with a loop start >= start_time_: the same floor covers it.
//   * A new path (path_state 1) plans from parameter 0, and so does a planner without a history
//     (count 0; the caller passes 0 for a planner without a path): floor 0.
// h_time / h_s are the planner's window history (count samples), start_time_sec is start_time_ in
// seconds as k_plan_begin converts it (ns / 1e9).
TPAMD_HD inline int cw_discard_floor(const double *h_time, const double *h_s, int count, double start_time_sec,
                                     int path_state, double delta) {
  if (path_state == 1 || count <= 0 || !(delta > 0.0)) return 0;
  int lo = 0, hi = count;                       // lower_bound(h_time, start_time_sec)
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (h_time[mid] < start_time_sec) lo = mid + 1; else hi = mid;
  }
  int offset = lo - 1;
  if (offset < 0) offset = 0;
  if (offset > count - 1) offset = count - 1;
  const double f = round(h_s[offset] / delta);
  if (!(f > 0.0)) return 0;
  return f >= 2147483647.0 ? 2147483647 : (int)f;
}

// In-place compaction of a table's live rows after a discard (k_pset_ik_compact): n elements move
// from index e + shift to index e, shift >= 1. The elements are visited in chunks of T = threads *
// unroll, in ascending order; within a chunk every thread loads its `unroll` elements, the
// workgroup meets at a barrier, then every thread stores them. Chunk c reads [cT + shift, (c+1)T +
// shift) and writes [cT, (c+1)T): it writes nothing a later chunk still has to read (those start at
// (c+1)T + shift) and only places that it or an earlier chunk has read, and the barrier puts all of
// its loads before its stores. tests/cpp/test_cartesian_discard_window.cc replays this schedule.
TPAMD_HD inline long long cw_compact_chunks(long long n, int threads, int unroll) {
  const long long T = (long long)threads * unroll;
  return (n + T - 1) / T;
}
// the destination index of load u (0 .. unroll-1) of thread tid in chunk c; it takes part if < n
TPAMD_HD inline long long cw_compact_index(long long c, int threads, int unroll, int tid, int u) {
  return (c * unroll + u) * threads + tid;
}

// Sample i of a window of N: q points at the sample's table row ([.][D], the next two rows are read
// where they are inside the window), J at its Jacobian [6][D]. Writes the (q', q'') pairs to
// rec[2 D] and the sample's 2D+2 constraint rows; jq1, if not null, receives J q' [6].
TPAMD_HD inline void cw_rows_at(int i, int N, int D, double inv_delta, const double *q, const double *J,
                                const double *vmax, const double *amax, double safety, double vt, double vr,
                                double *rec, double *a, double *bb, double *lo, double *hi, double *jq1 = nullptr) {
  double v6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int d = 0; d < D; d++) {
    double q1 = 0.0, q2 = 0.0;
    if (i < N - 1) {
      q1 = inv_delta * (q[D + d] - q[d]);
      if (i >= 1) {
        const double q1n = (i + 1 < N - 1) ? inv_delta * (q[2 * D + d] - q[D + d]) : 0.0;
        q2 = inv_delta * (q1n - q1);
      }
    }
    rec[2 * d] = q1;
    rec[2 * d + 1] = q2;
    const double am = amax[d] * safety;
    const double vm = vmax[d] * safety;
    a[d] = q1;       bb[d] = q2;          hi[d] = am;          lo[d] = -am;
    a[D + d] = 0.0;  bb[D + d] = q1 * q1; hi[D + d] = vm * vm; lo[D + d] = 0.0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 6; r++) v6[r] += J[r * D + d] * q1;
  }
  if (jq1)
    for (int r = 0; r < 6; r++) jq1[r] = v6[r];
  a[2 * D] = 0.0;
  bb[2 * D] = (v6[0] * v6[0] + v6[1] * v6[1]) + v6[2] * v6[2];
  hi[2 * D] = vt * vt;
  lo[2 * D] = -(vt * vt);
  a[2 * D + 1] = 0.0;
  bb[2 * D + 1] = (v6[3] * v6[3] + v6[4] * v6[4]) + v6[5] * v6[5];
  hi[2 * D + 1] = vr * vr;
  lo[2 * D + 1] = -(vr * vr);
}

// Ragged Cartesian batches (tpamd_time_cartesian_paths_ragged_*): path b has ns[b] samples in arrays
// of stride `stride`, and its rows start at first_row[b] of a row table or, without first_row, at
// b * stride of a [B][stride] batch. A count outside [2, stride] fails the path in the set-up kernel;
// the kernels that read rows treat it as a path of no samples, so none of its rows is touched.
TPAMD_HD inline int cw_ragged_count(int n, int stride) { return (n >= 2 && n <= stride) ? n : 0; }
TPAMD_HD inline size_t cw_ragged_first_row(const int *first_row, int b, int stride) {
  return first_row ? (size_t)first_row[b] : (size_t)b * stride;
}
// cw_rows_at for sample i of path b of a ragged batch: the window is the path's own ns[b] rows, so
// the end conditions sit at ns[b] - 1 whatever follows the path in the table. q_table / J_table are
// the whole inputs; vmax / amax the path's limits. False (nothing read or written) for i >= the
// path's count.
TPAMD_HD inline bool cw_rows_ragged_at(int b, int i, int stride, int D, const int *ns, const int *first_row,
                                       double inv_delta, const double *q_table, const double *J_table,
                                       const double *vmax, const double *amax, double safety, double vt, double vr,
                                       double *rec, double *a, double *bb, double *lo, double *hi,
                                       double *jq1 = nullptr) {
  const int n = cw_ragged_count(ns[b], stride);
  if (i >= n) return false;
  const size_t row = cw_ragged_first_row(first_row, b, stride) + (size_t)i;
  cw_rows_at(i, n, D, inv_delta, q_table + row * D, J_table + row * 6 * D, vmax, amax, safety, vt, vr, rec, a, bb,
             lo, hi, jq1);
  return true;
}

}  // namespace tpamd

// tpamd_cartesian_window.h -- one timing window of a Cartesian path, read out of its IK table.
//
// TimeableCartesianSplinePath keeps its IK solution in path_ik_positions_, one row per multiple of
// delta_parameter (timeable_path_cartesian_spline.cc:464-549, PathIkIndex = round(parameter /
// delta) :671-674). A window is arithmetic on N consecutive rows of that table:
//   cw_window     which rows (SamplePath :527-542), and whether the table holds them
//   cw_window_need  the same, and which rows a growing table still lacks (streaming Plan)
//   cw_rows_at    ComputePathDerivatives :39-68 (forward differences, q'[N-1] = 0, q''[0] =
//                 q''[N-1] = 0) and ConstraintSetup :551-595 (the 2D joint rows plus two rows
//                 bounding |(J q')_{1..3}|^2 and |(J q')_{4..6}|^2 with lower = -upper; J q' is
//                 accumulated over the dofs in index order)
// Both compile for the host as well (TPAMD_HD): tests/cpp/test_cartesian_window.cc holds them
// against the CPU restatement of the reference, bit for bit. k_plan_begin and k_cartesian_rows
// (tpamd_kernels.h) call them.
#pragma once

#include <math.h>

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

}  // namespace tpamd

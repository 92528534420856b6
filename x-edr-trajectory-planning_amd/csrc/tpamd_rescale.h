// tpamd_rescale.h -- stopping trajectories (include/tpamd.h tpamd_stop_trajectories_*,
// tpamd_planner_set_stop_trajectories*): TrajectoryBuffer::StopBeforeTime / StopAtIndex
// (trajectory_buffer.cc:296-385) with RescaleTrajectoryBackwardToStop (rescale_to_stop.cc) for a
// batch of sampled trajectories.
//
// Per trajectory (n samples) and stop time: index = min(lower_bound(time) + 1, n - 1); the checks
// (index in [1, n - 1], max_acceleration > 0, time_step > 0); on the last sample with |v| < 1e-4
// only its v and a become 0; times strictly increasing up to index; |v[index]| < 1e-8 is
// TPAMD_PLAN_INTERNAL, where the reference aborts (and so is a rest sample without an admissible
// deceleration, rs_front_finite). Then the squared time-scaling rate, 0 at
// sample `index`, is integrated backward: for every joint c with |qd_c| >= 1e-8 the candidates
// d = -2 (qdd_c rate2 -+ a_c) / qd_c; a candidate is valid if every joint's
// qdd_j rate2 + 0.5 qd_j d lies in [-a_j, a_j] up to 1e-8; d = min(0, smallest valid candidate);
// next = rate2 - d dt; the rescaled step is 2 dt / (sqrt(rate2) + sqrt(min(next, 1))); until
// next >= 1 or sample 2. The row of iteration i (velocity sqrt(min(next, 1)) qd[i], acceleration
// of sample i) pairs with position sample i - 1: the segment covers rows [index + 1 - m, index]
// of the input, row index being the rest row. Its times are shifted so that it starts at
// time[index + 1 - m]. A segment that uses every sample (m == index) must match the velocity
// the trajectory has at its start within 1e-2 (else TPAMD_PLAN_NOT_FOUND). The buffer after the
// stop is input[0, keep) ++ segment, keep from InsertSegment's search with tolerance 1e-6.
//
// The scalar parts compile for the host as well (TPAMD_HD): tests/cpp/test_stop_buffer.cc holds
// rs_stop_serial, which composes them, bit-equal to the mirror's TrajectoryBuffer
// (host/trajectory_buffer.cc). Every operation is in the mirror's order; the library is built with
// -ffp-contract=off, '/' and sqrt are correctly rounded, min / max are written as comparisons.
// Non-finite inputs are outside the contract.
//
// Layout (as tpamd_stop.h): a group of L = next_pow2(2 D) lanes serves one trajectory; lane c owns
// candidate c (joint c / 2, sign c & 1) and runs the validity test over the D joints, the group
// minimum comes from xor shuffles, and rate2 and the running rescaled time are group-uniform. The
// loads of sample i - 1 are issued before sample i is computed. The segment length m, and with it
// the time shift, is known only when the loop ends, and a stop that fails the velocity match must
// leave the outputs untouched; so the loop runs twice: once to find m, the shift, the status and
// keep, and, for a stop that succeeds, once more writing the rows with their final times.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__HIP__)
#include "tpamd_stop.h"          // stop_group_lanes, pset_time_to_sec
#endif

#include "tpamd_readout.h"       // TPAMD_HD, tb_bracket / tb_interpolate

namespace tpamd {

// TPAMD_PLAN_* (include/tpamd.h) of a stop
enum { kRsOk = 0, kRsOutOfRange = 2, kRsInvalidArgument = 3, kRsInternal = 4, kRsNotFound = 6 };

constexpr int kRsMaxDofs = 16;
constexpr double kRsTolerance = 1e-6;   // TrajectoryBufferOptions::timestep_tolerance default

// |v|_inf, NaN ignored (as the mirror's maxAbs)
TPAMD_HD inline double rs_max_abs(const double *v, int D) {
  double m = 0.0;
  for (int j = 0; j < D; j++) {
    const double a = fabs(v[j]);
    m = a > m ? a : m;
  }
  return m;
}

// StopBeforeTime's sample (:372-385): *index = min(lower_bound(time_sec) + 1, n - 1). An empty
// trajectory gives kRsOk with *index = -1 (nothing changes); a time before the first sample
// kRsOutOfRange.
TPAMD_HD inline int rs_index_for_time(const double *t, int n, double time_sec, int *index) {
  *index = -1;
  if (n <= 0) return kRsOk;
  if (time_sec < t[0]) return kRsOutOfRange;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t[mid] < time_sec) lo = mid + 1; else hi = mid;
  }
  *index = (n - 1 < lo + 1) ? n - 1 : lo + 1;
  return kRsOk;
}

// StopAtIndex's argument checks (:298-314)
TPAMD_HD inline int rs_check_args(int index, int n, const double *amax, int D, double time_step) {
  if (index <= 0 || index > n - 1) return kRsOutOfRange;
  double mn = amax[0];
  for (int j = 1; j < D; j++) mn = amax[j] < mn ? amax[j] : mn;
  if (mn <= 0.0) return kRsInvalidArgument;
  if (time_step <= 0.0) return kRsInvalidArgument;
  return kRsOk;
}

// The early return on the last sample (:316-322)
TPAMD_HD inline bool rs_last_at_rest(int index, int n, const double *qd_last, int D) {
  return index == n - 1 && rs_max_abs(qd_last, D) < 1e-4;
}

// AreInputsValidForSampledTrajectory's time test on the pairs (i, i + 1), lo <= i < hi
TPAMD_HD inline bool rs_increasing(const double *t, int lo, int hi) {
  for (int i = lo; i < hi; i++)
    if (t[i + 1] <= t[i]) return false;
  return true;
}

// The rescaling's "already at rest" test on sample index (rescale_to_stop.cc)
TPAMD_HD inline bool rs_at_rest(const double *qd_index, int D) { return rs_max_abs(qd_index, D) < 1e-8; }

// A rest sample whose moving joints all fail the validity test (a joint at the 1e-8 cut that asks
// more of a joint under the cut than its limit allows) has d = 0 at rate2 = 0: the first rescaled
// step is 2 dt / 0, rt is -inf and the segment's front time rt + (t[first] - rt) is NaN. The
// reference goes on and inserts rows with NaN times; here that stop is kRsInternal and nothing
// changes (the second deviation, next to the sample already at rest). Checked before the front
// time reaches a search.
TPAMD_HD inline bool rs_front_finite(double front) { return front - front == 0.0; }

// Candidate c (joint c / 2; c odd: +max_acceleration, even: -) of a sample with velocity v and
// acceleration acc at rate2: its diff_rate_squared if the joint moves, every scaled acceleration
// stays within the bounds and it is below 0; otherwise 0 (the loop's start value).
// The kernel passes the candidate joint's v_c, acc_c, a_c separately (no dynamic register index).
TPAMD_HD inline double rs_candidate_of(const double *v, const double *acc, const double *amax, int D, double rate2,
                                       double v_c, double acc_c, double a_c, bool plus) {
  if (fabs(v_c) < 1e-8) return 0.0;
  const double sign = plus ? 1.0 : -1.0;
  const double d = -2.0 * (acc_c * rate2 + sign * a_c) / v_c;
  bool valid = true;
  for (int j = 0; j < D; j++) {
    const double s = acc[j] * rate2 + 0.5 * v[j] * d;
    valid = valid && amax[j] - s >= -1e-8 && -amax[j] - s <= 1e-8;
  }
  return (valid && d < 0.0) ? d : 0.0;
}
TPAMD_HD inline double rs_candidate(const double *v, const double *acc, const double *amax, int D, double rate2,
                                    int c) {
  const int cj = c >> 1;
  return rs_candidate_of(v, acc, amax, D, rate2, v[cj], acc[cj], amax[cj], (c & 1) != 0);
}

// One backward step from sample i (t_cur) to i - 1 (t_prev) with the chosen d: returns
// next_rate_squared; *rate = sqrt(min(next, 1)), *dt_new the rescaled time step.
TPAMD_HD inline double rs_step(double rate2, double d, double t_cur, double t_prev, double *rate, double *dt_new) {
  const double udt = t_cur - t_prev;
  const double next = rate2 - d * udt;
  const double clamped = (1.0 < next) ? 1.0 : next;
  const double sc = sqrt(clamped);
  *dt_new = 2.0 * udt / (sqrt(rate2) + sc);
  *rate = sc;
  return next;
}

// The velocity match of a stop that uses every sample (:333-349): GetVelocityAtTime(front_time)
// on the whole trajectory against the segment's first velocity. kRsOk, kRsNotFound, or the
// bracket's status.
TPAMD_HD inline int rs_match(const double *t, int n, const double *qd, int D, double front_time,
                             const double *front_v) {
  int l = 0, u = 0;
  const int st = tb_bracket(t, n, front_time, &l, &u);
  if (st != kRdOk) return st;
  double v[kRsMaxDofs];
  tb_interpolate(qd, l, u, D, tb_fraction(t, l, u, front_time), v);
  double err = 0.0;
  for (int j = 0; j < D; j++) {
    const double e = fabs(v[j] - front_v[j]);
    err = e > err ? e : err;
  }
  return err > 1e-2 ? kRsNotFound : kRsOk;
}

// InsertSegment's kept count (:70-118) for a segment starting at `front`: the first sample with
// front <= time (upper_bound with a <= b), one less if the sample before it is within tol.
TPAMD_HD inline int rs_kept_count(const double *t, int n, double front, double tol) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t[mid] < front) lo = mid + 1; else hi = mid;
  }
  if (n <= 0 || lo == 0) return 0;
  if (front - t[lo - 1] < tol) lo--;
  return lo;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// The whole stop of one trajectory, composed from the parts above with one candidate after the
// other (the kernel runs the candidates on a lane group): time [n], qd / qdd [n][D] (D <= 16),
// max_acceleration [D]; stop at index `stop_index` if by_index, else before time_sec. Returns the
// status; *keep, *first, *last as tpamd_stop_trajectories_* gives them, and rows [first, last] of
// o_time [n], o_qd / o_qdd [n][D] (nothing else is written).
inline int rs_stop_serial(const double *t, const double *qd, const double *qdd, int n, int D, const double *amax,
                          double time_step, bool by_index, int stop_index, double time_sec, int *keep, int *first,
                          int *last, double *o_time, double *o_qd, double *o_qdd) {
  *keep = n; *first = n; *last = n - 1;
  int index = stop_index, st = kRsOk;
  if (!by_index) {
    st = rs_index_for_time(t, n, time_sec, &index);
    if (st == kRsOk && index < 0) return kRsOk;
  }
  if (st == kRsOk) st = rs_check_args(index, n, amax, D, time_step);
  if (st != kRsOk) return st;
  if (rs_last_at_rest(index, n, qd + (size_t)(n - 1) * D, D)) {
    *keep = n - 1; *first = *last = n - 1;
    o_time[n - 1] = t[n - 1];
    for (int j = 0; j < D; j++) o_qd[(size_t)(n - 1) * D + j] = o_qdd[(size_t)(n - 1) * D + j] = 0.0;
    return kRsOk;
  }
  if (!rs_increasing(t, 0, index)) return kRsInvalidArgument;
  if (rs_at_rest(qd + (size_t)index * D, D)) return kRsInternal;
  for (int pass = 0; pass < 2; pass++) {
    double rate2 = 0.0, rt = 0.0, vf[kRsMaxDofs] = {0.0}, offset = 0.0;
    int lo = 1;                        // pass 0: until next >= 1 or sample 2; pass 1: the rows found
    if (pass == 1) {
      lo = *first;
      offset = o_time[*last];          // parked there by pass 0
      o_time[index] = 0.0 + offset;
      for (int j = 0; j < D; j++) o_qd[(size_t)index * D + j] = o_qdd[(size_t)index * D + j] = 0.0;
    }
    int m = 1;
    for (int i = index; i > lo; --i) {
      const double *v = qd + (size_t)i * D, *acc = qdd + (size_t)i * D;
      double d = 0.0;
      for (int c = 0; c < 2 * D; c++) {
        const double x = rs_candidate(v, acc, amax, D, rate2, c);
        d = x < d ? x : d;
      }
      double rate, dtn;
      const double next = rs_step(rate2, d, t[i], t[i - 1], &rate, &dtn);
      rt = rt - dtn;
      m++;
      for (int j = 0; j < D; j++) vf[j] = rate * v[j];
      if (pass == 1) {
        o_time[i - 1] = rt + offset;
        for (int j = 0; j < D; j++) {
          o_qd[(size_t)(i - 1) * D + j] = vf[j];
          o_qdd[(size_t)(i - 1) * D + j] = acc[j] * rate2 + 0.5 * v[j] * d;
        }
      }
      if (pass == 0 && next >= 1.0) break;
      rate2 = next;
    }
    if (pass == 1) break;
    const int f = index + 1 - m;
    offset = t[f] - rt;
    const double front = rt + offset;
    if (!rs_front_finite(front)) return kRsInternal;
    if (m == index) {
      const int mst = rs_match(t, n, qd, D, front, vf);
      if (mst != kRsOk) return mst;
    }
    *keep = rs_kept_count(t, n, front, kRsTolerance);
    *first = f; *last = index;
    o_time[index] = offset;
  }
  return kRsOk;
}
#endif

#if defined(__HIPCC__) || defined(__HIP__)
// ------------------------------------------------------------------ the stop kernels
struct StopTrajParams {
  int Q, B, stride;                      // queries, rows, samples per row
  int mode;                              // kRsBatch, kRsSetFind, kRsSetWrite
  const double *time, *q, *qd, *qdd;     // [B][stride], [B][stride][D]
  const int *count;                      // [B] samples per row, clamped to [0, stride] (null: stride)
  const int *first;                      // [B] first sample of the row (null: 0) -- planner sets
  const int *ids;                        // [Q] row of query k (null: k); outside [0, B): invalid
  const double *amax;                    // [Q][D]
  double time_step;
  const double *stop_sec;                // [Q] StopBeforeTime, or
  const long long *stop_ns;              // [Q] in nanoseconds (planner sets: TimeToSec), or
  const int *stop_index;                 // [Q] StopAtIndex
  int *status, *keep, *seg_first, *seg_last;   // [Q]
  double *seg_offset;                    // [Q] time shift of the segment (planner sets)
  long long *seg_len;                    // [Q] rows of the segment, 0 unless OK (planner sets)
  const long long *offsets;              // [Q + 1] packed rows of the segments (kRsSetWrite)
  long long capacity;
  double *o_time, *o_q, *o_qd, *o_qdd;   // kRsBatch: [B][stride](D) at the input's rows (no o_q);
                                         // kRsSetWrite: packed rows offsets[k] .. (any may be null)
};

// kRsBatch: find the segment, then write it at the input's rows (tpamd_stop_trajectories_*).
// kRsSetFind: find the segment only; kRsSetWrite: write it (q included) at the packed rows.
enum { kRsBatch = 0, kRsSetFind = 1, kRsSetWrite = 2 };

// Group minimum of values that are 0 or negative (never -0, never NaN: see rs_candidate), so the
// order the lanes are combined in does not matter.
template <int L>
__device__ __forceinline__ double rs_group_min(double x) {
#pragma unroll
  for (int o = L / 2; o >= 1; o >>= 1) {
    const double other = __shfl_xor(x, o, 64);
    x = (other < x) ? other : x;
  }
  return x;
}

template <int D>
__global__ __launch_bounds__(64) void k_stop_trajectories(StopTrajParams p) {
  constexpr int L = stop_group_lanes(D);
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & (L - 1);
  const int k = blockIdx.x * G + (int)(threadIdx.x / L);
  if (k >= p.Q) return;                  // the whole group leaves together
  const bool writer = lane == 0;
  const int mode = p.mode;
  if (mode == kRsSetWrite && (p.offsets[p.Q] > p.capacity || p.seg_len[k] == 0)) return;
  const int row = p.ids ? p.ids[k] : k;
  if (row < 0 || row >= p.B) {
    if (writer) {
      p.status[k] = kRsInvalidArgument;
      p.keep[k] = 0; p.seg_first[k] = 0; p.seg_last[k] = -1;
      if (p.seg_len) p.seg_len[k] = 0;
    }
    return;
  }
  const size_t rbase = (size_t)row * p.stride + (p.first ? p.first[row] : 0);
  const int n = p.count ? min(max(p.count[row], 0), p.stride) : p.stride;
  const double *tm = p.time + rbase, *qd = p.qd + rbase * D, *qdd = p.qdd + rbase * D;
  double a[D];
#pragma unroll
  for (int j = 0; j < D; j++) a[j] = p.amax[(size_t)k * D + j];
  // this lane's candidate: joint cj, sign of the limit term
  const bool has_cand = lane < 2 * D;
  const int cj = has_cand ? (lane >> 1) : 0;
  const bool plus = (lane & 1) != 0;
  const double a_c = p.amax[(size_t)k * D + cj];

  int index, first, st = kRsOk, keep = n;
  double offset;
  if (mode == kRsSetWrite) {
    index = p.seg_last[k];
    first = p.seg_first[k];
    offset = p.seg_offset[k];
  } else {
    first = n;
    offset = 0.0;
    bool empty = false;
    if (p.stop_index) {
      index = p.stop_index[k];
    } else {
      const double ts = p.stop_ns ? pset_time_to_sec(p.stop_ns[k]) : p.stop_sec[k];
      st = rs_index_for_time(tm, n, ts, &index);
      empty = st == kRsOk && index < 0;              // no samples: OK, nothing changes
    }
    if (empty) {
      keep = 0; first = 0; index = -1;
    } else if (st == kRsOk) {
      st = rs_check_args(index, n, a, D, p.time_step);
      const bool last_rest = st == kRsOk && rs_last_at_rest(index, n, qd + (size_t)(n - 1) * D, D);
      if (last_rest) {
        keep = n - 1; first = n - 1; offset = tm[n - 1];      // one rest row at the last time
      } else if (st == kRsOk) {
        // times strictly increasing up to index: lane-strided, then the group's AND
        int ok = 1;
        for (int i = lane; i < index; i += L) ok &= tm[i + 1] > tm[i];
#pragma unroll
        for (int o = L / 2; o >= 1; o >>= 1) ok &= __shfl_xor(ok, o, 64);
        if (!ok) st = kRsInvalidArgument;
        else if (rs_at_rest(qd + (size_t)index * D, D)) st = kRsInternal;
      }
      if (st == kRsOk && !last_rest) {
        // pass 1: the segment's length, shift, match and kept count
        double v[D], acc[D], vf[D];
#pragma unroll
        for (int j = 0; j < D; j++) { v[j] = qd[(size_t)index * D + j]; acc[j] = qdd[(size_t)index * D + j]; vf[j] = 0.0; }
        double v_c = qd[(size_t)index * D + cj], acc_c = qdd[(size_t)index * D + cj];
        double t_cur = tm[index], rate2 = 0.0, rt = 0.0;
        int m = 1;
        for (int i = index; i > 1; --i) {
          // sample i - 1 is loaded before sample i is worked on
          double vn[D], accn[D];
#pragma unroll
          for (int j = 0; j < D; j++) { vn[j] = qd[(size_t)(i - 1) * D + j]; accn[j] = qdd[(size_t)(i - 1) * D + j]; }
          const double vn_c = qd[(size_t)(i - 1) * D + cj], accn_c = qdd[(size_t)(i - 1) * D + cj];
          const double t_prev = tm[i - 1];
          const double d =
              rs_group_min<L>(has_cand ? rs_candidate_of(v, acc, a, D, rate2, v_c, acc_c, a_c, plus) : 0.0);
          double rate, dtn;
          const double next = rs_step(rate2, d, t_cur, t_prev, &rate, &dtn);
          rt = rt - dtn;
          m++;
#pragma unroll
          for (int j = 0; j < D; j++) vf[j] = rate * v[j];
          if (next >= 1.0) break;
          rate2 = next;
#pragma unroll
          for (int j = 0; j < D; j++) { v[j] = vn[j]; acc[j] = accn[j]; }
          v_c = vn_c; acc_c = accn_c; t_cur = t_prev;
        }
        first = index + 1 - m;
        offset = tm[first] - rt;
        const double front = rt + offset;
        if (!rs_front_finite(front)) st = kRsInternal;
        else if (m == index) st = rs_match(tm, n, qd, D, front, vf);
        if (st == kRsOk) keep = rs_kept_count(tm, n, front, kRsTolerance);
        else first = n;
      }
    }
    if (st != kRsOk) keep = n, first = n, index = n - 1;
    if (writer) {
      p.status[k] = st;
      p.keep[k] = keep; p.seg_first[k] = first; p.seg_last[k] = index;
      if (p.seg_len) p.seg_len[k] = index - first + 1;
      if (p.seg_offset) p.seg_offset[k] = offset;
    }
    if (mode == kRsSetFind || st != kRsOk || index < first) return;
  }

  // pass 2: the rows [first, index] with their final times; the rest row at index
  const long long obase = mode == kRsSetWrite ? p.offsets[k] - first : (long long)rbase;
  {
    const size_t o = (size_t)(obase + index);
    if (writer && p.o_time) p.o_time[o] = 0.0 + offset;
    if (lane < D) {
      if (p.o_qd) p.o_qd[o * D + lane] = 0.0;
      if (p.o_qdd) p.o_qdd[o * D + lane] = 0.0;
      if (p.o_q) p.o_q[o * D + lane] = p.q[(rbase + index) * D + lane];
    }
  }
  double v[D], acc[D];
#pragma unroll
  for (int j = 0; j < D; j++) { v[j] = qd[(size_t)index * D + j]; acc[j] = qdd[(size_t)index * D + j]; }
  double v_c = qd[(size_t)index * D + cj], acc_c = qdd[(size_t)index * D + cj];
  double t_cur = tm[index], rate2 = 0.0, rt = 0.0;
  for (int i = index; i > first; --i) {
    double vn[D], accn[D];
#pragma unroll
    for (int j = 0; j < D; j++) { vn[j] = qd[(size_t)(i - 1) * D + j]; accn[j] = qdd[(size_t)(i - 1) * D + j]; }
    const double vn_c = qd[(size_t)(i - 1) * D + cj], accn_c = qdd[(size_t)(i - 1) * D + cj];
    const double t_prev = tm[i - 1];
    const double qn = (p.o_q && lane < D) ? p.q[(rbase + i - 1) * D + lane] : 0.0;
    const double d = rs_group_min<L>(has_cand ? rs_candidate_of(v, acc, a, D, rate2, v_c, acc_c, a_c, plus) : 0.0);
    double rate, dtn;
    const double next = rs_step(rate2, d, t_cur, t_prev, &rate, &dtn);
    rt = rt - dtn;
    const size_t o = (size_t)(obase + i - 1);
    if (writer && p.o_time) p.o_time[o] = rt + offset;
    // lane j writes joint j of the row; the values are the same on every lane
#pragma unroll
    for (int j = 0; j < D; j++)
      if (lane == j) {
        if (p.o_qd) p.o_qd[o * D + j] = rate * v[j];
        if (p.o_qdd) p.o_qdd[o * D + j] = acc[j] * rate2 + 0.5 * v[j] * d;
      }
    if (p.o_q && lane < D) p.o_q[o * D + lane] = qn;
    rate2 = next;
#pragma unroll
    for (int j = 0; j < D; j++) { v[j] = vn[j]; acc[j] = accn[j]; }
    v_c = vn_c; acc_c = accn_c; t_cur = t_prev;
  }
}

// One launch for Q queries with D joints (1..16); false: D out of range.
inline bool launch_stop_trajectories(int D, const StopTrajParams &p, hipStream_t st) {
  if (p.Q <= 0) return true;
  switch (D) {
#define TPAMD_RS_CASE(DD)                                                                        \
  case DD: {                                                                                     \
    constexpr int G = 64 / stop_group_lanes(DD);                                                 \
    hipLaunchKernelGGL(k_stop_trajectories<DD>, dim3((unsigned)((p.Q + G - 1) / G)), dim3(64), 0, st, p); \
    return true;                                                                                 \
  }
    TPAMD_RS_CASE(1) TPAMD_RS_CASE(2) TPAMD_RS_CASE(3) TPAMD_RS_CASE(4)
    TPAMD_RS_CASE(5) TPAMD_RS_CASE(6) TPAMD_RS_CASE(7) TPAMD_RS_CASE(8)
    TPAMD_RS_CASE(9) TPAMD_RS_CASE(10) TPAMD_RS_CASE(11) TPAMD_RS_CASE(12)
    TPAMD_RS_CASE(13) TPAMD_RS_CASE(14) TPAMD_RS_CASE(15) TPAMD_RS_CASE(16)
#undef TPAMD_RS_CASE
    default: return false;
  }
}

// offsets[k] = seg_len[0] + .. + seg_len[k - 1], offsets[Q] the total: one workgroup of
// kScanThreads, as k_pset_scan_offsets.
static __global__ void __launch_bounds__(kScanThreads) k_stop_scan_offsets(int Q, const long long *len,
                                                                           long long *offsets) {
  __shared__ long long part[kScanThreads];
  const int t = threadIdx.x;
  const int per = (Q + kScanThreads - 1) / kScanThreads;
  const int lo = min(Q, t * per), hi = min(Q, lo + per);
  long long sum = 0;
  for (int k = lo; k < hi; k++) sum += len[k];
  part[t] = sum;
  __syncthreads();
  for (int s = 1; s < kScanThreads; s <<= 1) {
    const long long add = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long run = part[t] - sum;
  for (int k = lo; k < hi; k++) {
    offsets[k] = run;
    run += len[k];
  }
  if (t == kScanThreads - 1) offsets[Q] = part[t];
}
#endif

}  // namespace tpamd

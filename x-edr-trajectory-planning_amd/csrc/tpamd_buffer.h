// tpamd_buffer.h -- buffer sets (include/tpamd.h tpamd_buffer_set_*): B TrajectoryBuffers
// (trajectory_buffer.{h,cc}) of D joints whose samples, sample count and sequence number stay on
// the device. Every operation of TrajectoryBuffer runs for a list of buffers in one launch and
// leaves each listed buffer as the host mirror (host/trajectory_buffer.cc) would, bit for bit.
//
// State per buffer b: first[b], count[b], sequence[b] and rows [cap] of time, [cap][D] of q, qd,
// qdd; the samples are rows first .. first + count - 1. DiscardSegmentBefore never moves a
// sample: it advances `first` (and writes at most one interpolated row). Room at the tail comes
// back when a call needs it: an insert or append whose result would end behind row cap first
// moves the kept rows to row 0 (compaction, inside the same kernel); a buffer that is replaced as
// a whole restarts at row 0 for free. A result of more than cap rows is TPAMD_PLAN_MORE and the
// buffer is unchanged.
//
//   bs_plan_insert / bs_plan_append   InsertSegment's search, kept count and sequence number
//                                     (:79-133), AppendSample's check (:135-149), and where the
//                                     rows go
//   bs_discard                        DiscardSegmentBefore (:151-208)
//   bs_stop_in_place<D>               StopBeforeTime / StopAtIndex (:296-385) that changes the
//                                     buffer, composed from the stop core of tpamd_rescale.h
//   bs_positions_up_to, bs_start_ns, bs_end_ns   GetPositionsUpToTime (:210-226), GetStartTime,
//                                     GetEndTime (:50-62)
//
// All of these compile for the host as well (TPAMD_HD): tests/cpp/test_buffer_core.cc drives them
// through random operation sequences next to a mirror TrajectoryBuffer. The kernels below add only
// the row copies. Interpolation and brackets are tb_bracket / tb_fraction / tb_interpolate of
// tpamd_readout.h; sample_at_ticks and the packed download run that header's kernels on a view of
// the buffer set, whose layout is that of a planner set's resident trajectories.
#pragma once

#include <math.h>
#include <stdint.h>

#include "tpamd_rescale.h"       // TPAMD_HD, the stop core, tb_bracket / tb_interpolate

namespace tpamd {

// TPAMD_PLAN_* (include/tpamd.h) of a buffer operation
enum { kBsOk = 0, kBsInvalidArgument = 3, kBsMore = 100 };

// One buffer of a set: its scalars and row 0 of its rows
struct BufRef {
  int *first, *count, *sequence;
  double *time, *q, *qd, *qdd;
  int cap, D;
  double tol;                      // TrajectoryBufferOptions::timestep_tolerance
};

// Where an insert or append puts its rows: the buffer becomes rows [first, first + count), of
// which the first `keep` are the kept samples (moved from the old first if move > 0) and the
// rest the new rows. status != kBsOk: nothing changes.
struct InsertPlan {
  int status, keep, first, count, sequence, move;
};

// InsertSegment of n rows starting at time `front` (unused for n == 0) into samples t [count]
// (t = time + first). The sequence number goes up first; an empty segment ends there; the buffer
// is replaced as a whole (sequence 0) if it is empty or no sample is before `front`; otherwise
// the kept count is rs_kept_count (upper_bound with <=, one less within the tolerance).
TPAMD_HD inline InsertPlan bs_plan_insert(const double *t, int first, int count, int sequence, int cap, double tol,
                                          long long n, double front) {
  InsertPlan r = {kBsOk, count, first, count, sequence, 0};
  if (n < 0) { r.status = kBsInvalidArgument; return r; }
  if (n == 0) { r.sequence = sequence + 1; return r; }
  const bool whole = count <= 0 || !(t[0] < front);
  const int keep = whole ? 0 : rs_kept_count(t, count, front, tol);
  if ((long long)keep + n > (long long)cap) { r.status = kBsMore; return r; }
  r.keep = keep;
  r.count = keep + (int)n;
  r.sequence = whole ? 0 : sequence + 1;
  if (keep == 0) r.first = 0;
  else if (first + r.count > cap) { r.first = 0; r.move = keep; }
  return r;
}

// AppendSample at `time`: InvalidArgument unless it is after the last sample; the sequence number
// stays.
TPAMD_HD inline InsertPlan bs_plan_append(const double *t, int first, int count, int sequence, int cap, double time) {
  InsertPlan r = {kBsOk, count, first, count, sequence, 0};
  if (count > 0 && t[count - 1] >= time) { r.status = kBsInvalidArgument; return r; }
  if (count + 1 > cap) { r.status = kBsMore; return r; }
  r.count = count + 1;
  if (count <= 0) { r.first = 0; r.keep = 0; }
  else if (first + r.count > cap) { r.first = 0; r.move = count; }
  return r;
}

// What a discard did (the test counts them)
enum { kBsDiscardEmpty = 0, kBsDiscardBeforeFront, kBsDiscardCleared, kBsDiscardOnSample, kBsDiscardCloseBefore,
       kBsDiscardInterpolated };

// DiscardSegmentBefore(time_sec): advances first / lowers count, and writes the interpolated
// state at time_sec into the new first row where the reference does. Returns the kBsDiscard* case.
TPAMD_HD inline int bs_discard(const BufRef &r, double time_sec) {
  const int first = *r.first, n = *r.count, D = r.D;
  double *t = r.time + first;
  if (n <= 0) return kBsDiscardEmpty;
  if (time_sec <= t[0]) return kBsDiscardBeforeFront;
  if (time_sec > t[n - 1]) {                     // Clear()
    *r.first = 0; *r.count = 0; *r.sequence = 0;
    return kBsDiscardCleared;
  }
  int lo = 0, hi = n;                            // the first sample at or after time_sec
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t[mid] < time_sec) lo = mid + 1; else hi = mid;
  }
  int offset = lo;
  if (offset <= 0) return kBsDiscardBeforeFront;
  if (offset >= n) offset = n - 1;               // unsorted times only: keeps the reads inside the samples
  const bool close = time_sec - t[offset - 1] <= r.tol;
  const bool interpolate = fabs(t[offset] - time_sec) > r.tol;
  if (close || interpolate) --offset;
  if (interpolate) {
    int l = 0, u = 0;
    if (tb_bracket(t, n, time_sec, &l, &u) == kRdOk) {
      const double at = tb_fraction(t, l, u, time_sec);
      double a[kRsMaxDofs], b[kRsMaxDofs], c[kRsMaxDofs];
      tb_interpolate(r.q + (size_t)first * D, l, u, D, at, a);
      tb_interpolate(r.qd + (size_t)first * D, l, u, D, at, b);
      tb_interpolate(r.qdd + (size_t)first * D, l, u, D, at, c);
      t[offset] = time_sec;
      for (int d = 0; d < D; d++) {
        r.q[(size_t)(first + offset) * D + d] = a[d];
        r.qd[(size_t)(first + offset) * D + d] = b[d];
        r.qdd[(size_t)(first + offset) * D + d] = c[d];
      }
    }
  }
  *r.first = first + offset;
  *r.count = n - offset;
  return interpolate ? kBsDiscardInterpolated : close ? kBsDiscardCloseBefore : kBsDiscardOnSample;
}

// GetPositionsUpToTime as a row count: the samples before the bracket of time_sec; 0 outside.
TPAMD_HD inline int bs_positions_up_to(const double *t, int n, double time_sec) {
  if (n <= 0 || time_sec < t[0] || time_sec > t[n - 1]) return 0;
  int lo = 0, hi = n;                            // upper_bound
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (t[mid] <= time_sec) lo = mid + 1; else hi = mid;
  }
  return lo - 1;
}

// GetStartTime / GetEndTime in nanoseconds (TimeFromSec truncates seconds * 1e9); without samples
// TimeFromSec(0) and absl::Time(), both 0.
TPAMD_HD inline long long bs_start_ns(const double *t, int n) { return n <= 0 ? 0 : (long long)(t[0] * 1e9); }
TPAMD_HD inline long long bs_end_ns(const double *t, int n) { return n <= 0 ? 0 : (long long)(t[n - 1] * 1e9); }

// rows [from, from + n) of one buffer to [to, to + n), one row after the other in an order that
// is safe when the ranges overlap
TPAMD_HD inline void bs_move_rows_serial(const BufRef &r, int from, int to, int n) {
  if (from == to || n <= 0) return;
  const int D = r.D;
  for (int s = 0; s < n; s++) {
    const int i = to < from ? s : n - 1 - s;
    r.time[to + i] = r.time[from + i];
    for (int d = 0; d < D; d++) {
      r.q[(size_t)(to + i) * D + d] = r.q[(size_t)(from + i) * D + d];
      r.qd[(size_t)(to + i) * D + d] = r.qd[(size_t)(from + i) * D + d];
      r.qdd[(size_t)(to + i) * D + d] = r.qdd[(size_t)(from + i) * D + d];
    }
  }
}

// What a successful stop did to the sequence number (the test counts them)
enum { kBsStopNothing = 0, kBsStopRestOnLast = 1, kBsStopInserted = 2 };

// StopBeforeTime(time_sec, amax, time_step), or StopAtIndex(stop_index, ...) if by_index, that
// changes the buffer: the status; on kRsOk the samples from keep on are the rescaled tail (rows
// [index + 1 - m, index] rescaled where they stand and then moved down to row keep if keep is
// before them, or written straight at row keep if it is behind their first row, whose sample is
// kept then), and count / sequence follow InsertSegment. A stop that fails changes nothing; so the
// segment is found first without a write (pass 0) and written in a second pass, as
// rs_stop_serial does. Writing in place, sample i - 1 is read before row i - 1 is written.
// kBsMore only if the segment's front time lies more than the tolerance behind the sample it was
// computed from (keep beyond that sample) on a buffer without room: that takes a tolerance below
// the rounding of a time stamp (1e-6 s and stamps of 2^34 s, tests/stop_reference.py "late_clock").
template <int D>
TPAMD_HD inline int bs_stop_in_place(const BufRef &r, bool by_index, int stop_index, double time_sec,
                                     const double *amax_in, double time_step, int *what) {
  *what = kBsStopNothing;
  const int first = *r.first, n = *r.count;
  double *t = r.time + first, *qd = r.qd + (size_t)first * D, *qdd = r.qdd + (size_t)first * D;
  double amax[D];
  for (int j = 0; j < D; j++) amax[j] = amax_in[j];
  int index = stop_index, st = kRsOk;
  if (!by_index) {
    st = rs_index_for_time(t, n, time_sec, &index);
    if (st == kRsOk && index < 0) return kRsOk;
  }
  if (st == kRsOk) st = rs_check_args(index, n, amax, D, time_step);
  if (st != kRsOk) return st;
  if (rs_last_at_rest(index, n, qd + (size_t)(n - 1) * D, D)) {
    for (int j = 0; j < D; j++) qd[(size_t)(n - 1) * D + j] = qdd[(size_t)(n - 1) * D + j] = 0.0;
    *what = kBsStopRestOnLast;
    return kRsOk;
  }
  if (!rs_increasing(t, 0, index)) return kRsInvalidArgument;
  if (rs_at_rest(qd + (size_t)index * D, D)) return kRsInternal;

  int m = 1, keep = 0, f = index;
  double offset = 0.0;
  bool whole = false;
  for (int pass = 0; pass < 2; pass++) {
    double v[D], acc[D], vf[D];
    for (int j = 0; j < D; j++) { v[j] = qd[(size_t)index * D + j]; acc[j] = qdd[(size_t)index * D + j]; vf[j] = 0.0; }
    double t_cur = t[index], rate2 = 0.0, rt = 0.0;
    const int lo = pass == 0 ? 1 : f;
    // A segment that goes behind its own first sample (keep > f) is written where it belongs: row
    // i - 1 + up is at or behind sample i, which is in registers by then, and samples [f, keep)
    // stay as they are. One that goes before it (keep < f) is written in place and moved after.
    const int up = (pass == 1 && keep > f) ? keep - f : 0;
    if (pass == 1) {
      t[index + up] = 0.0 + offset;
      for (int j = 0; j < D; j++) {
        qd[(size_t)(index + up) * D + j] = qdd[(size_t)(index + up) * D + j] = 0.0;
        if (up) r.q[(size_t)(first + index + up) * D + j] = r.q[(size_t)(first + index) * D + j];
      }
    }
    int rows = 1;
    for (int i = index; i > lo; --i) {
      double vn[D], accn[D];
      for (int j = 0; j < D; j++) { vn[j] = qd[(size_t)(i - 1) * D + j]; accn[j] = qdd[(size_t)(i - 1) * D + j]; }
      const double t_prev = t[i - 1];
      double d = 0.0;
      for (int c = 0; c < 2 * D; c++) {
        const double x = rs_candidate(v, acc, amax, D, rate2, c);
        d = x < d ? x : d;
      }
      double rate, dtn;
      const double next = rs_step(rate2, d, t_cur, t_prev, &rate, &dtn);
      rt = rt - dtn;
      rows++;
      for (int j = 0; j < D; j++) vf[j] = rate * v[j];
      if (pass == 1) {
        t[i - 1 + up] = rt + offset;
        for (int j = 0; j < D; j++) {
          qd[(size_t)(i - 1 + up) * D + j] = vf[j];
          qdd[(size_t)(i - 1 + up) * D + j] = acc[j] * rate2 + 0.5 * v[j] * d;
          if (up) r.q[(size_t)(first + i - 1 + up) * D + j] = r.q[(size_t)(first + i - 1) * D + j];
        }
      }
      if (pass == 0 && next >= 1.0) break;
      rate2 = next;
      for (int j = 0; j < D; j++) { v[j] = vn[j]; acc[j] = accn[j]; }
      t_cur = t_prev;
    }
    if (pass == 1) break;
    m = rows;
    f = index + 1 - m;
    offset = t[f] - rt;
    const double front = rt + offset;
    if (!rs_front_finite(front)) return kRsInternal;
    if (m == index) {
      const int mst = rs_match(t, n, qd, D, front, vf);
      if (mst != kRsOk) return mst;
    }
    whole = !(t[0] < front);
    keep = whole ? 0 : rs_kept_count(t, n, front, r.tol);
    if (first + keep + m > r.cap) return kBsMore;
  }
  if (keep < f) bs_move_rows_serial(r, first + f, first + keep, m);
  *r.count = keep + m;
  *r.sequence = whole ? 0 : *r.sequence + 1;
  *what = kBsStopInserted;
  return kRsOk;
}

// bs_stop_in_place<D> for D in 1..16 (kRsInvalidArgument outside)
inline int bs_stop_in_place_any(const BufRef &r, bool by_index, int stop_index, double time_sec, const double *amax,
                                double time_step, int *what) {
  switch (r.D) {
#define TPAMD_BS_CASE(DD) case DD: return bs_stop_in_place<DD>(r, by_index, stop_index, time_sec, amax, time_step, what);
    TPAMD_BS_CASE(1) TPAMD_BS_CASE(2) TPAMD_BS_CASE(3) TPAMD_BS_CASE(4)
    TPAMD_BS_CASE(5) TPAMD_BS_CASE(6) TPAMD_BS_CASE(7) TPAMD_BS_CASE(8)
    TPAMD_BS_CASE(9) TPAMD_BS_CASE(10) TPAMD_BS_CASE(11) TPAMD_BS_CASE(12)
    TPAMD_BS_CASE(13) TPAMD_BS_CASE(14) TPAMD_BS_CASE(15) TPAMD_BS_CASE(16)
#undef TPAMD_BS_CASE
    default: *what = kBsStopNothing; return kRsInvalidArgument;
  }
}

// A planned insert / append carried out by one thread (the kernel copies with a workgroup): the
// kept rows to their place, the n new rows (time [n], q / qd / qdd [n][D]) behind them, the scalars.
inline void bs_apply_serial(const BufRef &r, const InsertPlan &p, int n, const double *time, const double *q,
                            const double *qd, const double *qdd) {
  if (p.status != kBsOk) return;
  if (p.move > 0) bs_move_rows_serial(r, *r.first, 0, p.move);
  const size_t o = (size_t)p.first + p.keep, D = r.D;
  for (int i = 0; i < n; i++) r.time[o + i] = time[i];
  for (size_t i = 0; i < (size_t)n * D; i++) {
    r.q[o * D + i] = q[i];
    r.qd[o * D + i] = qd[i];
    r.qdd[o * D + i] = qdd[i];
  }
  *r.first = p.first; *r.count = p.count; *r.sequence = p.sequence;
}

#if (defined(__HIPCC__) || defined(__HIP__)) && !defined(TPAMD_HD_ROUTINES_ONLY)
// ------------------------------------------------------------------ the buffer-set kernels
struct BufferSetState {
  int B, D, cap;
  double tol;
  int *first, *count, *sequence;       // [B]
  double *time, *q, *qd, *qdd;         // [B][cap], [B][cap][D]
};

__device__ __forceinline__ BufRef bs_ref(const BufferSetState &S, int b) {
  const size_t o = (size_t)b * S.cap;
  return BufRef{S.first + b, S.count + b, S.sequence + b, S.time + o, S.q + o * S.D, S.qd + o * S.D,
                S.qdd + o * S.D, S.cap, S.D, S.tol};
}

enum { kBsFromRows = 0, kBsFromPlanners = 1, kBsAppend = 2 };

struct BufferOpParams {
  BufferSetState S;
  int count;                           // listed buffers
  const int *ids;                      // [count] buffer of entry k; null: k
  int *status;                         // [count] TPAMD_PLAN_* (null: not reported)
  // insert / append
  int source;                          // kBsFromRows, kBsFromPlanners, kBsAppend
  const long long *offsets;            // kBsFromRows: [count + 1], entry k's rows offsets[k] .. offsets[k + 1)
  long long capacity;                  // kBsFromRows: rows the source arrays hold
  const double *i_time, *i_q, *i_qd, *i_qdd;      // [rows], [rows][D]; kBsAppend: row k
  int pB, ptcap;                       // kBsFromPlanners: the planner set's resident trajectories
  const int *planner_ids;              // [count] planner of entry k; null: k
  const int *t_first, *t_count;        // [pB]
  // discard / stop / info / add_offset: one of the two per call
  const long long *time_ns;            // [count] nanoseconds (TimeToSec)
  const double *time_sec;              // [count] seconds
  const double *amax;                  // [count][D]
  double time_step;
  // info
  int *o_count, *o_sequence, *o_up_to; // [count], any may be null
  long long *o_start_ns, *o_end_ns;    // [count], any may be null
};

// the buffer of entry k, or -1 for an id outside the set
__device__ __forceinline__ int bs_buffer(const BufferOpParams &p, int k) {
  const int b = p.ids ? p.ids[k] : k;
  return (b < 0 || b >= p.S.B) ? -1 : b;
}
__device__ __forceinline__ double bs_time_arg(const BufferOpParams &p, int k) {
  return p.time_ns ? pset_time_to_sec(p.time_ns[k]) : p.time_sec[k];
}

constexpr int kBsThreads = 256;

// n doubles from src to dst by the whole workgroup, consecutive lanes on consecutive doubles
// ([rows][D] runs are contiguous on both sides, whatever D is).
__device__ __forceinline__ void bs_copy_wg(double *dst, const double *src, long long n) {
  for (long long i = threadIdx.x; i < n; i += kBsThreads) dst[i] = src[i];
}
// The same within one array towards lower addresses (dst < src), ranges possibly overlapping: a
// chunk of kBsThreads doubles is read by all lanes before any of them writes it, and chunk c's
// writes end below chunk c + 1's reads.
__device__ __forceinline__ void bs_move_down_wg(double *dst, const double *src, long long n) {
  for (long long base = 0; base < n; base += kBsThreads) {
    const long long i = base + threadIdx.x;
    const double x = i < n ? src[i] : 0.0;
    __syncthreads();
    if (i < n) dst[i] = x;
    __syncthreads();
  }
}

// InsertSegment / AppendSample: workgroup k serves entry k. Lane 0 searches and decides
// (bs_plan_insert / bs_plan_append) while the others wait at one barrier; then the workgroup
// compacts the kept rows if the plan says so, copies the new rows, and lane 0 publishes first,
// count and sequence. The sources are read-only here and never a row of the buffer set.
static __global__ void __launch_bounds__(kBsThreads) k_bset_insert(BufferOpParams p) {
  __shared__ InsertPlan plan;
  __shared__ long long s_src, s_n;
  __shared__ int s_b;
  const int k = blockIdx.x;
  if (threadIdx.x == 0) {
    const int b = bs_buffer(p, k);
    long long src = 0, n = 0;
    bool ok = b >= 0;
    if (ok && p.source == kBsFromRows) {
      src = p.offsets[k];
      n = p.offsets[k + 1] - src;
      ok = src >= 0 && n >= 0 && p.offsets[k + 1] <= p.capacity;
    } else if (ok && p.source == kBsAppend) {
      src = k; n = 1;
    } else if (ok) {
      const int pl = p.planner_ids ? p.planner_ids[k] : k;
      ok = pl >= 0 && pl < p.pB;
      if (ok) {
        const int pf = p.t_first[pl];
        n = min(max(p.t_count[pl], 0), p.ptcap);
        src = (long long)pl * p.ptcap + pf;
        ok = pf >= 0 && pf + n <= p.ptcap;
      }
    }
    InsertPlan r = {kBsInvalidArgument, 0, 0, 0, 0, 0};
    if (ok) {
      const BufRef f = bs_ref(p.S, b);
      const int first = *f.first, cnt = *f.count;
      const double front = n > 0 ? p.i_time[src] : 0.0;
      r = p.source == kBsAppend ? bs_plan_append(f.time + first, first, cnt, *f.sequence, f.cap, front)
                                : bs_plan_insert(f.time + first, first, cnt, *f.sequence, f.cap, f.tol, n, front);
    }
    plan = r; s_src = src; s_n = n; s_b = b;
    if (p.status) p.status[k] = r.status;
  }
  __syncthreads();
  if (plan.status != kBsOk) return;    // the whole workgroup
  const BufRef f = bs_ref(p.S, s_b);
  const int D = p.S.D;
  if (plan.move > 0) {
    const size_t from = (size_t)*f.first;           // > 0: a compaction happens only then
    bs_move_down_wg(f.time, f.time + from, plan.move);
    bs_move_down_wg(f.q, f.q + from * D, (long long)plan.move * D);
    bs_move_down_wg(f.qd, f.qd + from * D, (long long)plan.move * D);
    bs_move_down_wg(f.qdd, f.qdd + from * D, (long long)plan.move * D);
  }
  const size_t o = (size_t)plan.first + plan.keep, src = (size_t)s_src;
  bs_copy_wg(f.time + o, p.i_time + src, s_n);
  bs_copy_wg(f.q + o * D, p.i_q + src * D, s_n * D);
  bs_copy_wg(f.qd + o * D, p.i_qd + src * D, s_n * D);
  bs_copy_wg(f.qdd + o * D, p.i_qdd + src * D, s_n * D);
  __syncthreads();                     // every lane has read *f.first
  if (threadIdx.x == 0) { *f.first = plan.first; *f.count = plan.count; *f.sequence = plan.sequence; }
}

// One lane per listed buffer. A discard is a search (log2(samples) dependent loads) and at most
// one row of 3 D + 1 doubles.
static __global__ void __launch_bounds__(64) k_bset_discard(BufferOpParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = bs_buffer(p, k);
  if (b >= 0) bs_discard(bs_ref(p.S, b), bs_time_arg(p, k));
  if (p.status) p.status[k] = b < 0 ? kBsInvalidArgument : kBsOk;
}

// One lane per listed buffer runs bs_stop_in_place<D>: the same code the CPU test holds equal to
// the mirror. A stop is rare and its backward integration is a serial chain over the segment's
// samples either way; the lane-group layout of k_stop_trajectories (candidates across lanes)
// would shorten each step, not the chain.
template <int D>
static __global__ void __launch_bounds__(64) k_bset_stop(BufferOpParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = bs_buffer(p, k);
  int what;
  p.status[k] = b < 0 ? kBsInvalidArgument
                      : bs_stop_in_place<D>(bs_ref(p.S, b), false, 0, bs_time_arg(p, k), p.amax + (size_t)k * D,
                                            p.time_step, &what);
}

inline bool launch_bset_stop(const BufferOpParams &p, hipStream_t st) {
  if (p.count <= 0) return true;
  const dim3 grid((unsigned)((p.count + 63) / 64));
  switch (p.S.D) {
#define TPAMD_BS_CASE(DD) case DD: hipLaunchKernelGGL(k_bset_stop<DD>, grid, dim3(64), 0, st, p); return true;
    TPAMD_BS_CASE(1) TPAMD_BS_CASE(2) TPAMD_BS_CASE(3) TPAMD_BS_CASE(4)
    TPAMD_BS_CASE(5) TPAMD_BS_CASE(6) TPAMD_BS_CASE(7) TPAMD_BS_CASE(8)
    TPAMD_BS_CASE(9) TPAMD_BS_CASE(10) TPAMD_BS_CASE(11) TPAMD_BS_CASE(12)
    TPAMD_BS_CASE(13) TPAMD_BS_CASE(14) TPAMD_BS_CASE(15) TPAMD_BS_CASE(16)
#undef TPAMD_BS_CASE
    default: return false;
  }
}

// AddOffsetToTimestamps: workgroup k adds entry k's offset (seconds, or nanoseconds / 1e9) to the
// time stamps of its buffer.
static __global__ void __launch_bounds__(kBsThreads) k_bset_add_offset(BufferOpParams p) {
  const int k = blockIdx.x;
  const int b = bs_buffer(p, k);
  if (threadIdx.x == 0 && p.status) p.status[k] = b < 0 ? kBsInvalidArgument : kBsOk;
  if (b < 0) return;
  const BufRef f = bs_ref(p.S, b);
  const double offset = p.time_ns ? (double)p.time_ns[k] / 1e9 : p.time_sec[k];
  double *t = f.time + *f.first;
  const int n = *f.count;
  for (int i = threadIdx.x; i < n; i += kBsThreads) t[i] = t[i] + offset;
}

// Clear: one lane per listed buffer
static __global__ void __launch_bounds__(64) k_bset_clear(BufferOpParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = bs_buffer(p, k);
  if (b >= 0) { p.S.first[b] = 0; p.S.count[b] = 0; p.S.sequence[b] = 0; }
  if (p.status) p.status[k] = b < 0 ? kBsInvalidArgument : kBsOk;
}

// GetNumSamples, GetSequenceNumber, GetStartTime, GetEndTime and GetPositionsUpToTime(time) (a
// row count) of each listed buffer; an id outside the set gives zeros and TPAMD_PLAN_INVALID_ARGUMENT.
static __global__ void __launch_bounds__(64) k_bset_info(BufferOpParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = bs_buffer(p, k);
  int n = 0, seq = 0, up = 0;
  long long s = 0, e = 0;
  if (b >= 0) {
    const BufRef f = bs_ref(p.S, b);
    const double *t = f.time + *f.first;
    n = *f.count; seq = *f.sequence;
    s = bs_start_ns(t, n); e = bs_end_ns(t, n);
    if (p.o_up_to && (p.time_ns || p.time_sec)) up = bs_positions_up_to(t, n, bs_time_arg(p, k));
  }
  if (p.o_count) p.o_count[k] = n;
  if (p.o_sequence) p.o_sequence[k] = seq;
  if (p.o_start_ns) p.o_start_ns[k] = s;
  if (p.o_end_ns) p.o_end_ns[k] = e;
  if (p.o_up_to) p.o_up_to[k] = up;
  if (p.status) p.status[k] = b < 0 ? kBsInvalidArgument : kBsOk;
}

// rows of a buffer set to arrays of a larger per-buffer capacity: the samples move to row 0
static __global__ void __launch_bounds__(kBsThreads) k_bset_regrow(BufferSetState o, BufferSetState n) {
  const int b = blockIdx.x;
  const size_t from = (size_t)b * o.cap + o.first[b], to = (size_t)b * n.cap;
  const long long cnt = o.count[b];
  const int D = o.D;
  bs_copy_wg(n.time + to, o.time + from, cnt);
  bs_copy_wg(n.q + to * D, o.q + from * D, cnt * D);
  bs_copy_wg(n.qd + to * D, o.qd + from * D, cnt * D);
  bs_copy_wg(n.qdd + to * D, o.qdd + from * D, cnt * D);
}
static __global__ void k_bset_zero_first(int B, int *first) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) first[b] = 0;
}
#endif

}  // namespace tpamd

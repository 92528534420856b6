// tpamd_stop.h -- the fastest stop along a timed path (include/tpamd.h tpamd_fastest_stop_*,
// tpamd_planner_set_stop_parameters): PathTimingTrajectory::GetPathStopParameter
// (path_timing_trajectory.cc:235-287) with ComputeFastestStop (:75-172) for a batch of paths.
//
// Per path b and query time t_b: the start index is lower_bound(t_b) over time[0 .. count_b)
// (:244); none: "not in timed path range" (:245-249). From that offset the time scaling
// rate2 = (ds/dt)^2, starting at 1, is integrated with the steepest admissible decrease
// d = d(rate2)/ds (:111-157):
//   bias_j = qdd_j * rate2;
//   for every joint c with |qd_c| >= 1e-6, the candidates 2 (-bias_c - a_c) / qd_c and
//   2 (-bias_c + a_c) / qd_c; a candidate d is valid if every joint's bias_j + (0.5 qd_j) d lies
//   in [-a_j, a_j] up to 1e-10; d = min(0, smallest valid candidate);
//   next = max(0, rate2 + dt d); duration += 2 dt / (sqrt(rate2) + sqrt(next)),
// until rate2 > 0 fails or the last sample is reached. The result is the path parameter of the
// sample the loop ends at (:280-286). Starting ON the last sample gives s[count-1] and duration 0,
// which is what the loop gives for one sample (:250-252).
//
// Bit-exactness: every operation is written in the order of the scalar restatement
// (host/fastest_stop.cc); the library is built with -ffp-contract=off, '/' and sqrt are the
// correctly rounded ones, std::min / std::max are written as their comparisons. Non-finite
// inputs (time, qd, qdd, max_acceleration, query time) are outside the contract.
//
// Layout: the recurrence over samples is sequential (bias depends on the previous rate2), so the
// parallelism is across paths and across the 2 D candidates of one sample. A group of
// L = next_pow2(2 D) lanes serves one path (64 / L paths per wave): lane c owns candidate c
// (joint c / 2, sign c & 1) and runs the validity test over the D joints; the group then takes
// the minimum with xor shuffles. Every lane of a group carries the same rate2 / duration, so the
// group leaves the loop together and no broadcast is needed. The loads of sample i + 1 are issued
// before sample i is computed, so that the dependent fp64 chain (divide, check, group minimum,
// update) does not wait on memory.
#pragma once

#include "tpamd_kernels.h"
#include "tpamd_planner_set.h"   // pset_time_to_sec

namespace tpamd {

struct FastestStopParams {
  int Q;                    // queries (paths) of this launch
  int stride;               // samples per row
  const double *time, *s;   // [rows][stride]
  const double *qd, *qdd;   // [rows][stride][D]
  const int *count;         // [rows] samples per row, clamped to [0, stride] (null: stride)
  const int *first;         // [rows] first sample of the row (null: 0) -- planner sets
  const int *initial_plan;  // [rows] 0: no plan yet, the answer is 0.0 (:239-242) (null: all planned)
  const int *ids;           // [Q] row of query k (null: k)
  const double *amax;       // [rows][D]
  const double *query_sec;  // [Q] query time in seconds, or
  const long long *query_ns;// [Q] in nanoseconds (planner sets: TimeToSec, pset_time_to_sec)
  double *stop_s;           // [Q]
  int *stop_index;          // [Q] absolute sample index within the row (may be null)
  double *duration;         // [Q] (may be null)
  int *status;              // [Q] TPAMD_PLAN_*
  double *p_time, *p_rate2, *p_drate2;  // [Q][stride] profile (null: not written)
};

constexpr int stop_group_lanes(int D) {
  int l = 2;
  while (l < 2 * D) l *= 2;
  return l;
}

template <int D>
__global__ __launch_bounds__(64) void k_fastest_stop(FastestStopParams p) {
  constexpr int L = stop_group_lanes(D);
  static_assert(L <= 64, "D <= 32");
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & (L - 1);
  const int k = blockIdx.x * G + (int)(threadIdx.x / L);
  if (k >= p.Q) return;                       // the whole group leaves together
  const int row = p.ids ? p.ids[k] : k;
  const bool writer = lane == 0;
  const double tq = p.query_ns ? pset_time_to_sec(p.query_ns[k]) : p.query_sec[k];
  if (p.initial_plan && !p.initial_plan[row]) {
    if (writer) {
      p.stop_s[k] = 0.0;
      if (p.stop_index) p.stop_index[k] = 0;
      if (p.duration) p.duration[k] = 0.0;
      p.status[k] = kPlanOk;
    }
    return;
  }
  const size_t rbase = (size_t)row * p.stride + (p.first ? p.first[row] : 0);
  const int n = p.count ? min(max(p.count[row], 0), p.stride) : p.stride;   // never past the row
  const double *tm = p.time + rbase;
  // lower_bound (:244)
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (tm[mid] < tq) lo = mid + 1; else hi = mid;
  }
  if (lo >= n) {
    if (writer) {
      p.stop_s[k] = 0.0;
      if (p.stop_index) p.stop_index[k] = -1;
      if (p.duration) p.duration[k] = 0.0;
      p.status[k] = kPlanInvalidArgument;
    }
    return;
  }
  const int off = lo, m = n - off;            // FastestStopTrajectoryView.sample_count
  const double *qd = p.qd + (rbase + off) * D, *qdd = p.qdd + (rbase + off) * D;
  tm += off;
  // this lane's candidate: joint cj, sign of the limit term
  const bool has_cand = lane < 2 * D;
  const int cj = has_cand ? (lane >> 1) : 0;
  const bool plus = (lane & 1) != 0;
  double a[D];
#pragma unroll
  for (int j = 0; j < D; j++) a[j] = p.amax[(size_t)row * D + j];
  const double a_c = p.amax[(size_t)row * D + cj];
  // sample 0
  double v[D], acc[D];
#pragma unroll
  for (int j = 0; j < D; j++) { v[j] = qd[j]; acc[j] = qdd[j]; }
  double v_c = qd[cj], acc_c = qdd[cj], t_cur = tm[0];
  const double t0 = t_cur;
  double rate2 = 1.0, sr = 1.0;              // sr = sqrt(rate2) (sqrt(1) = 1 exactly)
  double drate2 = 0.0, dur = 0.0;
  double *pt = p.p_time ? p.p_time + (size_t)k * p.stride : nullptr;
  double *pr = p.p_rate2 ? p.p_rate2 + (size_t)k * p.stride : nullptr;
  double *pd = p.p_drate2 ? p.p_drate2 + (size_t)k * p.stride : nullptr;
  int i = 0;
  for (; (i < m - 1) && (rate2 > 0.0); i++) {
    // sample i + 1 (i + 1 <= m - 1: in range) is loaded before sample i is worked on
    double vn[D], accn[D];
    const double *qn = qd + (size_t)(i + 1) * D, *qan = qdd + (size_t)(i + 1) * D;
#pragma unroll
    for (int j = 0; j < D; j++) { vn[j] = qn[j]; accn[j] = qan[j]; }
    const double vn_c = qn[cj], accn_c = qan[cj], t_next = tm[i + 1];
    // this lane's candidate (:125-154)
    double cand = 0.0;                       // 0: no candidate below the start value 0
    if (has_cand && !(fabs(v_c) < 1e-6)) {
      const double bias_c = acc_c * rate2;
      const double d = plus ? 2.0 * (-bias_c + a_c) / v_c : 2.0 * (-bias_c - a_c) / v_c;
      bool valid = true;
#pragma unroll
      for (int j = 0; j < D; j++) {
        const double aj = acc[j] * rate2 + (0.5 * v[j]) * d;
        valid = valid && (a[j] - aj >= -1e-10) && (-a[j] - aj <= 1e-10);
      }
      if (valid && d < 0.0) cand = d;
    }
    // Group minimum. The scalar loop starts at 0 and replaces only on strictly less, so the
    // result is the smallest valid candidate below 0, or 0; NaN never replaces. Every lane holds
    // 0 or a value < 0 (never -0), and equal nonzero doubles have equal bits, so the minimum does
    // not depend on the order the lanes are combined in.
#pragma unroll
    for (int o = L / 2; o >= 1; o >>= 1) {
      const double other = __shfl_xor(cand, o, 64);
      cand = (other < cand) ? other : cand;
    }
    const double dr = (0.0 < cand) ? 0.0 : cand;          // std::min(min, 0.0)
    if (writer && pt) { pt[i] = t0 + dur; pr[i] = rate2; pd[i] = dr; }
    // forward Euler (:159-167)
    const double udt = t_next - t_cur;
    const double x = rate2 + udt * dr;
    const double next = (0.0 < x) ? x : 0.0;               // std::max(0.0, x)
    const double sn = sqrt(next);
    dur += 2.0 * udt / (sr + sn);
    rate2 = next;
    sr = sn;
    drate2 = dr;
#pragma unroll
    for (int j = 0; j < D; j++) { v[j] = vn[j]; acc[j] = accn[j]; }
    v_c = vn_c; acc_c = accn_c; t_cur = t_next;
  }
  if (writer) {
    if (pt) { pt[i] = t0 + dur; pr[i] = rate2; pd[i] = drate2; }
    p.stop_s[k] = p.s[rbase + off + i];
    if (p.stop_index) p.stop_index[k] = off + i;
    if (p.duration) p.duration[k] = dur;
    p.status[k] = kPlanOk;
  }
}

// One launch for Q queries with D joints (1..16); false: D out of range.
inline bool launch_fastest_stop(int D, const FastestStopParams &p, hipStream_t st) {
  if (p.Q <= 0) return true;
  switch (D) {
#define TPAMD_STOP_CASE(DD)                                                                      \
  case DD: {                                                                                     \
    constexpr int G = 64 / stop_group_lanes(DD);                                                 \
    hipLaunchKernelGGL(k_fastest_stop<DD>, dim3((unsigned)((p.Q + G - 1) / G)), dim3(64), 0, st, p); \
    return true;                                                                                 \
  }
    TPAMD_STOP_CASE(1) TPAMD_STOP_CASE(2) TPAMD_STOP_CASE(3) TPAMD_STOP_CASE(4)
    TPAMD_STOP_CASE(5) TPAMD_STOP_CASE(6) TPAMD_STOP_CASE(7) TPAMD_STOP_CASE(8)
    TPAMD_STOP_CASE(9) TPAMD_STOP_CASE(10) TPAMD_STOP_CASE(11) TPAMD_STOP_CASE(12)
    TPAMD_STOP_CASE(13) TPAMD_STOP_CASE(14) TPAMD_STOP_CASE(15) TPAMD_STOP_CASE(16)
#undef TPAMD_STOP_CASE
    default: return false;
  }
}

}  // namespace tpamd

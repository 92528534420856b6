// tpamd_readout.h -- reading a planner set's resident trajectories out in bulk
// (include/tpamd.h tpamd_planner_set_sample_at_ticks*, tpamd_planner_set_download_trajectories*):
//   tb_bracket / tb_interpolate  TrajectoryBuffer::GetOffsetBracket (trajectory_buffer.cc:233-251)
//                                and the InterpolateLinear of Get{Position,Velocity,Acceleration}AtTime
//                                (:253-294); shared with the switch (sw_velocity_at_time)
//   k_pset_sample_at_ticks       one lane per (listed planner, tick): one bracket search, then q, qd
//                                and qdd from that bracket
//   k_pset_scan_offsets          exclusive scan of the listed planners' sample counts (one workgroup)
//   k_pset_pack_trajectories     one workgroup per listed planner: its rows, contiguous on both sides
//
// The bracket and the interpolation compile for the host as well (TPAMD_HD):
// tests/cpp/test_readout_interp.cc holds them bit-equal to the mirror's TrajectoryPlanner::Get*AtTime.
// The lerp is a + t (b - a) with t = (time - t_l) / (t_u - t_l), a correctly rounded division, and
// the library is built with -ffp-contract=off, so both sides round alike.
#pragma once

#include <stdint.h>

#ifndef TPAMD_HD
#if defined(__HIPCC__) || defined(__HIP__)
#define TPAMD_HD __host__ __device__
#else
#define TPAMD_HD
#endif
#endif

namespace tpamd {

// TPAMD_PLAN_* (include/tpamd.h) of a readout
enum { kRdOk = 0, kRdFailedPrecondition = 1, kRdOutOfRange = 2, kRdInvalidArgument = 3 };

// TrajectoryBuffer::GetOffsetBracket over time [n]: "No samples." (n == 0), a time outside
// [time[0], time[n - 1]], or the bracket *l, *u by upper_bound. A time at or after the last time
// stamp gives *l == *u == n - 1: that sample. Otherwise time[*l] <= time_sec < time[*u].
TPAMD_HD inline int tb_bracket(const double *time, int n, double time_sec, int *l, int *u) {
  if (n <= 0) return kRdFailedPrecondition;
  if (time_sec < time[0] || time_sec > time[n - 1]) return kRdOutOfRange;
  int lo = 0, hi = n;                            // upper_bound
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (time[mid] <= time_sec) lo = mid + 1; else hi = mid;
  }
  if (lo == n) {
    *l = *u = n - 1;
    return kRdOk;
  }
  *l = lo - 1;
  *u = lo;
  return kRdOk;
}

// The bracket's time fraction (unused when l == u)
TPAMD_HD inline double tb_fraction(const double *time, int l, int u, double time_sec) {
  return l == u ? 0.0 : (time_sec - time[l]) / (time[u] - time[l]);
}

// InterpolateLinear between rows l and u of values [n][D] (lerp a + t (b - a)); l == u: row l.
TPAMD_HD inline void tb_interpolate(const double *values, int l, int u, int D, double at, double *out) {
  if (l == u) {
    for (int d = 0; d < D; d++) out[d] = values[(size_t)l * D + d];
    return;
  }
  for (int d = 0; d < D; d++) {
    const double a = values[(size_t)l * D + d], b = values[(size_t)u * D + d];
    out[d] = a + at * (b - a);
  }
}

// start_ns + j * step_ns, or false if that overflows int64
TPAMD_HD inline bool tb_tick_time(int64_t start_ns, int64_t step_ns, int64_t j, int64_t *out) {
  int64_t off;
  if (__builtin_mul_overflow(j, step_ns, &off)) return false;
  return !__builtin_add_overflow(start_ns, off, out);
}

#if (defined(__HIPCC__) || defined(__HIP__)) && !defined(TPAMD_HD_ROUTINES_ONLY)
// ------------------------------------------------------------------ the readout kernels
struct ReadoutParams {
  int B, D, tcap;                      // planners, joints, trajectory row stride of the set
  int count, num_ticks;                // listed planners; ticks per planner
  const int *ids;                      // [count] planner of entry k; null: k
  const int *t_first, *t_count;        // [B] the resident trajectories: rows t_first .. + t_count
  const double *t_time, *t_s, *t_sd, *t_sdd;      // [B][tcap]
  const double *t_q, *t_qd, *t_qdd;               // [B][tcap][D]
  // sample_at_ticks
  const long long *start_ns;           // [count]
  long long step_ns;
  double *q, *qd, *qdd;                // [count][num_ticks][D], any may be null
  int *status;                         // [count][num_ticks]
  // pack
  long long *offsets;                  // [count + 1]
  long long capacity;
  double *o_time, *o_s, *o_sd, *o_sdd; // [rows], any may be null
  double *o_q, *o_qd, *o_qdd;          // [rows][D], any may be null
};

// the planner of entry k, or -1 for an id outside the set
__device__ __forceinline__ int rd_planner(const ReadoutParams &p, int k) {
  const int b = p.ids ? p.ids[k] : k;
  return (b < 0 || b >= p.B) ? -1 : b;
}

// One lane per (entry k, tick j): TrajectoryBuffer::Get{Position,Velocity,Acceleration}AtTime at
// start_ns[k] + j step_ns on the planner's resident trajectory. A lane's bracket search is about
// log2(samples) dependent loads; its three D-double rows go to [k][j][D], so a wave's rows are
// contiguous. Ticks that are not OK leave q / qd / qdd as they were.
static __global__ void __launch_bounds__(256) k_pset_sample_at_ticks(ReadoutParams p) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)p.count * p.num_ticks) return;
  const int k = (int)(idx / p.num_ticks), j = (int)(idx - (long long)k * p.num_ticks);
  const int b = rd_planner(p, k);
  if (b < 0) { p.status[idx] = kRdInvalidArgument; return; }
  int64_t ns;
  if (!tb_tick_time(p.start_ns[k], p.step_ns, j, &ns)) { p.status[idx] = kRdOutOfRange; return; }
  const size_t o = (size_t)b * p.tcap + p.t_first[b];
  const double *tm = p.t_time + o;
  const double time_sec = (double)ns / 1e9;      // TimeToSec
  int l = 0, u = 0;
  const int st = tb_bracket(tm, p.t_count[b], time_sec, &l, &u);
  p.status[idx] = st;
  if (st != kRdOk) return;
  const double at = tb_fraction(tm, l, u, time_sec);
  const int D = p.D;
  const size_t w = (size_t)idx * D;
  if (p.q) tb_interpolate(p.t_q + o * D, l, u, D, at, p.q + w);
  if (p.qd) tb_interpolate(p.t_qd + o * D, l, u, D, at, p.qd + w);
  if (p.qdd) tb_interpolate(p.t_qdd + o * D, l, u, D, at, p.qdd + w);
}

// offsets[k] = sum of the sample counts of entries 0 .. k-1 (an id outside the set counts 0),
// offsets[count] the total. One workgroup of kScanThreads: each thread sums a run of entries, a
// Hillis-Steele scan over the threads' sums, then each thread writes its run.
constexpr int kScanThreads = 1024;
static __global__ void __launch_bounds__(kScanThreads) k_pset_scan_offsets(ReadoutParams p) {
  __shared__ long long part[kScanThreads];
  const int t = threadIdx.x;
  const int per = (p.count + kScanThreads - 1) / kScanThreads;
  const int lo = min(p.count, t * per), hi = min(p.count, lo + per);
  long long sum = 0;
  for (int k = lo; k < hi; k++) {
    const int b = rd_planner(p, k);
    sum += b < 0 ? 0 : p.t_count[b];
  }
  part[t] = sum;
  __syncthreads();
  for (int s = 1; s < kScanThreads; s <<= 1) {
    const long long add = t >= s ? part[t - s] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  long long run = part[t] - sum;                 // exclusive prefix of this thread's run
  for (int k = lo; k < hi; k++) {
    p.offsets[k] = run;
    const int b = rd_planner(p, k);
    run += b < 0 ? 0 : p.t_count[b];
  }
  if (t == kScanThreads - 1) p.offsets[p.count] = part[t];
}

// Workgroup k copies entry k's rows to packed rows offsets[k] .. offsets[k + 1); nothing at all if
// offsets[count] exceeds the capacity. Row runs are contiguous on both sides (D-wide arrays: n D
// doubles), so the lanes of a wave read and write consecutive doubles.
static __global__ void __launch_bounds__(256) k_pset_pack_trajectories(ReadoutParams p) {
  const int k = blockIdx.x;
  if (p.offsets[p.count] > p.capacity) return;
  const int b = rd_planner(p, k);
  if (b < 0) return;
  const long long dst = p.offsets[k];
  const long long n = p.offsets[k + 1] - dst;
  const size_t src = (size_t)b * p.tcap + p.t_first[b];
  const double *in1[4] = {p.t_time, p.t_s, p.t_sd, p.t_sdd};
  double *out1[4] = {p.o_time, p.o_s, p.o_sd, p.o_sdd};
  for (int a = 0; a < 4; a++) {
    if (!out1[a]) continue;
    for (long long i = threadIdx.x; i < n; i += blockDim.x) out1[a][dst + i] = in1[a][src + i];
  }
  const long long nD = n * p.D;
  const double *inD[3] = {p.t_q, p.t_qd, p.t_qdd};
  double *outD[3] = {p.o_q, p.o_qd, p.o_qdd};
  for (int a = 0; a < 3; a++) {
    if (!outD[a]) continue;
    for (long long i = threadIdx.x; i < nD; i += blockDim.x) outD[a][dst * p.D + i] = inD[a][src * p.D + i];
  }
}
#endif

}  // namespace tpamd

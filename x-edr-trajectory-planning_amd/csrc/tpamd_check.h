// tpamd_check.h -- does a solution keep its constraint rows? (include/tpamd.h tpamd_check_*):
// TimeOptimalPathProfile::SolutionSatisfiesConstraints (time_optimal_path_timing.cc:492-518) for
// every path of a batch, on the rows the matching solve forms.
//
// Per path b, sample i < n_b and row c < C, with sd2 = sol.sd2[b][i] (or sd[b][i]^2) and
// sdd = sol.sdd[b][i]:
//   v = a(i,c) * sdd + b(i,c) * sd2                  two products, one sum (-ffp-contract=off)
//   violated  <=>  v + kTiny < lower || v - kTiny > upper          (rows_valid, tpamd_device.h)
//   excess = max(lower - v, v - upper), NaN if either difference is NaN
// The path's record: the number of violated rows, the largest excess that is not NaN with its
// (sample, row) -- among equal values the smallest flattened index i * C + c -- and the first sample
// with a violated row. A NaN v violates nothing (both comparisons are false) and has no excess.
// A path that is not checked -- its status is not TPAMD_PATH_OK, its sample count lies outside
// [2, stride], or (joint form) it has fewer than 3 control points -- gets -1 / NaN / -1 / -1 / -1.
//
// The rows are those of the solve, formed by the same device functions in the same order:
//   rows form       the caller's arrays
//   joint form      SamplePath as sample_lp_joint_body (knot_span_deg2, basis_ders_deg2, the clamp of
//                   u, the end padding) and k_setup_joint's limits
//   Cartesian form  cw_rows_at (ComputePathDerivatives + ConstraintSetup, tpamd_cartesian_window.h)
//
// Layout: one workgroup of kCheckThreads = 256 threads per path (blockIdx.x = b) loops over the
// path. Every thread keeps its own (count, worst excess, flattened index, first sample); check_merge
// is associative and commutative, so the order in which the wave's xor shuffles, the four waves'
// LDS words and a thread's own trips combine them cannot change the result. Thread 0 stores the
// record. No atomics, no second launch, nothing of the engine's workspace is read or written.
//   rows form: lanes run over the flattened element e = i * C + c, so consecutive lanes read
//   consecutive doubles of a, b, lower, upper; sd2 / sdd of sample e / C come through L1 / L2.
//   joint form: knots, control points and the 2 * 2D limits go to LDS once (the limits are formed
//   in the prologue); one thread per sample evaluates q', q'' and walks the 2D rows.
//   Cartesian form: one thread per sample reads q[i], q[i+1], q[i+2] and J[i] (strided, or through
//   first_row) and walks the 2D + 2 rows.
// The sample loops of the joint and the Cartesian form are check_joint_path / check_cartesian_path,
// shared with the kernels that check the windows of a planner set inside its Plan calls (at the end
// of this file).
#pragma once

#include <limits.h>

#include "tpamd_kernels.h"

namespace tpamd {

constexpr int kCheckThreads = 256;

struct CheckSolution {
  const double *sd2, *sd, *sdd;   // [B][N]; sd is read only without sd2
  const int32_t *status;          // [B] or null: every path is checked
};
struct CheckOutputs {
  int32_t *violations;            // [B]
  double *worst_excess;           // [B] or null, as the three below
  int32_t *worst_sample, *worst_row, *first_sample;
};

struct CheckAcc {
  int count = 0;
  double worst = 0.0;
  int flat = -1;                  // i * C + c of `worst`; -1: no row with an excess yet
  int first = INT_MAX;            // first sample with a violated row; INT_MAX: none
};

__device__ __forceinline__ void check_merge(CheckAcc &a, int count, double worst, int flat, int first) {
  a.count += count;
  if (first < a.first) a.first = first;
  if (flat >= 0 && (a.flat < 0 || worst > a.worst || (worst == a.worst && flat < a.flat))) {
    a.worst = worst;
    a.flat = flat;
  }
}

// one row of sample i, flattened index `flat`
__device__ __forceinline__ void check_row(CheckAcc &acc, double a, double b, double lo, double hi, double sdd,
                                          double sd2, int i, int flat) {
  const double v = a * sdd + b * sd2;
  if (v + kTiny < lo || v - kTiny > hi) check_merge(acc, 1, 0.0, -1, i);
  const double e_lo = lo - v, e_hi = v - hi;
  if (e_lo == e_lo && e_hi == e_hi) check_merge(acc, 0, e_lo > e_hi ? e_lo : e_hi, flat, INT_MAX);
}

__device__ __forceinline__ double check_sd2(const CheckSolution &sol, size_t o) {
  if (sol.sd2) return sol.sd2[o];
  const double sd = sol.sd[o];
  return sd * sd;
}

// The record of a path that is not checked. Every thread of the workgroup takes this way together.
__device__ __forceinline__ void check_store_skipped(int b, const CheckOutputs &out) {
  if (threadIdx.x != 0) return;
  out.violations[b] = -1;
  if (out.worst_excess) out.worst_excess[b] = qnan();
  if (out.worst_sample) out.worst_sample[b] = -1;
  if (out.worst_row) out.worst_row[b] = -1;
  if (out.first_sample) out.first_sample[b] = -1;
}

// Workgroup reduction of the threads' records: true for thread 0, whose `acc` is then the path's.
__device__ __forceinline__ bool check_reduce(CheckAcc &acc) {
  __shared__ double s_worst[kCheckThreads / 64];
  __shared__ int s_int[kCheckThreads / 64][3];
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1)
    check_merge(acc, __shfl_xor(acc.count, off, 64), __shfl_xor(acc.worst, off, 64), __shfl_xor(acc.flat, off, 64),
                __shfl_xor(acc.first, off, 64));
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_worst[wave] = acc.worst;
    s_int[wave][0] = acc.count; s_int[wave][1] = acc.flat; s_int[wave][2] = acc.first;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int w = 1; w < kCheckThreads / 64; w++) check_merge(acc, s_int[w][0], s_worst[w], s_int[w][1], s_int[w][2]);
  return true;
}

// The reduction and the store of the path's five results.
__device__ __forceinline__ void check_store(CheckAcc acc, int b, int C, const CheckOutputs &out) {
  if (!check_reduce(acc)) return;
  out.violations[b] = acc.count;
  if (out.worst_excess) out.worst_excess[b] = acc.flat >= 0 ? acc.worst : qnan();
  if (out.worst_sample) out.worst_sample[b] = acc.flat >= 0 ? acc.flat / C : -1;
  if (out.worst_row) out.worst_row[b] = acc.flat >= 0 ? acc.flat % C : -1;
  if (out.first_sample) out.first_sample[b] = acc.first != INT_MAX ? acc.first : -1;
}

// whether path b is checked, and with how many samples (block-uniform)
__device__ __forceinline__ int check_count(const CheckSolution &sol, const int32_t *ns, int b, int N) {
  if (sol.status && sol.status[b] != 0) return 0;
  return cw_ragged_count(ns ? ns[b] : N, N);
}

// ------------------------------------------------------------------ rows form
// grid = B, block = kCheckThreads. a, bm, lo, hi: [B][N][C].
static __global__ void __launch_bounds__(kCheckThreads)
k_check_rows(int N, int C, const double *a, const double *bm, const double *lo, const double *hi, const int32_t *ns,
             CheckSolution sol, CheckOutputs out) {
  const int b = blockIdx.x;
  const int n = check_count(sol, ns, b, N);
  if (n == 0) {
    check_store_skipped(b, out);
    return;
  }
  const size_t row0 = (size_t)b * N;
  const double *pa = a + row0 * C, *pb = bm + row0 * C, *plo = lo + row0 * C, *phi = hi + row0 * C;
  const int total = n * C;
  // (i, c) of element e, advanced without a division per trip
  const int di = kCheckThreads / C, dc = kCheckThreads % C;
  int i = (int)threadIdx.x / C, c = (int)threadIdx.x % C;
  CheckAcc acc;
  for (int e = threadIdx.x; e < total; e += kCheckThreads) {
    const double va = pa[e], vb = pb[e], vlo = plo[e], vhi = phi[e];
    const double sdd = sol.sdd[row0 + i], sd2 = check_sd2(sol, row0 + i);
    check_row(acc, va, vb, vlo, vhi, sdd, sd2, i, e);
    i += di;
    c += dc;
    if (c >= C) { c -= C; i++; }
  }
  check_store(acc, b, C, out);
}

// The n samples of one joint path against its 2D rows, by the whole workgroup (every thread's own
// record comes back). The path's Pb control points, Pb + 3 knots and D limits are the caller's;
// `lds` is laid out for P_lds >= Pb points (check_joint_lds); the solution's samples start at row0.
__device__ __forceinline__ CheckAcc check_joint_path(double *lds, int n, int D, int Pb, int P_lds, double safety,
                                                     const double *knots_b, const double *cps_b,
                                                     const double *vmax_b, const double *amax_b, double path_start,
                                                     double delta, const CheckSolution &sol, size_t row0) {
  const int tid = threadIdx.x;
  const int C = 2 * D;
  const int Kb = Pb + 3;
  double *s_knots = lds;
  double *s_cp = s_knots + (P_lds + 3);
  double *s_lo = s_cp + (size_t)P_lds * D;
  double *s_hi = s_lo + C;
  for (int k = tid; k < Kb; k += kCheckThreads) s_knots[k] = knots_b[k];
  for (int k = tid; k < Pb * D; k += kCheckThreads) s_cp[k] = cps_b[k];
  // the limit rows, k_setup_joint's arithmetic
  for (int d = tid; d < D; d += kCheckThreads) {
    const double am = amax_b[d], vm = vmax_b[d];
    const double al = am * safety;
    const double na = -am * safety;
    const double v = vm * safety;
    const double vv = v * v;
    s_hi[d] = al;
    s_lo[d] = na;
    s_hi[D + d] = vv;
    s_lo[D + d] = 0.0;
  }
  __syncthreads();
  const double k0 = s_knots[0], kend = s_knots[Kb - 1];
  CheckAcc acc;
  for (int i = tid; i < n; i += kCheckThreads) {
    const double sdd = sol.sdd[row0 + i], sd2 = check_sd2(sol, row0 + i);
    const double parameter = path_start + i * delta;
    if (parameter < kend + delta) {
      double u = parameter;
      if (u < k0) u = k0;
      if (kend < u) u = kend;
      int span = knot_span_deg2(s_knots, Kb, u);
      span = min(max(span, 2), Kb - 4);          // (stays inside the slot whatever the knots hold)
      double ders[3][3];
      basis_ders_deg2(s_knots, span, u, ders);
      const double *p0 = s_cp + (size_t)(span - 2) * D, *p1 = p0 + D, *p2 = p1 + D;
      for (int d = 0; d < D; d++) {
        double v1 = 0.0, v2 = 0.0;
        v1 += ders[1][0] * p0[d]; v1 += ders[1][1] * p1[d]; v1 += ders[1][2] * p2[d];
        v2 += ders[2][0] * p0[d]; v2 += ders[2][1] * p1[d]; v2 += ders[2][2] * p2[d];
        check_row(acc, v1, v2, s_lo[d], s_hi[d], sdd, sd2, i, i * C + d);
        check_row(acc, 0.0, v1 * v1, s_lo[D + d], s_hi[D + d], sdd, sd2, i, i * C + D + d);
      }
    } else {
      // behind the end of the spline: q' = q'' = 0
      for (int d = 0; d < D; d++) {
        check_row(acc, 0.0, 0.0, s_lo[d], s_hi[d], sdd, sd2, i, i * C + d);
        check_row(acc, 0.0, 0.0 * 0.0, s_lo[D + d], s_hi[D + d], sdd, sd2, i, i * C + D + d);
      }
    }
  }
  return acc;
}

// ----------------------------------------------------------------- joint form
// grid = B, block = kCheckThreads. Dynamic LDS: knots[P+3] | control points [P][D] | lim_lo[2D] |
// lim_hi[2D]. knots [B][P+3], control points [B][P][D]; with np, path b uses the first np[b] + 3 and
// np[b] entries of its slot (a count outside [3, P] is not checked).
static __global__ void __launch_bounds__(kCheckThreads)
k_check_joint(int N, int D, int P, double safety, const double *knots_g, const double *cps_g, const double *vmax,
              const double *amax, const double *path_start_g, const double *delta_g, const int32_t *ns,
              const int32_t *np, CheckSolution sol, CheckOutputs out) {
  extern __shared__ double lds[];
  const int b = blockIdx.x;
  const int C = 2 * D;
  const int Pb = np ? np[b] : P;
  const int n = (Pb >= 3 && Pb <= P) ? check_count(sol, ns, b, N) : 0;
  if (n == 0) {
    check_store_skipped(b, out);
    return;
  }
  const CheckAcc acc = check_joint_path(lds, n, D, Pb, P, safety, knots_g + (size_t)b * (P + 3), cps_g + (size_t)b * P * D,
                                        vmax + (size_t)b * D, amax + (size_t)b * D, path_start_g[b], delta_g[b], sol,
                                        (size_t)b * N);
  check_store(acc, b, C, out);
}

// The n samples of one Cartesian path against its 2D + 2 rows, by the whole workgroup: its table
// rows start at row table0 of q_g / J_g, the solution's samples at row0.
__device__ __forceinline__ CheckAcc check_cartesian_path(int n, int D, double safety, const double *q_g,
                                                         const double *J_g, size_t table0, const double *vmax_b,
                                                         const double *amax_b, double vt, double vr, double delta,
                                                         const CheckSolution &sol, size_t row0) {
  const int C = 2 * D + 2;
  const double inv = 1.0 / delta;
  CheckAcc acc;
  for (int i = threadIdx.x; i < n; i += kCheckThreads) {
    double rec[32], ra[34], rb[34], rlo[34], rhi[34];
    const size_t row = table0 + (size_t)i;
    cw_rows_at(i, n, D, inv, q_g + row * D, J_g + row * 6 * D, vmax_b, amax_b, safety, vt, vr, rec, ra, rb, rlo, rhi);
    const double sdd = sol.sdd[row0 + i], sd2 = check_sd2(sol, row0 + i);
    for (int c = 0; c < C; c++) check_row(acc, ra[c], rb[c], rlo[c], rhi[c], sdd, sd2, i, i * C + c);
  }
  return acc;
}

// ------------------------------------------------------------- Cartesian form
// grid = B, block = kCheckThreads. q_g / J_g: [B][N] rows, or row tables read from first_row[b] on.
static __global__ void __launch_bounds__(kCheckThreads)
k_check_cartesian(int N, int D, double safety, const double *q_g, const double *J_g, const double *vmax,
                  const double *amax, const double *vtrans, const double *vrot, const double *delta_g,
                  const int32_t *ns, const int32_t *first_row, CheckSolution sol, CheckOutputs out) {
  const int b = blockIdx.x;
  const int C = 2 * D + 2;
  const int n = check_count(sol, ns, b, N);
  if (n == 0) {
    check_store_skipped(b, out);
    return;
  }
  const CheckAcc acc =
      check_cartesian_path(n, D, safety, q_g, J_g, cw_ragged_first_row(first_row, b, N), vmax + (size_t)b * D,
                           amax + (size_t)b * D, vtrans[b], vrot[b], delta_g[b], sol, (size_t)b * N);
  check_store(acc, b, C, out);
}

inline size_t check_joint_lds(int P, int D) { return ((size_t)(P + 3) + (size_t)P * D + 4 * (size_t)D) * 8; }

// ---------------------------------------------------------------- planner sets
// tpamd_planner_set_set_checking (include/tpamd.h): every window a set's Plan call solves is checked
// in the window loop, directly behind the sweep and in front of k_plan_end / k_plan_append (or
// k_plan_append_early and the step kernel), while the window's arrays, its path_start and the
// loop state are those of the solve. One workgroup per planner as above; a planner that solved no
// window in this iteration (not active: idle, failed, suspended for IK rows, or skipped by the
// start-velocity projection) or whose window is not TPAMD_PATH_OK leaves at once, uncounted.
// Thread 0 merges the window's record into the planner's (planner_check_merge): nothing else
// writes that record during a Plan call, so no atomics.
struct PlannerCheckDev {                 // tpamd_planner_check
  int32_t windows, violations, last_window_violations;
  int32_t worst_window, worst_sample, worst_row, first_window, first_sample;
  double worst_excess, worst_parameter;
};
static_assert(sizeof(PlannerCheckDev) == 48, "tpamd_planner_check is 48 bytes");

__device__ __forceinline__ PlannerCheckDev planner_check_none() {
  PlannerCheckDev r;
  r.windows = 0;
  r.violations = r.last_window_violations = -1;
  r.worst_window = r.worst_sample = r.worst_row = r.first_window = r.first_sample = -1;
  r.worst_excess = r.worst_parameter = qnan();
  return r;
}

// Window `window`'s record (a reduced CheckAcc of C rows per sample) into the planner's. Windows
// arrive in solve order, so an equal excess keeps the earlier window and the first violated
// (window, sample) is set once. w_s: the window's path parameters.
__device__ __forceinline__ void planner_check_merge(PlannerCheckDev &r, const CheckAcc &acc, int C, int window,
                                                    const double *w_s) {
  r.windows += 1;
  r.violations = (r.violations < 0 ? 0 : r.violations) + acc.count;
  r.last_window_violations = acc.count;
  if (acc.flat >= 0 && (r.worst_window < 0 || acc.worst > r.worst_excess)) {
    r.worst_excess = acc.worst;
    r.worst_window = window;
    r.worst_sample = acc.flat / C;
    r.worst_row = acc.flat % C;
    r.worst_parameter = w_s[r.worst_sample];
  }
  if (r.first_window < 0 && acc.first != INT_MAX) {
    r.first_window = window;
    r.first_sample = acc.first;
  }
}

// whether planner b's window of this iteration is checked (block-uniform)
__device__ __forceinline__ bool planner_check_takes_part(const PlanParams &p, int b) {
  return p.active[b] && p.w_status[b] == 0;
}

static __global__ void k_pset_check_clear(int B, PlannerCheckDev *rec) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b < B) rec[b] = planner_check_none();
}

// grid = B, block = kCheckThreads. Dynamic LDS: check_joint_lds(P_lds, D), P_lds the largest path
// of the set. cps [B][pcap][D]; knots p.knots [B][p.K]; sd2 [B][N] is the solver's.
static __global__ void __launch_bounds__(kCheckThreads)
k_pset_check_joint(PlanParams p, int P_lds, int pcap, double safety, const double *cps, const double *vmax,
                   const double *amax, const double *sd2, PlannerCheckDev *rec) {
  extern __shared__ double lds[];
  const int b = blockIdx.x;
  if (!planner_check_takes_part(p, b)) return;
  const int Pb = p.np[b];
  if (Pb < 3 || Pb > P_lds) return;
  const int N = p.N, D = p.D;
  const CheckSolution sol{sd2, nullptr, p.w_sdd, nullptr};
  CheckAcc acc = check_joint_path(lds, N, D, Pb, P_lds, safety, p.knots + (size_t)b * p.K, cps + (size_t)b * pcap * D,
                                  vmax + (size_t)b * D, amax + (size_t)b * D, p.path_start[b], p.delta[b], sol,
                                  (size_t)b * N);
  if (!check_reduce(acc)) return;
  PlannerCheckDev r = rec[b];
  planner_check_merge(r, acc, 2 * D, p.windows[b], p.w_s + (size_t)b * N);
  rec[b] = r;
}

// grid = B, block = kCheckThreads. The window's rows are slots p.first[b] .. + N - 1 of planner b's
// resident table ([B][table_stride] rows), as k_cartesian_lp reads them.
static __global__ void __launch_bounds__(kCheckThreads)
k_pset_check_cartesian(PlanParams p, double safety, const double *q_g, const double *J_g, int table_stride,
                       const double *vmax, const double *amax, const double *vtrans, const double *vrot,
                       const double *sd2, PlannerCheckDev *rec) {
  const int b = blockIdx.x;
  if (!planner_check_takes_part(p, b)) return;
  const int N = p.N, D = p.D;
  const CheckSolution sol{sd2, nullptr, p.w_sdd, nullptr};
  CheckAcc acc = check_cartesian_path(N, D, safety, q_g, J_g, (size_t)b * table_stride + p.first[b], vmax + (size_t)b * D,
                                      amax + (size_t)b * D, vtrans[b], vrot[b], p.delta[b], sol, (size_t)b * N);
  if (!check_reduce(acc)) return;
  PlannerCheckDev r = rec[b];
  planner_check_merge(r, acc, 2 * D + 2, p.windows[b], p.w_s + (size_t)b * N);
  rec[b] = r;
}

// out[k] = the record of planner ids[k] (k, without ids); without `rec` (checking is off), or for an
// id outside the set, the record of "nothing checked".
static __global__ void k_pset_check_results(int B, int count, const int32_t *ids, const PlannerCheckDev *rec,
                                            PlannerCheckDev *out) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= count) return;
  const int b = ids ? ids[k] : k;
  out[k] = (rec && b >= 0 && b < B) ? rec[b] : planner_check_none();
}

}  // namespace tpamd

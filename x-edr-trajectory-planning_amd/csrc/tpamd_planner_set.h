// tpamd_planner_set.h -- B receding-horizon planners whose whole state lives on the device
// (include/tpamd.h tpamd_planner_set_*): the path (spline, limits), the window history
// (*_at_path_samples_), the planner scalars and the resampled trajectory of every
// PathTimingTrajectory stay in HBM between Plan calls; a Plan call moves the two time arguments up
// and one status + summary record per planner down.
//
// PathTimingTrajectory::Plan (path_timing_trajectory.cc:579-684) per planner, one thread each
// where it is control flow:
//   k_pset_prologue  HandleTimeArguments :502-538, UpdatePathTrackingStatus :477-500, the
//                    "already planned enough" branch with EraseTrajectoryBefore :540-577, and the
//                    truncation at GetTimeOffsetAfter :289-305 / :604-621
//   k_pset_resume    in place of the prologue when a streaming Plan of a Cartesian set is resumed
//                    (tpamd_planner_set_plan_resume): the planners that waited for IK rows re-enter
//                    the window loop with the loop state they had
//   window loop      k_plan_begin / set-up / K1 / k_plan_project / sweep / k_plan_end /
//                    k_plan_append (tpamd_kernels.h), as in tpamd_plan_joint_windows_host; with
//                    tpamd_planner_set_set_checking on, k_pset_check_joint / k_pset_check_cartesian
//                    (tpamd_check.h) behind the sweep: the window against its constraint rows
//   resample         k_resample / k_resample_skip over the histories (:755-836)
//   k_pset_epilogue  :662-684: end_time_, final_decel_start_ clamped to time-step multiples,
//                    target_reached_
// tpamd_planner_set_plan_device runs the same bodies with the host out of the loop (a bounded number
// of window iterations, a per-planner capacity gate, fused bookkeeping kernels): see below,
// k_pset_prologue_step .. k_pset_finish_device.
// Times are int64 nanoseconds; TimeFromSec truncates seconds * 1e9, TimeToSec divides by 1e9
// (trajectory_planning/time.h:22-29).
#pragma once

#include "tpamd_kernels.h"

namespace tpamd {

enum { kPsetIdle = 0, kPsetEraseOnly = 1, kPsetWindows = 2 };

struct PlannerSetState {
  int B, N, D, K, cap, tcap, method, max_iterations;
  double time_step_sec;
  long long time_step_duration_ns;      // absl::Seconds(time_step_sec_): llround(s * 1e9)
  // path
  const double *knots;                  // [B][K]: K = P_cap + 3, the stride
  int *np;                              // [B] control points of each planner's path (<= P_cap)
  const double *path_end;               // Cartesian sets: [B] knots.back() of each path; joint sets: null
  const double *amax;                   // [B][D]
  int *path_state;                      // [B]
  int *has_path;                        // [B]
  // history (*_at_path_samples_)
  int *count;
  double *h_time, *h_s, *h_sd, *h_sdd, *h_q, *h_qd, *h_qdd;
  // planner scalars
  int *initial_plan, *planned_to_end, *target_reached;
  double *path_horizon, *path_start, *path_start_velocity, *path_time_start;
  long long *start_time_ns, *end_time_ns, *final_decel_start_ns;
  // profile_ of the last window each planner solved
  const double *w_time;                 // [B][N]
  const int *w_lei;                     // [B]
  // resampled trajectory (time_, positions_, ...): samples t_first .. t_first + t_count - 1
  int *t_first, *t_count;
  double *t_time, *t_s, *t_sd, *t_sdd, *t_q, *t_qd, *t_qdd;
  // this call
  const long long *start_ns, *horizon_ns;
  int *mode, *status, *active, *finish;
  int *num_active;                      // [2]: planners that loop; "a history is full" flag
  int *resample_skip;                   // [B] != 0: no resample for this planner
  double *start_sec;                    // [B]
  int *resample_count;                  // [B]
};

__device__ __forceinline__ long long pset_time_from_sec(double s) { return (long long)(s * 1e9); }
__device__ __forceinline__ double pset_time_to_sec(long long t) { return (double)t / 1e9; }

// path_timing_trajectory.cc:686-695 on a planner's history
__device__ __forceinline__ int pset_lower_index(const double *ht, int n, int starting_index, double time) {
  for (int index = starting_index; index < n - 1; ++index)
    if (ht[index + 1] > time) return index;
  return n - 1;
}

// Everything of Plan() before the window loop. One thread per planner.
__device__ __forceinline__ void pset_prologue_planner(const PlannerSetState &S, int b) {
  const int D = S.D;
  S.mode[b] = kPsetIdle;
  S.active[b] = 0;
  S.finish[b] = 0;
  S.status[b] = kPlanOk;
  S.resample_skip[b] = 1;
  const long long start = S.start_ns[b], horizon = S.horizon_ns[b];
  const double start_sec = pset_time_to_sec(start);
  S.start_sec[b] = start_sec;
  if (!S.has_path[b]) { S.status[b] = kPlanFailedPrecondition; return; }     // :582-584
  // HandleTimeArguments :502-538
  if (S.initial_plan[b] && start > S.end_time_ns[b] + S.time_step_duration_ns) { S.status[b] = kPlanOutOfRange; return; }
  if (!S.initial_plan[b]) {
    S.start_time_ns[b] = start;
    S.end_time_ns[b] = start;
    S.path_start[b] = 0.0;
  } else {
    if (start > S.end_time_ns[b] || start < S.start_time_ns[b]) { S.status[b] = kPlanInvalidArgument; return; }
    S.start_time_ns[b] = start;
  }
  // UpdatePathTrackingStatus :477-500
  const int state = S.path_state[b];
  const bool fresh = (state == 1) || (state == 2);      // kNewPath / kModifiedPath
  int target_reached = 0, planned_to_end = 0;
  if (!S.initial_plan[b]) {
    S.path_horizon[b] = 0.0;
    S.path_start[b] = 0.0;
  } else {
    const double kend = S.path_end ? S.path_end[b] : S.knots[(size_t)b * S.K + S.np[b] + 2];
    planned_to_end = S.path_horizon[b] >= kend - 1e-4;    // CloseToEnd
    if (planned_to_end) {
      if (!fresh) {
        target_reached = 1;
      } else {
        S.path_horizon[b] = 0.0; S.path_time_start[b] = 0.0; S.path_start[b] = 0.0;
        S.path_start_velocity[b] = 0.0;
        planned_to_end = 0;
      }
    }
  }
  S.target_reached[b] = target_reached;
  S.planned_to_end[b] = planned_to_end;
  double *tt = S.t_time + (size_t)b * S.tcap;
  const int first = S.t_first[b], tn = S.t_count[b];
  const bool planned_enough = !fresh && (S.final_decel_start_ns[b] >= start + horizon);
  if (tn > 0 && planned_enough) {
    // EraseTrajectoryBefore(start) :540-577, then done
    S.mode[b] = kPsetEraseOnly;
    const double *tm = tt + first;
    if (start_sec < tm[0]) return;
    int offset;
    if (S.method == 1) {       // kSkipSamplesCloserThanTimeStep
      int lo = 0, hi = tn;     // samples with a time stamp < start_sec (lower_bound)
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (tm[mid] < start_sec) lo = mid + 1; else hi = mid;
      }
      int smaller = min(lo, tn - 1);
      // InterpolateAtTime(start_sec, smaller) over the history (:709-753)
      const int hn = S.count[b];
      const double *ht = S.h_time + (size_t)b * S.cap;
      const int lower = pset_lower_index(ht, hn, max(smaller, 0), start_sec);
      const int upper = min(hn - 1, lower + 1);
      const double at = (fabs(ht[upper] - ht[lower]) < DBL_EPSILON) ? 0.5 : (start_sec - ht[lower]) / (ht[upper] - ht[lower]);
      offset = (tm[smaller] < start_sec + 0.95 * S.time_step_sec) ? smaller : smaller - 1;
      const int nf = first + max(min(offset, tn), 0);        // EraseSamplesUntil(offset) :868-880
      const size_t hl = (size_t)b * S.cap + lower, hu = (size_t)b * S.cap + upper, o = (size_t)b * S.tcap + nf;
      S.t_time[o] = start_sec;
      S.t_s[o] = lerp_ref(at, S.h_s[hl], S.h_s[hu]);
      S.t_sd[o] = lerp_ref(at, S.h_sd[hl], S.h_sd[hu]);
      S.t_sdd[o] = lerp_ref(at, S.h_sdd[hl], S.h_sdd[hu]);
      for (int d = 0; d < D; d++) {
        const double am = S.amax[(size_t)b * D + d];
        S.t_q[o * D + d] = lerp_ref(at, S.h_q[hl * D + d], S.h_q[hu * D + d]);
        S.t_qd[o * D + d] = lerp_ref(at, S.h_qd[hl * D + d], S.h_qd[hu * D + d]);
        const double a = lerp_ref(at, S.h_qdd[hl * D + d], S.h_qdd[hu * D + d]);
        S.t_qdd[o * D + d] = fmin(fmax(a, -am), am);
      }
    } else {
      offset = min((int)round((start_sec - tm[0]) / S.time_step_sec), tn - 1);
    }
    if (offset > 0) {
      const int drop = min(offset, tn);
      S.t_first[b] = first + drop;
      S.t_count[b] = tn - drop;
    }
    return;
  }
  if (S.initial_plan[b]) {
    // GetTimeOffsetAfter(start) :289-305, then everything from there on is dropped (:604-621)
    if (tn == 0) { S.status[b] = kPlanFailedPrecondition; return; }
    const double *tm = tt + first;
    if (start_sec < tm[0]) { S.status[b] = kPlanOutOfRange; return; }
    int lo = 0, hi = tn;       // upper_bound
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (tm[mid] <= start_sec) lo = mid + 1; else hi = mid;
    }
    if (lo == tn) { S.status[b] = kPlanInternal; return; }
    S.t_count[b] = lo;
  }
  S.mode[b] = kPsetWindows;
  S.finish[b] = 1;
  S.resample_skip[b] = 0;
  if (!planned_to_end) {           // the loop condition of :632 before the first window
    S.active[b] = 1;
    atomicAdd(S.num_active, 1);
  }
}
static __global__ void k_pset_prologue(PlannerSetState S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  pset_prologue_planner(S, b);
}

// A resume of a streaming Plan (tpamd_planner_set_plan_resume) runs this in place of the prologue.
// A planner that waited and whose table now holds its window re-enters the window loop: loop,
// windows, loop_start_ns, start_sec and the start_ns / horizon_ns of the suspending call are kept,
// so k_plan_begin recomputes the same window from the unchanged history and the
// max_planning_iterations deadline counts across suspensions. A planner still short of rows keeps
// waiting with a fresh need. Every other planner takes no part: neither the resample nor the
// epilogue touches its trajectory again.
static __global__ void k_pset_resume(PlannerSetState S, PlanParams p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  S.active[b] = 0;
  S.finish[b] = 0;
  S.resample_skip[b] = 1;
  p.need_first[b] = 0;
  p.need_count[b] = 0;
  if (!p.suspended[b]) return;
  int first, last, need_first, need_count;
  if (cw_window_need_from(p.path_start[b], p.path_horizon[b], p.delta[b], p.N, p.rows[b], p.first_row[b], &first, &last,
                          &need_first, &need_count) == kCwNeedsRows) {
    p.need_first[b] = need_first;
    p.need_count[b] = need_count;
    return;
  }
  p.suspended[b] = 0;
  S.status[b] = kPlanOk;
  S.active[b] = 1;
  S.finish[b] = 1;
  S.resample_skip[b] = 0;
  atomicAdd(S.num_active, 1);
}

// "does every looping planner's history have room for one more window?" (count + N <= cap)
static __global__ void k_pset_check_capacity(PlannerSetState S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  if (S.active[b] && S.count[b] + S.N > S.cap) S.num_active[1] = 1;
}

// planners whose window loop ended in an error do not resample (Plan returned before :660)
__device__ __forceinline__ void pset_before_resample_planner(const PlannerSetState &S, int b) {
  if (S.finish[b] && S.status[b] != kPlanOk) { S.finish[b] = 0; S.resample_skip[b] = 1; }
  if (S.finish[b] && S.count[b] < 2) {
    S.resample_skip[b] = 1;
    if (S.method == 0) { S.status[b] = kPlanInternal; S.finish[b] = 0; }   // "nothing to resample"
    else { S.t_first[b] = 0; S.t_count[b] = 0; S.resample_count[b] = 0; }   // kSkip: cleared, no error
  }
}
static __global__ void k_pset_before_resample(PlannerSetState S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  pset_before_resample_planner(S, b);
}

// :662-684 after the resample. resample_count[b] = samples the resample produced. It may exceed
// tcap. The synchronous Plan (need_trajectory null) then reports the count to the host, which
// grows the trajectory arrays and repeats the resample and this kernel.
// tpamd_planner_set_plan_device cannot grow anything: the planner gets kPlanResourceExhausted and
// an empty trajectory (the resample filled tcap slots of a trajectory that does not end at rest,
// which nothing may read out), need_trajectory[b] receives the count, and the scalars are those of
// a plan without samples -- the next Plan of this planner fails its precondition until it is reset.
__device__ __forceinline__ void pset_epilogue_planner(const PlannerSetState &S, int b, int *need_trajectory) {
  if (!S.finish[b]) return;
  if (!S.resample_skip[b]) {
    const int M = S.resample_count[b];
    if (S.method == 0 && M < 1) { S.status[b] = kPlanInternal; return; }   // negative trajectory duration
    S.t_first[b] = 0;
    if (need_trajectory) {
      if (M > S.tcap) { S.status[b] = kPlanResourceExhausted; need_trajectory[b] = M; }
      S.t_count[b] = M > S.tcap ? 0 : M;
    } else {
      if (M > S.tcap) atomicMax(&S.num_active[1], M);      // does not fit: the host grows the buffers and repeats
      S.t_count[b] = min(M, S.tcap);
    }
  }
  S.initial_plan[b] = 1;
  const int tn = S.t_count[b];
  if (tn > 0) {
    const double step = S.time_step_sec;
    long long end = pset_time_from_sec(S.t_time[(size_t)b * S.tcap + S.t_first[b] + tn - 1]);
    end = pset_time_from_sec((double)(long long)round(pset_time_to_sec(end) / step) * step);
    S.end_time_ns[b] = end;
    long long fd = pset_time_from_sec(S.w_time[(size_t)b * S.N + S.w_lei[b]]);
    fd = pset_time_from_sec((double)(long long)round(pset_time_to_sec(fd) / step) * step);
    S.final_decel_start_ns[b] = fd;
  } else {
    S.end_time_ns[b] = S.start_time_ns[b];
    S.final_decel_start_ns[b] = S.end_time_ns[b];
  }
  S.target_reached[b] = S.planned_to_end[b];
}
static __global__ void k_pset_epilogue(PlannerSetState S) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  pset_epilogue_planner(S, b, nullptr);
}

// rows of `count[b]` valid entries (x width doubles) from a buffer of stride old_cap to one of
// stride new_cap (history / trajectory growth)
static __global__ void k_pset_regrow(int B, int old_cap, int new_cap, int width, const int *first, const int *count,
                                     const double *src, double *dst) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int f = first ? first[b] : 0;
  const int n = (f + count[b]) * width;
  if (i >= n) return;
  dst[(size_t)b * new_cap * width + i] = src[(size_t)b * old_cap * width + i];
}

// ---- Cartesian sets: IK tables of the listed planners into the resident arrays
// (tpamd_planner_set_upload_ik_tables*). Planner ids[k]'s table is rows offsets[k] .. offsets[k+1])
// of the packed inputs; it goes to rows 0.. of the planner's [table_stride] rows.
struct IkUploadParams {
  int count, D, table_stride;
  const int *ids, *offsets;             // [count], [count + 1]
  // packed inputs (device)
  const double *q, *J;                  // [rows][D], [rows][6][D]
  const double *path_end, *vmax, *amax, *vtrans, *vrot, *delta, *iv;   // iv may be null (zero)
  const int *state;
  // the set's arrays
  double *t_q, *t_J;
  double *s_path_end, *s_vmax, *s_amax, *s_vtrans, *s_vrot, *s_delta, *s_iv;
  int *s_rows, *s_state, *s_has;
  int *s_first_row;                     // [B] path row in slot 0 of each table (0 after an upload)
  // append (tpamd_planner_set_append_ik_rows*): not null, and the planner's rows go behind its last
  // resident row as the DEVICE counts it (path row s_rows, slot s_rows - s_first_row); dst_first[k] is
  // the host's count, the same number for every planner the kernels accept. null: an upload, rows 0..
  const int *dst_first;                 // [count]
};

// rows of `width` doubles; grid = (ceil(longest table * width / 256), count). An append leaves a
// planner without a path (its table was rejected at the upload) untouched. A destination row offset
// moves a planner's run of Jacobians by a multiple of a row, 48 D bytes: for D = 6 that is 288
// bytes, so the runs k_cartesian_lp<1, 6> reads as double2 stay 16-byte aligned. A discard
// (k_pset_ik_compact) moves the rows down by whole rows as well, so every slot offset stays a
// multiple of a row and this holds after any sequence of discards and appends.
static __global__ void k_pset_ik_rows(IkUploadParams p, int width, const double *src, double *dst) {
  const int k = blockIdx.y;
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)(p.offsets[k + 1] - p.offsets[k]) * width;
  if (e >= n) return;
  size_t row0 = (size_t)p.ids[k] * p.table_stride;
  if (p.dst_first) {
    // the device's own row count is the destination; a planner whose count the host sees differently
    // (its table was rejected at a _device upload) has no path and is skipped, and nothing is ever
    // written past the planner's rows
    const int b = p.ids[k], have = p.s_rows[b], live = have - p.s_first_row[b];
    if (!p.s_has[b] || have != p.dst_first[k] || live < 0 || live + (p.offsets[k + 1] - p.offsets[k]) > p.table_stride)
      return;
    row0 += (size_t)live;
  }
  dst[row0 * width + e] = src[(size_t)p.offsets[k] * width + e];
}

// an append's row counts; one thread per listed planner. A planner without a table is skipped.
static __global__ void k_pset_ik_append_scalars(IkUploadParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = p.ids[k];
  const int live = p.s_rows[b] - p.s_first_row[b];
  if (!p.s_has[b] || p.s_rows[b] != p.dst_first[k] || live < 0 || live + (p.offsets[k + 1] - p.offsets[k]) > p.table_stride)
    return;
  p.s_rows[b] += p.offsets[k + 1] - p.offsets[k];
}

// limits, delta, initial velocity, state and row count; one thread per listed planner. The _device
// entry cannot check delta and the state on the host: a planner whose delta is not > 0 or whose
// state is not 1 / 2 is left without a path (Plan: failed precondition).
static __global__ void k_pset_ik_scalars(IkUploadParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = p.ids[k], D = p.D;
  p.s_first_row[b] = 0;
  if (!(p.delta[k] > 0.0) || (p.state[k] != 1 && p.state[k] != 2)) {
    p.s_rows[b] = 0;
    p.s_state[b] = 0;
    p.s_has[b] = 0;
    return;
  }
  for (int d = 0; d < D; d++) {
    p.s_vmax[(size_t)b * D + d] = p.vmax[(size_t)k * D + d];
    p.s_amax[(size_t)b * D + d] = p.amax[(size_t)k * D + d];
    p.s_iv[(size_t)b * D + d] = p.iv ? p.iv[(size_t)k * D + d] : 0.0;
  }
  p.s_path_end[b] = p.path_end[k];
  p.s_vtrans[b] = p.vtrans[k];
  p.s_vrot[b] = p.vrot[k];
  p.s_delta[b] = p.delta[k];
  p.s_rows[b] = p.offsets[k + 1] - p.offsets[k];
  p.s_state[b] = p.state[k];
  p.s_has[b] = 1;
}

// ---- Cartesian sets: discarding the consumed rows at the front of the listed planners' tables
// (tpamd_planner_set_discard_ik_rows). k_pset_discard_begin picks each planner's new first resident
// row, k_pset_ik_compact moves the live rows down to slot 0.
struct IkDiscardParams {
  int count, D, table_stride, cap;
  const int *ids;                       // [count]
  const int *keep_from;                 // [count] path rows; null: cw_discard_floor of each planner
  int *shift;                           // [count] out: rows each table moves down by (0: nothing to do)
  int *first_out;                       // [count] out: the new first resident row
  double *t_q, *t_J;
  const int *s_rows, *s_has, *s_state, *s_count;
  int *s_first_row;
  const double *h_time, *h_s, *delta;   // the window histories [B][cap], delta [B]
  const long long *start_time_ns;       // [B] start_time_
};

// One thread per listed planner. The new first row is keep_from (or the floor) clamped to
// [first_row, rows - 1]: the last resident row always stays, the streaming chain seeds the IK with
// it. A planner without a path on the device (its table was rejected at a _device upload) is left
// as it is.
static __global__ void k_pset_discard_begin(IkDiscardParams p) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= p.count) return;
  const int b = p.ids[k];
  const int old_first = p.s_first_row[b], rows = p.s_rows[b];
  int keep = old_first;
  if (p.s_has[b] && rows - old_first >= 1) {
    keep = p.keep_from ? p.keep_from[k]
                       : cw_discard_floor(p.h_time + (size_t)b * p.cap, p.h_s + (size_t)b * p.cap, p.s_count[b],
                                          (double)p.start_time_ns[b] / 1e9, p.s_state[b], p.delta[b]);
    keep = min(max(keep, old_first), rows - 1);
  }
  p.shift[k] = keep - old_first;
  p.first_out[k] = keep;
  p.s_first_row[b] = keep;
}

// The move: rows (new) first_row .. rows - 1 of planner ids[k] from slot `shift` on to slot 0 on, in
// place; blockIdx.z picks the array (0: q, width D; 1: J, width 6 D). Source and destination
// overlap whenever shift < live rows, the normal case (a replan consumes a fraction of a window),
// so the elements are visited in the order of cw_compact_chunks / cw_compact_index
// (tpamd_cartesian_window.h, with the argument why one barrier per chunk is enough): one workgroup
// (blockIdx.x == 0) walks the chunks in ascending order, kCompactUnroll loads in flight per thread,
// all of them complete (vmcnt(0)) before the barrier, stores after it. Where they do not overlap
// (shift >= live) the chunks are independent and the gridDim.x workgroups share them.
// V is double2 where the planner's base, the shift and the length keep 16-byte alignment (J rows
// are 48 D bytes: always; q rows at odd D only for even shifts and lengths), else double.
constexpr int kCompactThreads = 256, kCompactUnroll = 4, kCompactSplit = 8;
template <typename V>
__device__ __forceinline__ void pset_compact_run(V *base, long long n, long long shift, bool overlap) {
  const long long chunks = cw_compact_chunks(n, kCompactThreads, kCompactUnroll);
  const long long c0 = overlap ? 0 : blockIdx.x, step = overlap ? 1 : gridDim.x;
  const int tid = threadIdx.x;
  static_assert(kCompactUnroll == 4, "the four loads below are written out");
  for (long long c = c0; c < chunks; c += step) {
    // written out rather than kept in an array: an indexed array lands in LDS, not in registers
    const long long e0 = cw_compact_index(c, kCompactThreads, kCompactUnroll, tid, 0);
    const long long e1 = cw_compact_index(c, kCompactThreads, kCompactUnroll, tid, 1);
    const long long e2 = cw_compact_index(c, kCompactThreads, kCompactUnroll, tid, 2);
    const long long e3 = cw_compact_index(c, kCompactThreads, kCompactUnroll, tid, 3);
    // clamped, not branched: the loads stay in flight together
    const V v0 = base[(e0 < n ? e0 : n - 1) + shift];
    const V v1 = base[(e1 < n ? e1 : n - 1) + shift];
    const V v2 = base[(e2 < n ? e2 : n - 1) + shift];
    const V v3 = base[(e3 < n ? e3 : n - 1) + shift];
    if (overlap) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the loads have landed, not merely been issued
      __syncthreads();
    }
    if (e0 < n) base[e0] = v0;
    if (e1 < n) base[e1] = v1;
    if (e2 < n) base[e2] = v2;
    if (e3 < n) base[e3] = v3;
  }
}
static __global__ __launch_bounds__(kCompactThreads) void k_pset_ik_compact(IkDiscardParams p) {
  const int k = blockIdx.y;
  const int shift = p.shift[k];
  if (shift <= 0) return;
  const int b = p.ids[k];
  const int live = p.s_rows[b] - p.s_first_row[b];       // rows that stay (first_row is the new one)
  if (live <= 0 || shift + live > p.table_stride) return;
  const bool overlap = shift < live;
  if (overlap && blockIdx.x != 0) return;
  const int width = blockIdx.z ? 6 * p.D : p.D;
  double *base = (blockIdx.z ? p.t_J : p.t_q) + (size_t)b * p.table_stride * width;
  const long long n = (long long)live * width, s = (long long)shift * width;
  if ((((size_t)base >> 3) | (size_t)n | (size_t)s) & 1)
    pset_compact_run<double>(base, n, s, overlap);
  else
    pset_compact_run<double2>((double2 *)base, n >> 1, s >> 1, overlap);
}

// ---- tpamd_planner_set_plan_device: Plan with the host out of the loop. The number of window
// iterations is an argument, so nothing has to come down between them; what the synchronous Plan
// settles on the host (is there room for one more window? does the trajectory fit?) is settled
// per planner here, and the one-thread-per-planner kernels that would run back to back are one
// kernel:
//   k_pset_prologue_step  time arguments from the caller's device arrays, loop state cleared,
//                         k_pset_prologue, gate, k_plan_begin of window 0
//   k_pset_step           k_plan_end of window i, gate, k_plan_begin of window i + 1
//   k_pset_last_step      k_plan_end of the last window, k_pset_before_resample
//   k_pset_epilogue_device, k_pset_finish_device
// Each body is the synchronous kernel's (the same __device__ function), so a planner ends in the
// same state bit for bit. k_plan_append_early (tpamd_kernels.h) runs in front of the step kernels.
//
// The gate, in place of the call-wide flag of k_pset_check_capacity: a looping planner whose
// history has no room for one more window wherever it connects (count + N > cap) stops looping
// with kPlanResourceExhausted; k_pset_before_resample then takes it out of the resample and the
// epilogue like any planner whose loop ended in an error. need_history[b] = count + N.
__device__ __forceinline__ void pset_gate_planner(const PlannerSetState &S, int b, int *need_history) {
  if (!S.active[b]) return;
  const int want = S.count[b] + S.N;
  if (want <= S.cap) return;
  S.status[b] = kPlanResourceExhausted;
  S.active[b] = 0;
  need_history[b] = want;
}

// need [2][B]: history samples / trajectory samples a planner lacked in this call (0: none)
static __global__ void k_pset_prologue_step(PlannerSetState S, PlanParams p, const long long *start_ns,
                                            const long long *horizon_ns, long long *d_start, long long *d_horizon,
                                            int *need) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  const long long start = start_ns[b];
  d_start[b] = start;
  d_horizon[b] = horizon_ns[b];
  p.loop_start_ns[b] = start;                 // :630
  p.old_state[b] = 0; p.offset[b] = 0; p.loop[b] = 0; p.append[b] = 0; p.windows[b] = 0;
  need[b] = 0;
  need[S.B + b] = 0;
  pset_prologue_planner(S, b);
  pset_gate_planner(S, b, need);
  plan_begin_planner(p, b);
}

static __global__ void k_pset_step(PlannerSetState S, PlanParams p, int *need) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  plan_end_planner(p, b);
  pset_gate_planner(S, b, need);
  plan_begin_planner(p, b);
}

static __global__ void k_pset_last_step(PlannerSetState S, PlanParams p) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  plan_end_planner(p, b);
  pset_before_resample_planner(S, b);
}

static __global__ void k_pset_epilogue_device(PlannerSetState S, int *need) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  pset_epilogue_planner(S, b, need + S.B);
}

// summary record per planner (what the mirror's getters need without a trajectory download)
struct PlannerSummaryDev {
  long long end_time_ns, final_decel_start_ns, start_time_ns;
  int num_samples, target_reached, planned_to_end, windows, path_state, history_count, status, pad;
};
static __global__ void k_pset_summary(PlannerSetState S, const int *windows, PlannerSummaryDev *out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= S.B) return;
  PlannerSummaryDev r;
  r.end_time_ns = S.end_time_ns[b]; r.final_decel_start_ns = S.final_decel_start_ns[b];
  r.start_time_ns = S.start_time_ns[b];
  r.num_samples = S.t_count[b]; r.target_reached = S.target_reached[b]; r.planned_to_end = S.planned_to_end[b];
  r.windows = windows[b]; r.path_state = S.path_state[b]; r.history_count = S.count[b]; r.status = S.status[b];
  r.pad = 0;
  out[b] = r;
}

// tpamd_plan_device_info (include/tpamd.h)
struct PlanDeviceInfoDev {
  int num_ok, num_failed, num_exhausted, needed_history, needed_trajectory, max_windows_solved, reserved[2];
};
// The summaries (into the set's own array and, if not null, the caller's) and the call's info record:
// one workgroup of kFinishThreads strides over the planners, each wave reduces its lanes' counts
// with shuffles, LDS combines the waves.
constexpr int kFinishThreads = 256;
static __global__ __launch_bounds__(kFinishThreads) void k_pset_finish_device(PlannerSetState S, const int *windows,
                                                                             const int *need, PlannerSummaryDev *own,
                                                                             PlannerSummaryDev *out,
                                                                             PlanDeviceInfoDev *info) {
  int v[6] = {0, 0, 0, 0, 0, 0};     // ok, failed, exhausted (sums); history, trajectory, windows (maxima)
  for (int b = threadIdx.x; b < S.B; b += kFinishThreads) {
    PlannerSummaryDev r;
    r.end_time_ns = S.end_time_ns[b]; r.final_decel_start_ns = S.final_decel_start_ns[b];
    r.start_time_ns = S.start_time_ns[b];
    r.num_samples = S.t_count[b]; r.target_reached = S.target_reached[b]; r.planned_to_end = S.planned_to_end[b];
    r.windows = windows[b]; r.path_state = S.path_state[b]; r.history_count = S.count[b]; r.status = S.status[b];
    r.pad = 0;
    own[b] = r;
    if (out) out[b] = r;
    v[0] += r.status == kPlanOk;
    v[1] += r.status != kPlanOk;
    v[2] += r.status == kPlanResourceExhausted;
    v[3] = max(v[3], need[b]);
    v[4] = max(v[4], need[S.B + b]);
    v[5] = max(v[5], r.windows);
  }
  if (!info) return;
  __shared__ int part[kFinishThreads / 64][6];
#pragma unroll
  for (int k = 0; k < 6; k++) {
    int x = v[k];
    for (int off = 32; off > 0; off >>= 1) {
      const int y = __shfl_down(x, off, 64);
      x = k < 3 ? x + y : max(x, y);
    }
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6][k] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int t[6];
    for (int k = 0; k < 6; k++) {
      t[k] = part[0][k];
      for (int w = 1; w < kFinishThreads / 64; w++) t[k] = k < 3 ? t[k] + part[w][k] : max(t[k], part[w][k]);
    }
    PlanDeviceInfoDev r;
    r.num_ok = t[0]; r.num_failed = t[1]; r.num_exhausted = t[2];
    r.needed_history = t[3]; r.needed_trajectory = t[4]; r.max_windows_solved = t[5];
    r.reserved[0] = r.reserved[1] = 0;
    *info = r;
  }
}

}  // namespace tpamd

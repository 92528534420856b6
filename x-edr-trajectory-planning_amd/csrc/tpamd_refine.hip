// tpamd_refine.hip -- the three kernels of tpamd_refine.h in a translation unit of their own, so
// that every other kernel keeps its code.
#include <hip/hip_runtime.h>

#include "tpamd_refine.h"

namespace tpamd {

constexpr int kSelectThreads = 256;                // one chunk of paths
constexpr int kSelectWaves = kSelectThreads / 64;
constexpr int kStepThreads = 256;

// One workgroup walks the paths in chunks of kSelectThreads. In a chunk, thread t has path
// base + t: the wave's ballot of "is a candidate" and the count of set bits below the lane give the
// path's rank inside its wave in path order, the waves' totals cross through LDS, and `running`
// (the same in every thread) carries the rank across chunks.
static __global__ void __launch_bounds__(kSelectThreads) k_refine_select(RefineSelectParams p) {
  __shared__ int s_total[2][kSelectWaves];         // double-buffered: one barrier per chunk
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  int buf = 0;
  for (int base = 0; base < p.B; base += kSelectThreads, buf ^= 1) {
    const int b = base + tid;
    int cand = kRefineNothing, n = 0;
    if (b < p.B) {
      n = p.ns ? p.ns[b] : p.N;
      cand = refine_candidate(p.violations[b], p.worst_excess[b], p.tolerance, n, p.max_samples);
    }
    const unsigned long long votes = __ballot(cand == 0);
    const int below = __popcll(votes & ((1ull << lane) - 1ull));
    if (lane == 0) s_total[buf][wave] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < kSelectWaves; w++) {
      const int t = s_total[buf][w];
      if (w < wave) before += t;
      total += t;
    }
    if (b < p.B) {
      const int code = refine_slot_code(cand, running + before + below, p.M);
      p.slot[b] = code;
      if (code >= 0) {
        const RefineSlot s = refine_first(n, p.delta[b]);
        p.slot_path[code] = b;
        p.rounds[code] = s.rounds;
        p.num_samples[code] = s.num_samples;
        p.delta_out[code] = s.delta;
        p.next_samples[code] = s.next_samples;
        p.next_delta[code] = s.next_delta;
      }
    }
    running += total;
  }
  const int used = running < p.M ? running : p.M;
  for (int k = used + tid; k < p.M; k += kSelectThreads) {
    const RefineSlot s = refine_unused();
    p.slot_path[k] = -1;
    p.rounds[k] = s.rounds;
    p.num_samples[k] = s.num_samples;
    p.delta_out[k] = s.delta;
    p.next_samples[k] = s.next_samples;
    p.next_delta[k] = s.next_delta;
  }
  // every slot's record starts as "not checked" (tpamd_check.h); k_refine_step replaces a used slot's
  for (int k = tid; k < p.M; k += kSelectThreads) {
    if (p.record.violations) p.record.violations[k] = -1;
    if (p.record.worst_excess) p.record.worst_excess[k] = __builtin_nan("");
    if (p.record.worst_sample) p.record.worst_sample[k] = -1;
    if (p.record.worst_row) p.record.worst_row[k] = -1;
    if (p.record.first_sample) p.record.first_sample[k] = -1;
  }
  if (tid == 0) {
    *p.num_refined = used;
    *p.live = used;
  }
}

// One 64-lane workgroup per slot: the path's spline, limits and start values into the sub-batch.
static __global__ void __launch_bounds__(64) k_refine_gather(RefineGatherParams p) {
  const int k = blockIdx.x, lane = threadIdx.x;
  const int b = p.slot_path[k];
  if (b < 0) {
    if (p.np_out && lane == 0) p.np_out[k] = 0;
    return;
  }
  const int K = p.knots_per_path, PD = p.points_per_path * p.D, D = p.D;
  const double *knots = p.knots + (size_t)b * K, *cps = p.cps + (size_t)b * PD;
  double *knots_out = p.knots_out + (size_t)k * K, *cps_out = p.cps_out + (size_t)k * PD;
  for (int i = lane; i < K; i += 64) knots_out[i] = knots[i];
  for (int i = lane; i < PD; i += 64) cps_out[i] = cps[i];
  for (int i = lane; i < D; i += 64) {
    p.vmax_out[(size_t)k * D + i] = p.vmax[(size_t)b * D + i];
    p.amax_out[(size_t)k * D + i] = p.amax[(size_t)b * D + i];
  }
  if (lane == 0) {
    p.path_start_out[k] = p.path_start ? p.path_start[b] : 0.0;
    p.sd_start_out[k] = p.sd_start ? p.sd_start[b] : 0.0;
    p.sdd_start_out[k] = p.sdd_start ? p.sdd_start[b] : 0.0;
    p.time_start_out[k] = p.time_start ? p.time_start[b] : 0.0;
    if (p.np_out) p.np_out[k] = p.np[b];
  }
}

// One workgroup, one thread per slot and trip: the record of the solve a slot just made goes to the
// caller's arrays, the slot's counters advance, and its next count is decided. The number of slots
// that go on is summed through LDS (no atomics).
static __global__ void __launch_bounds__(kStepThreads) k_refine_step(RefineStepParams p) {
  __shared__ int s_live[kStepThreads / 64];
  const int tid = threadIdx.x;
  int live = 0;
  for (int k = tid; k < p.M; k += kStepThreads) {
    RefineSlot s;
    s.rounds = p.rounds[k];
    s.num_samples = p.num_samples[k];
    s.delta = p.delta_out[k];
    s.next_samples = p.next_samples[k];
    s.next_delta = p.next_delta[k];
    const int violations = p.made.violations[k];
    const double excess = p.made.worst_excess[k];
    if (!refine_step(s, violations, excess, p.tolerance, p.max_rounds, p.max_samples)) continue;
    p.rounds[k] = s.rounds;
    p.num_samples[k] = s.num_samples;
    p.delta_out[k] = s.delta;
    p.next_samples[k] = s.next_samples;
    p.next_delta[k] = s.next_delta;
    if (p.out.violations) p.out.violations[k] = violations;
    if (p.out.worst_excess) p.out.worst_excess[k] = excess;
    if (p.out.worst_sample) p.out.worst_sample[k] = p.made.worst_sample[k];
    if (p.out.worst_row) p.out.worst_row[k] = p.made.worst_row[k];
    if (p.out.first_sample) p.out.first_sample[k] = p.made.first_sample[k];
    if (s.next_samples > 0) live++;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) live += __shfl_xor(live, off, 64);
  if ((tid & 63) == 0) s_live[tid >> 6] = live;
  __syncthreads();
  if (tid == 0) {
    int total = 0;
    for (int w = 0; w < kStepThreads / 64; w++) total += s_live[w];
    *p.live = total;
  }
}

void launch_refine_select(const RefineSelectParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_refine_select, dim3(1), dim3(kSelectThreads), 0, st, p);
}

void launch_refine_gather(const RefineGatherParams &p, hipStream_t st) {
  if (p.M < 1) return;
  hipLaunchKernelGGL(k_refine_gather, dim3((unsigned)p.M), dim3(64), 0, st, p);
}

void launch_refine_step(const RefineStepParams &p, hipStream_t st) {
  hipLaunchKernelGGL(k_refine_step, dim3(1), dim3(kStepThreads), 0, st, p);
}

}  // namespace tpamd

// tpamd_state.hip -- the kernels of tpamd_state.h in a translation unit of their own: planner
// state records written from and read into the resident arrays of a planner set.
#include <hip/hip_runtime.h>

#include "tpamd_state.h"

namespace tpamd {

namespace {

constexpr int kStateCopyThreads = 256;

__device__ __forceinline__ uint64_t st_bits(double x) { return (uint64_t)__double_as_longlong(x); }
__device__ __forceinline__ double st_double(uint64_t x) { return __longlong_as_double((long long)x); }
__device__ __forceinline__ int st_clamp(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Section s of planner b in the set's arrays; tf: the trajectory's first live sample.
__device__ __forceinline__ uint64_t *state_section(const StateSetView &v, int b, int tf, int s) {
  const size_t D = (size_t)v.D, sb = (size_t)b;
  double *p = nullptr;
  switch (s) {
    case kSecKnots: p = v.knots + sb * v.K; break;
    case kSecCp: p = v.cp + sb * v.pcap * D; break;
    case kSecVmax: p = v.vmax + sb * D; break;
    case kSecAmax: p = v.amax + sb * D; break;
    case kSecIv: p = v.iv + sb * D; break;
    case kSecHTime: case kSecHS: case kSecHSd: case kSecHSdd: p = v.h[s - kSecHTime] + sb * v.cap; break;
    case kSecHQ: case kSecHQd: case kSecHQdd: p = v.h[s - kSecHTime] + sb * v.cap * D; break;
    case kSecWTime: p = v.w_time + sb * v.N; break;
    case kSecTTime: case kSecTS: case kSecTSd: case kSecTSdd: p = v.t[s - kSecTTime] + sb * v.tcap + tf; break;
    case kSecTQ: case kSecTQd: case kSecTQdd: p = v.t[s - kSecTTime] + (sb * v.tcap + tf) * D; break;
    case kSecTableQ: p = v.tq + sb * v.table_cap * D; break;
    case kSecTableJ: p = v.tJ + sb * v.table_cap * 6 * D; break;
  }
  return (uint64_t *)p;
}

// The header of planner b as the set holds it. Counts are clamped to the set's capacities, so the
// copy kernel stays inside the arrays whatever the count arrays hold. *tf: t_first.
__device__ __forceinline__ StateRecordHeader state_header_of(const StateSetView &v, int b, int *tf) {
  StateRecordHeader h;
  const bool cart = v.shape.kind == kStateCartesian;
  const bool has = v.has_path[b] != 0;
  h.magic = kStateMagic;
  h.version = kStateVersion;
  h.bytes = 0;
  h.shape = v.shape;
  h.num_points = (!cart && has) ? st_clamp(v.np[b], 0, v.pcap) : 0;
  h.history_count = st_clamp(v.count[b], 0, v.cap);
  const int first = st_clamp(v.t_first[b], 0, v.tcap);
  *tf = first;
  h.trajectory_count = st_clamp(v.t_count[b], 0, v.tcap - first);
  h.first_row = 0;
  h.table_rows = 0;
  if (cart && has) {
    h.first_row = st_clamp(v.first_row[b], 0, kStateMaxSamples);
    const int live = st_clamp(v.rows[b] - h.first_row, 0, v.table_cap);
    h.table_rows = st_clamp(h.first_row + live, 0, kStateMaxSamples);
    if (h.first_row > h.table_rows) h.first_row = h.table_rows;
  }
  h.has_path = has;
  h.path_state = v.path_state[b];
  h.initial_plan = v.initial_plan[b] != 0;
  h.planned_to_end = v.planned_to_end[b] != 0;
  h.target_reached = v.target_reached[b] != 0;
  h.w_lei = h.initial_plan ? st_clamp(v.w_lei[b], 0, v.N - 1) : 0;
  h.reserved = 0;
  h.path_horizon = st_bits(v.path_horizon[b]);
  h.path_start = st_bits(v.path_start[b]);
  h.path_start_velocity = st_bits(v.path_start_velocity[b]);
  h.path_time_start = st_bits(v.path_time_start[b]);
  h.start_time_ns = v.start_time_ns[b];
  h.end_time_ns = v.end_time_ns[b];
  h.final_decel_start_ns = v.final_decel_start_ns[b];
  h.delta = has ? st_bits(v.delta[b]) : 0;
  h.path_end = (cart && has) ? st_bits(v.path_end[b]) : 0;
  h.vtrans = (cart && has) ? st_bits(v.vtrans[b]) : 0;
  h.vrot = (cart && has) ? st_bits(v.vrot[b]) : 0;
  return h;
}

__device__ __forceinline__ StateSummaryDev state_summary_of(const StateRecordHeader &h, int status) {
  StateSummaryDev r;
  r.end_time_ns = h.end_time_ns; r.final_decel_start_ns = h.final_decel_start_ns; r.start_time_ns = h.start_time_ns;
  r.num_samples = h.trajectory_count; r.target_reached = h.target_reached; r.planned_to_end = h.planned_to_end;
  r.windows = 0; r.path_state = h.path_state; r.history_count = h.history_count; r.status = status; r.pad = 0;
  return r;
}

__device__ __forceinline__ void state_item_store(StateItem *dst, int b, int go, int tf, const StateLayout &L) {
  dst->b = b; dst->go = go; dst->t_first = tf; dst->pad = 0;
  uint64_t units = 0;
  for (int s = 0; s < kStateSections; s++) {
    dst->off[s] = L.off[s];
    dst->words[s] = L.words[s];
    dst->ustart[s] = units;
    units += (L.words[s] + 1) >> 1;
  }
  dst->ustart[kStateSections] = units;
  dst->ustart[kStateSections + 1] = 0;
}

// Export, one thread per listed planner: the header into the planner's slot, the sections for the
// copy kernel, the status and (if asked for) the info record. With a slot that is too small only
// the header is written (not even that below 192 bytes).
__global__ void __launch_bounds__(64) k_state_export_layout(StateSetView v, StateCall c) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= c.count) return;
  const int b = c.ids ? c.ids[k] : k;
  StateItem *item = c.items + k;
  item->b = 0; item->go = 0; item->t_first = 0; item->pad = 0;
  StateInfoDev info{};
  int status = kStPlanOk;
  if (b < 0 || b >= v.B) {
    status = kStPlanInvalidArgument;
  } else if (v.suspended && v.suspended[b]) {
    status = kStPlanFailedPrecondition;
  } else {
    int tf = 0;
    StateRecordHeader h = state_header_of(v, b, &tf);
    const StateLayout L = state_record_layout(h);
    h.bytes = L.bytes;
    info.bytes = (long long)L.bytes;
    info.num_points = h.num_points; info.history_count = h.history_count; info.trajectory_count = h.trajectory_count;
    info.table_rows = h.table_rows; info.first_row = h.first_row; info.has_path = h.has_path;
    info.path_state = h.path_state; info.initial_plan = h.initial_plan; info.planned_to_end = h.planned_to_end;
    info.target_reached = h.target_reached; info.trajectory_first = tf;
    if (c.blob) {
      const long long at = c.offsets[k], slot = c.offsets[k + 1] - at;
      if (at < 0 || (at & 15)) {
        status = kStPlanInvalidArgument;
      } else if (slot < (long long)sizeof(StateRecordHeader)) {
        status = kStPlanResourceExhausted;
      } else {
        uint64_t *dst = (uint64_t *)(c.blob + at);
        const uint64_t *src = (const uint64_t *)&h;
        for (int i = 0; i < (int)(sizeof(StateRecordHeader) / 8); i++) dst[i] = src[i];
        if ((long long)L.bytes > slot) status = kStPlanResourceExhausted;
        else state_item_store(item, b, 1, tf, L);
      }
    }
  }
  info.status = status;
  if (c.status) c.status[k] = status;
  if (c.info) c.info[k] = info;
}

// Import, one thread per listed planner: the record is validated before anything is read through
// a size it states, then gated against the set's capacities; a planner that passes gets its
// scalars here and its sections from the copy kernel. A planner that does not pass keeps its state.
__global__ void __launch_bounds__(64) k_state_import_layout(StateSetView v, StateCall c) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= c.count) return;
  const int b = c.ids ? c.ids[k] : k;
  StateItem *item = c.items + k;
  item->b = 0; item->go = 0; item->t_first = 0; item->pad = 0;
  int status = kStPlanOk;
  StateSummaryDev summary{};
  if (b < 0 || b >= v.B) {
    status = kStPlanInvalidArgument;
  } else {
    const bool cart = v.shape.kind == kStateCartesian;
    const long long at = c.offsets[k], len = c.offsets[k + 1] - at;
    const unsigned char *rec = c.blob + at;
    if (at < 0 || (at & 15) || len < 0 || state_record_validate(rec, (size_t)len, v.shape) != kStateOk) {
      status = kStPlanInvalidArgument;
    } else if (v.suspended && v.suspended[b]) {
      status = kStPlanFailedPrecondition;
    } else {
      const StateRecordHeader h = state_record_header(rec);
      if (h.num_points > v.pcap || h.history_count > v.cap || h.trajectory_count > v.tcap ||
          h.table_rows - h.first_row > v.table_cap) {
        status = kStPlanResourceExhausted;
      } else {
        const StateLayout L = state_record_layout(h);
        state_item_store(item, b, 1, 0, L);
        v.has_path[b] = h.has_path;
        v.path_state[b] = h.path_state;
        if (h.num_points) v.np[b] = h.num_points;
        v.count[b] = h.history_count;
        v.initial_plan[b] = h.initial_plan;
        v.planned_to_end[b] = h.planned_to_end;
        v.target_reached[b] = h.target_reached;
        if (h.initial_plan) v.w_lei[b] = h.w_lei;
        v.t_first[b] = 0;
        v.t_count[b] = h.trajectory_count;
        if (v.check) {       // the windows checked in this slot were another planner's: "nothing checked"
          StateCheckDev none;
          none.windows = 0;
          none.violations = none.last_window_violations = -1;
          none.worst_window = none.worst_sample = none.worst_row = none.first_window = none.first_sample = -1;
          none.worst_excess = none.worst_parameter = __longlong_as_double(0x7ff8000000000000LL);
          v.check[b] = none;
        }
        v.path_horizon[b] = st_double(h.path_horizon);
        v.path_start[b] = st_double(h.path_start);
        v.path_start_velocity[b] = st_double(h.path_start_velocity);
        v.path_time_start[b] = st_double(h.path_time_start);
        v.start_time_ns[b] = h.start_time_ns;
        v.end_time_ns[b] = h.end_time_ns;
        v.final_decel_start_ns[b] = h.final_decel_start_ns;
        if (h.has_path) v.delta[b] = st_double(h.delta);
        if (cart) {
          v.rows[b] = h.table_rows;
          v.first_row[b] = h.first_row;
          if (h.has_path) {
            v.path_end[b] = st_double(h.path_end);
            v.vtrans[b] = st_double(h.vtrans);
            v.vrot[b] = st_double(h.vrot);
          }
        }
        summary = state_summary_of(h, status);
      }
    }
    if (status != kStPlanOk) {
      int tf = 0;
      summary = state_summary_of(state_header_of(v, b, &tf), status);
    }
  }
  summary.status = status;
  if (c.status) c.status[k] = status;
  if (c.summary) c.summary[k] = summary;
}

// The sections of every listed planner that passed the layout kernel, between its record and the
// set's arrays. grid = (copy_blocks, count). The record behind its header is one run of 16-byte
// units (StateItem); the workgroups of a planner stride over that run, lane i next to lane i + 1,
// kStateUnroll units per thread in flight: all loads of a trip are issued before its first store,
// so a trip costs one memory round trip whatever sections its units fall into (a loop over the
// sections costs one per section). The record's side of a unit is always one 16-byte access; the
// set's side is one where the section's slot is 16-byte aligned and the unit holds two words, and
// 8-byte accesses otherwise (a row that starts at an odd sample: a trajectory from an odd t_first, a
// slot at an odd stride; a section's last word). An export stores the zero pad word with the last
// word of an odd section, so the record's bytes never depend on what the blob held before.
constexpr int kStateUnroll = 4;
template <bool kImport>
__global__ void __launch_bounds__(kStateCopyThreads) k_state_copy(StateSetView v, StateCall c) {
  const int k = blockIdx.y;
  const StateItem *item = c.items + k;
  if (!item->go) return;
  __shared__ uint64_t s_start[kStateSections + 1], s_words[kStateSections];
  __shared__ uint64_t *s_set[kStateSections];
  if (threadIdx.x < kStateSections) {
    s_start[threadIdx.x] = item->ustart[threadIdx.x];
    s_words[threadIdx.x] = item->words[threadIdx.x];
    s_set[threadIdx.x] = state_section(v, item->b, item->t_first, threadIdx.x);
  }
  if (threadIdx.x == 0) s_start[kStateSections] = item->ustart[kStateSections];
  __syncthreads();
  const uint64_t total = s_start[kStateSections];
  ulonglong2 *rec = (ulonglong2 *)(c.blob + c.offsets[k] + sizeof(StateRecordHeader));
  const uint64_t trip = (uint64_t)kStateCopyThreads * kStateUnroll;
  for (uint64_t u0 = (uint64_t)blockIdx.x * trip; u0 < total; u0 += (uint64_t)gridDim.x * trip) {
    uint64_t *p[kStateUnroll];
    ulonglong2 val[kStateUnroll];
    bool live[kStateUnroll], both[kStateUnroll], wide[kStateUnroll];
#pragma unroll
    for (int j = 0; j < kStateUnroll; j++) {
      const uint64_t u = u0 + (uint64_t)j * kStateCopyThreads + threadIdx.x;
      live[j] = u < total;
      int s = 0;
      for (int t = 1; t < kStateSections; t++) s += (live[j] && s_start[t] <= u) ? 1 : 0;   // ustart is non-decreasing
      const uint64_t i = live[j] ? u - s_start[s] : 0;
      p[j] = s_set[s] + 2 * i;
      both[j] = 2 * i + 1 < s_words[s];
      wide[j] = both[j] && ((uintptr_t)s_set[s] & 15) == 0;
      val[j] = make_ulonglong2(0, 0);
      if (!live[j]) continue;
      if (kImport) {
        val[j] = rec[u];
      } else if (wide[j]) {
        val[j] = *(const ulonglong2 *)p[j];
      } else {
        val[j].x = p[j][0];
        if (both[j]) val[j].y = p[j][1];
      }
    }
#pragma unroll
    for (int j = 0; j < kStateUnroll; j++) {
      if (!live[j]) continue;
      const uint64_t u = u0 + (uint64_t)j * kStateCopyThreads + threadIdx.x;
      if (!kImport) {
        rec[u] = val[j];
      } else if (wide[j]) {
        *(ulonglong2 *)p[j] = val[j];
      } else {
        p[j][0] = val[j].x;
        if (both[j]) p[j][1] = val[j].y;
      }
    }
  }
}

}  // namespace

void launch_state_export(const StateSetView &v, const StateCall &c, int copy_blocks, hipStream_t st) {
  if (c.count <= 0) return;
  hipLaunchKernelGGL(k_state_export_layout, dim3((unsigned)((c.count + 63) / 64)), dim3(64), 0, st, v, c);
  if (c.blob)
    hipLaunchKernelGGL(k_state_copy<false>, dim3((unsigned)copy_blocks, (unsigned)c.count), dim3(kStateCopyThreads), 0, st,
                       v, c);
}

void launch_state_import(const StateSetView &v, const StateCall &c, int copy_blocks, hipStream_t st) {
  if (c.count <= 0) return;
  hipLaunchKernelGGL(k_state_import_layout, dim3((unsigned)((c.count + 63) / 64)), dim3(64), 0, st, v, c);
  hipLaunchKernelGGL(k_state_copy<true>, dim3((unsigned)copy_blocks, (unsigned)c.count), dim3(kStateCopyThreads), 0, st,
                     v, c);
}

}  // namespace tpamd

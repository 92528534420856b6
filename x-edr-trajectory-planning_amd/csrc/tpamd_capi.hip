// tpamd_capi.hip -- C-ABI of the engine (include/tpamd.h): workspace, launches,
// host-buffer convenience paths and per-kernel event timing.
#include "../../include/tpamd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <vector>

#include "tpamd_kernels.h"
#include "tpamd_launch.h"
#include "tpamd_planner_set.h"
#include "tpamd_readout.h"
#include "tpamd_rescale.h"
#include "tpamd_buffer.h"
#include "tpamd_stop.h"
#include "tpamd_switch.h"
#include "tpamd_fit.h"
#include "tpamd_retarget.h"
#include "tpamd_pose_fit.h"
#include "tpamd_joint_fit.h"
#include "tpamd_sweep_joint.h"   // LDS layout, tile size, k_rebuild_time; the kernel instances live in tpamd_sweep_inst.hip
#include "tpamd_check.h"
#include "tpamd_refine.h"
#include "tpamd_state.h"

using namespace tpamd;

namespace {

enum KernelIndex { KI_SETUP = 0, KI_SAMPLE_LP, KI_DETECT, KI_FINAL, KI_SWEEP, KI_EPILOGUE, KI_COUNT };
const char *kKernelNames[KI_COUNT] = {"k_setup", "k_sample_lp", "k_boundary_detect",
                                      "k_boundary_final", "k_sweep", "k_epilogue"};

struct EventPair {
  hipEvent_t start, stop;
  int kernel;
};

#define HIPCHK(expr)                                                              \
  do {                                                                            \
    hipError_t e_ = (expr);                                                       \
    if (e_ != hipSuccess) {                                                       \
      std::fprintf(stderr, "[tpamd] HIP error %s at %s:%d: %s\n", #expr, __FILE__, \
                   __LINE__, hipGetErrorString(e_));                              \
      return TPAMD_E_HIP;                                                         \
    }                                                                             \
  } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// bump allocator over a device layout (with base == null it only sizes)
struct Stage {
  char *base;
  size_t off = 0;
  size_t align;
  explicit Stage(void *b, size_t a = 256) : base((char *)b), align(a) {}
  template <typename T>
  T *take(size_t count) {
    T *p = base ? (T *)(base + off) : nullptr;
    off = align_up(off + count * sizeof(T), align);
    return p;
  }
};

// A device allocation that grows (free, then malloc) and does not keep its contents.
struct DeviceBuffer {
  void *p = nullptr;
  size_t bytes = 0;
  int reserve(size_t need) {
    if (need <= bytes) return 0;
    if (p) HIPCHK(hipFree(p));
    p = nullptr;
    bytes = 0;
    HIPCHK(hipMalloc(&p, need));
    bytes = need;
    return 0;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// The host arrays of one call, staged in one device buffer. Each array is declared once: the
// pointer that receives its device address, the host memory it comes from and/or goes back to,
// its element count. upload() patches every declared pointer and queues the copies up (and the
// zero fills) in declaration order; download() queues the copies down in order and synchronises.
// up / down / both with a null host pointer stage nothing and yield a null device pointer; the
// other forms always stage the array.
// Packed: the arrays declared to go up travel in one copy of a host image of [0, end of the last of
// them), the arrays declared to come back in one copy of their span. Tight: those spans, and
// bytes(), end at the last array's last byte instead of the next alignment boundary.
class HostStage {
 public:
  explicit HostStage(bool packed = false, bool tight = false, size_t align = 256)
      : packed_(packed), tight_(tight), layout_(nullptr, align) {}

  template <typename T> void up(T **dev, const void *host, size_t n) { add(dev, sizeof(T) * n, host, nullptr, kUp, host, false); }
  template <typename T> void down(T **dev, void *host, size_t n) { add(dev, sizeof(T) * n, nullptr, host, kDown, host, false); }
  template <typename T> void both(T **dev, void *host, size_t n) { add(dev, sizeof(T) * n, host, host, kUp | kDown, host, false); }
  template <typename T> void scratch(T **dev, size_t n) { add(dev, sizeof(T) * n, nullptr, nullptr, 0, true, false); }
  // an input the device needs either way: zero-filled when the caller passes none
  template <typename T> void up_or_zero(T **dev, const void *host, size_t n) {
    add(dev, sizeof(T) * n, host, nullptr, kUp, true, true);
  }
  // an output the kernel writes either way: copied back only if the caller asked for it
  template <typename T> void down_or_scratch(T **dev, void *host, size_t n) {
    add(dev, sizeof(T) * n, nullptr, host, kDown, true, false);
  }
  // up from `from` (or zero-filled if `from` is null and `zero`), back to `to` if that is not null
  template <typename T> void up_down(T **dev, const void *from, void *to, size_t n, bool zero = false) {
    add(dev, sizeof(T) * n, from, to, kUp | kDown, true, zero);
  }

  size_t bytes() const { return tight_ ? tight_end_ : layout_.off; }

  int upload(DeviceBuffer &buf, hipStream_t st) {
    if (buf.reserve(bytes())) return TPAMD_E_HIP;
    return upload(buf.p, st);
  }
  int upload(void *base, hipStream_t st) {
    base_ = (char *)base;
    for (const Item &a : items_) {
      char *p = a.staged ? base_ + a.off : nullptr;
      std::memcpy(a.dev, &p, sizeof p);   // dev is the address of a T* of any T
    }
    if (packed_) {
      const size_t end = span_end(up_end_);
      if (end == 0) return 0;
      std::vector<char> image(end, 0);
      for (const Item &a : items_)
        if (a.from && a.bytes) std::memcpy(image.data() + a.off, a.from, a.bytes);
      HIPCHK(hipMemcpyAsync(base_, image.data(), end, hipMemcpyHostToDevice, st));
      return 0;
    }
    for (const Item &a : items_) {
      if (!a.bytes) continue;
      if (a.from) HIPCHK(hipMemcpyAsync(base_ + a.off, a.from, a.bytes, hipMemcpyHostToDevice, st));
      else if (a.zero) HIPCHK(hipMemsetAsync(base_ + a.off, 0, a.bytes, st));
    }
    return 0;
  }
  int download(hipStream_t st) {
    if (packed_ && down_begin_ != SIZE_MAX) {
      std::vector<char> image(span_end(down_end_) - down_begin_);
      HIPCHK(hipMemcpyAsync(image.data(), base_ + down_begin_, image.size(), hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      for (const Item &a : items_)
        if (a.to && a.bytes) std::memcpy(a.to, image.data() + (a.off - down_begin_), a.bytes);
      return 0;
    }
    if (!packed_)
      for (const Item &a : items_)
        if (a.to && a.bytes) HIPCHK(hipMemcpyAsync(a.to, base_ + a.off, a.bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return 0;
  }

 private:
  struct Item {
    void *dev;
    const void *from;
    void *to;
    size_t off, bytes;
    bool staged, zero;
  };
  enum { kUp = 1, kDown = 2 };
  // An array that is not staged takes no bytes but keeps its place: a packed span that it ends,
  // ends at its (aligned) offset.
  void add(void *dev, size_t size, const void *from, void *to, int dir, bool staged, bool zero) {
    const size_t bytes = staged ? size : 0;
    const size_t off = layout_.off;
    layout_.take<char>(bytes);
    items_.push_back(Item{dev, from, to, off, bytes, staged, zero});
    tight_end_ = off + bytes;
    if (dir & kUp) up_end_ = off + bytes;
    if (dir & kDown) {
      down_begin_ = std::min(down_begin_, off);
      down_end_ = off + bytes;
    }
  }
  size_t span_end(size_t end) const { return tight_ ? end : align_up(end, layout_.align); }

  bool packed_, tight_;
  Stage layout_;
  std::vector<Item> items_;
  char *base_ = nullptr;
  size_t tight_end_ = 0, up_end_ = 0, down_begin_ = SIZE_MAX, down_end_ = 0;
};

}  // namespace

struct tpamd_engine {
  int device = 0;
  DeviceBuffer ws_buf;         // the current workspace
  DeviceBuffer stage;          // staging for the _host entry points
  DeviceBuffer rows;           // assembled constraint rows of Cartesian batches
  DeviceBuffer pose_ints;      // the offset arrays of the _device pose-fit / IK-target calls
  hipEvent_t ev_pose = nullptr;   // the last of those calls has read pose_ints
  bool pose_busy = false;
  DeviceBuffer wp_fit;         // waypoint batches (tpamd_time_waypoint_paths_*): the fitted splines, one slot of
                               // the largest control-point count per path, and what the fit knows per path
  DeviceBuffer refine;         // refined calls (tpamd_time_*_paths_refined_*): the sub-batch of slots and their state
  DeviceBuffer refine_ws;      // the workspace of their rounds: the current one keeps what round 0 left in it
  bool rows_for_plan = false;  // rows holds only zeros and rows written by window chaining (of any set on
                               // this engine, under its own split of the buffer: finite values, no more)
  Workspace ws{};
  int last_B = 0, last_N = 0;
  const double *last_time = nullptr;   // out->time of the last solve (tpamd_query_device's check)
  int profile = 0;             // 0 off, 1 every kernel, 2 the sweep kernel only
  bool force_generic = false;  // TPAMD_FORCE_GENERIC=1: A/B the specialised kernels
  bool keep_boundary = false;  // tpamd_debug_keep_boundary
  // Pipelined mode (tpamd_engine_set_pipelining): two workspaces used alternately, the front
  // stage (set-up + sampling/LP kernel) of a joint-space solve runs on the engine's own stream
  // so that it overlaps the sweep of the previous solve.
  int pipelining = 0;          // 0 off, 1 front stage on the engine's stream, 2 sweeps as well
  hipStream_t aux = nullptr;
  hipStream_t sweep_stream[2] = {nullptr, nullptr};
  hipEvent_t ev_front[2] = {nullptr, nullptr}, ev_sweep[2] = {nullptr, nullptr},
             ev_call[2] = {nullptr, nullptr};
  DeviceBuffer ws_spare;       // the workspace of the slot not in use
  // tpamd_planner_set_plan_device leaves solves in flight on the caller's stream when it returns:
  // ev_async is recorded behind them, and every later user of the workspace (SlotGuard) waits for it
  hipEvent_t ev_async = nullptr;
  bool async_pending = false;
  int slot = 0;                // workspace slot e->ws_buf currently refers to
  // Concurrent groups (tpamd_time_joint_groups_*): each lane is a stream of the engine with a
  // workspace of its own; the groups of one call are spread over the lanes and run side by side.
  struct Lane {
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;
    hipEvent_t front = nullptr;   // this lane's sampling/LP kernel has finished
    DeviceBuffer ws;
  };
  static constexpr int kLanes = 4;   // lanes used side by side (the runtime has 4 hardware queues)
  Lane lanes[kLanes];
  hipEvent_t ev_fork = nullptr;
  bool in_lane = false;        // a lane's workspace is swapped in: no slot bookkeeping
  hipEvent_t front_wait = nullptr, front_record = nullptr;   // see tpamd_time_joint_groups_device
  bool order_ragged = true;    // TPAMD_ORDER_RAGGED=0: A/B the longest-first order of ragged batches
  // Idle time in front of a pipelined front stage (TPAMD_FRONT_DELAY_US). The front stage of solve k+1
  // and the sweep of solve k become runnable at the same moment (the sweep of solve k-1 has ended); if
  // the sampling/LP kernel's 16 k blocks reach the CUs first, the sweep's workgroups (35 KB of LDS each)
  // wait for them and the overlap is lost: 0.54 instead of 0.49 ms per step, measured with a front
  // stage that starts 7.5 us after that moment; 10.5 us and everything above (up to 47) give the overlap.
  int front_delay_us = 10;
  // Event timing: pending (start, stop) pairs are folded into acc_ms/acc_n and their events
  // recycled through `pool` once kMaxPendingEvents are outstanding, so a long profiled run
  // holds a bounded number of HIP events.
  std::vector<EventPair> events;
  std::vector<EventPair> pool;
  double acc_ms[KI_COUNT] = {};
  int acc_n[KI_COUNT] = {};
};

namespace {

// Carve the workspace for (B, N, C). Returns the bytes needed; fills ws when base != null.
size_t carve_workspace(char *base, int B, int N, int C, Workspace *ws) {
  Stage s(base);
  const size_t nb = (size_t)B, ns = (size_t)B * N;
  Workspace w{};
  w.ds = s.take<double>(nb);
  w.s_start = s.take<double>(nb);
  w.s_end = s.take<double>(nb);
  w.sd_start = s.take<double>(nb);
  w.sdd_start = s.take<double>(nb);
  w.t_start = s.take<double>(nb);
  w.delta = s.take<double>(nb);
  w.err_bits = s.take<uint32_t>(nb);
  w.lim = s.take<double>(nb * 2 * C);
  // + one tile of records: the sweep's tile prefetch always loads 32 whole records, so the
  // last path's partial tile reads up to 31 records past its end (tpamd_sweep_joint.h)
  w.q12 = s.take<double>((ns + kTileSamples) * (C + 2));
  w.m0 = s.take<double>(ns);
  w.z0 = s.take<double>(ns);
  w.X0 = s.take<double>(ns);
  w.Y0 = s.take<double>(ns);
  w.Xz = s.take<double>(ns);
  w.Yz = s.take<double>(ns);
  w.at0 = s.take<uint8_t>(ns);
  w.fix_flag = s.take<uint8_t>(ns);
  w.fix_val = s.take<double>(ns);
  w.m = s.take<double>(ns);
  w.X = s.take<double>(ns);
  w.Y = s.take<double>(ns);
  w.type = s.take<uint8_t>(ns);
  w.sd2 = s.take<double>(ns);
  w.diag = s.take<long long>(nb * kDiagRow);
  w.order = s.take<int32_t>(nb);
  if (ws) *ws = w;
  return s.off;
}

int ensure_workspace(tpamd_engine *e, int B, int N, int C) {
  const size_t need = carve_workspace(nullptr, B, N, C, nullptr);
  if (need > e->ws_buf.bytes) {
    if (e->ws_buf.reserve(need)) return TPAMD_E_HIP;
  }
  carve_workspace((char *)e->ws_buf.p, B, N, C, &e->ws);
  e->ws.keep_boundary = e->keep_boundary ? 1 : 0;
  return 0;
}

// Pipelined mode: make workspace slot `slot` the current one (e->ws_buf).
void select_slot(tpamd_engine *e, int slot) {
  if (slot == e->slot) return;
  std::swap(e->ws_buf, e->ws_spare);
  e->slot = slot;
}

bool stream_is_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  return hipStreamIsCapturing(st, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone;
}

// Every entry point that touches the CURRENT workspace slot from the caller's stream while the
// engine has streams of its own (a pipelined mode is or was on) goes through this guard: the
// caller's stream first waits for the front stage and the sweep that last used the slot (they may
// still be running on the engine's streams), and the slot's "sweep done" event is re-recorded on
// the caller's stream afterwards, so that the next pipelined front stage that takes the slot is
// ordered behind this user. A stream that is being captured cannot wait for outside events: the
// caller must have fenced the engine before capturing (include/tpamd.h).
struct SlotGuard {
  tpamd_engine *e;
  hipStream_t st;
  int slot;
  bool on;
  SlotGuard(tpamd_engine *e_, hipStream_t st_, bool record_after = true, bool enable = true)
      : e(e_), st(st_), slot(e_->slot),
        on(enable && !e_->in_lane && e_->aux != nullptr && !stream_is_capturing(st_)) {
    // an enqueued-only Plan (tpamd_planner_set_plan_device) may still be using the workspace
    if (e->async_pending && !stream_is_capturing(st)) (void)hipStreamWaitEvent(st, e->ev_async, 0);
    if (!on) return;
    (void)hipStreamWaitEvent(st, e->ev_front[slot], 0);
    (void)hipStreamWaitEvent(st, e->ev_sweep[slot], 0);
    on = record_after;
  }
  ~SlotGuard() {
    if (on) (void)hipEventRecord(e->ev_sweep[slot], st);
  }
};

constexpr size_t kMaxPendingEvents = 512;

// Fold every pending event pair into the per-kernel sums (waits for the recorded work) and
// hand the events back to the pool.
void fold_events(tpamd_engine *e) {
  for (auto &ev : e->events) {
    float ms = 0.f;
    if (hipEventSynchronize(ev.stop) == hipSuccess &&
        hipEventElapsedTime(&ms, ev.start, ev.stop) == hipSuccess) {
      e->acc_ms[ev.kernel] += ms;
      e->acc_n[ev.kernel]++;
    }
    e->pool.push_back(ev);
  }
  e->events.clear();
}

struct Timer {
  tpamd_engine *e;
  hipStream_t st;
  int kernel;
  EventPair ev{};
  bool on;
  Timer(tpamd_engine *e_, hipStream_t st_, int k)
      : e(e_), st(st_), kernel(k), on(e_->profile == 1 || (e_->profile == 2 && k == KI_SWEEP)) {
    if (!on) return;
    if (e->events.size() >= kMaxPendingEvents) fold_events(e);
    if (!e->pool.empty()) {
      ev = e->pool.back();
      e->pool.pop_back();
    } else if (hipEventCreate(&ev.start) != hipSuccess || hipEventCreate(&ev.stop) != hipSuccess) {
      on = false;
      return;
    }
    ev.kernel = kernel;
    (void)hipEventRecord(ev.start, st);
  }
  ~Timer() {
    if (on) {
      (void)hipEventRecord(ev.stop, st);
      e->events.push_back(ev);
    }
  }
};

// Makes e->device current for the duration of an entry point and restores the caller's
// device afterwards (the caller may be PyTorch with another device current).
struct DeviceScope {
  int prev = -1;
  hipError_t err;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = (prev == device) ? hipSuccess : hipSetDevice(device);
    if (prev == device) prev = -1;   // nothing to restore
  }
  ~DeviceScope() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};
#define TPAMD_ON_DEVICE(e)          \
  DeviceScope device_scope_((e)->device); \
  HIPCHK(device_scope_.err)

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel: it is set
// for every kernel that can ask for more than 64 KB of LDS, once per device ordinal, when the
// first engine on that device is created (thread-safe; a failure is reported).
constexpr int kMaxDevices = 64;
constexpr size_t kSampleLpLdsLimitBytes = 160 * 1024;   // the LDS of one CU: the sampling/LP kernel's limit
std::mutex g_config_mutex;
bool g_device_configured[kMaxDevices] = {};

template <typename K>
hipError_t allow_big_lds(K kernel, int bytes = 160 * 1024) {
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
}

// The current device must be `device`.
int configure_kernels_for_device(int device) {
  if (device < 0 || device >= kMaxDevices) return TPAMD_E_INVALID_ARGUMENT;
  std::lock_guard<std::mutex> lock(g_config_mutex);
  if (g_device_configured[device]) return 0;
#define TPAMD_BIG_LDS(...) HIPCHK(allow_big_lds(__VA_ARGS__))
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 0>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 3>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 4>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 5>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 6>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 7>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 8>);
  TPAMD_BIG_LDS(k_sample_lp_joint<1, 14>);
  TPAMD_BIG_LDS(k_sample_lp_joint_wide<1, 14>);
  TPAMD_BIG_LDS(k_lp_rows<1>);
  TPAMD_BIG_LDS(k_lp_rows<2>);
  TPAMD_BIG_LDS(k_sweep<JointSource>);
  TPAMD_BIG_LDS(k_sweep<GenericSource>);
#define TPAMD_CONFIGURE_SWEEP(D, E) HIPCHK((configure_sweep_joint<D, E>()));
  TPAMD_SWEEP_INSTANCES(TPAMD_CONFIGURE_SWEEP)
#undef TPAMD_CONFIGURE_SWEEP
  TPAMD_BIG_LDS(k_cartesian_lp<1, 6>);
  TPAMD_BIG_LDS(k_cartesian_lp<1, 7>);
  TPAMD_BIG_LDS(k_cartesian_lp<1, 6, true>);
  TPAMD_BIG_LDS(k_cartesian_lp<1, 7, true>);
  // (the kernel has static LDS of its own; what a spline the solve accepts needs lies 2 * D * 64 * 8 bytes and
  // more below the sampling/LP kernel's limit)
  TPAMD_BIG_LDS(k_check_joint, (int)kSampleLpLdsLimitBytes - 1024);
  TPAMD_BIG_LDS(k_pset_check_joint, (int)kSampleLpLdsLimitBytes - 1024);
#undef TPAMD_BIG_LDS
  g_device_configured[device] = true;
  return 0;
}

// Joint counts with a specialised sweep kernel (which also runs the boundary passes 2-4 of
// its path and the planner epilogue).
bool has_joint_sweep(int D) { return (D >= 3 && D <= 8) || D == 14; }

// The sweep launch: joint-space batches with D in {3..8, 14} take the specialised kernel
// (6, 7, 14 are the BASELINE.json configurations), everything else the generic one.
// Returns true if the kernel also wrote qd/qdd (the planner epilogue).
template <class Source>
bool launch_sweep(hipStream_t st, int B, int N, int max_loops, const Source &src,
                  const Workspace &ws, const tpamd_path_outputs *out, bool /*force_generic*/) {
  const size_t lds = (2 * (size_t)N + 64) * sizeof(double);
  hipLaunchKernelGGL((k_sweep<Source>), dim3(B), dim3(64), lds, st, N, max_loops, src, ws,
                     out->time, out->s, out->sd, out->sdd, out->last_extremal_index,
                     out->max_time_increment, out->status);
  return false;
}

template <>
bool launch_sweep<JointSource>(hipStream_t st, int B, int N, int max_loops, const JointSource &src,
                               const Workspace &ws, const tpamd_path_outputs *out,
                               bool force_generic) {
#define TPAMD_LAUNCH_JOINT(DD)                                              \
  do {                                                                      \
    launch_sweep_joint<DD, 0>(B, st, N, max_loops, src, ws, out);           \
    return true;                                                            \
  } while (0)
  if (!force_generic) {
    switch (src.D) {
      case 3: TPAMD_LAUNCH_JOINT(3);
      case 4: TPAMD_LAUNCH_JOINT(4);
      case 5: TPAMD_LAUNCH_JOINT(5);
      case 6: TPAMD_LAUNCH_JOINT(6);
      case 7: TPAMD_LAUNCH_JOINT(7);
      case 8: TPAMD_LAUNCH_JOINT(8);
      case 14: TPAMD_LAUNCH_JOINT(14);
      default: break;
    }
  }
#undef TPAMD_LAUNCH_JOINT
  const size_t lds = (2 * (size_t)N + 64) * sizeof(double);
  hipLaunchKernelGGL((k_sweep<JointSource>), dim3(B), dim3(64), lds, st, N, max_loops, src, ws,
                     out->time, out->s, out->sd, out->sdd, out->last_extremal_index,
                     out->max_time_increment, out->status);
  return false;
}

template <class Source> bool sweep_runs_boundary_passes(const tpamd_engine *, const Source &) { return false; }
template <> bool sweep_runs_boundary_passes<JointSource>(const tpamd_engine *e, const JointSource &src) {
  return !e->force_generic && has_joint_sweep(src.D);
}

// Shared tail: boundary passes 2-4 (separate kernels unless the sweep kernel runs them itself)
// -> sweep (-> epilogue in joint mode).
template <class Source>
int run_boundary_and_sweep(tpamd_engine *e, hipStream_t st, int B, int N, int max_loops,
                           const Source &src, const tpamd_path_outputs *out,
                           bool *epilogue_done = nullptr) {
  e->ws.sd2_out = out->sd2;
  const Workspace &ws = e->ws;
  const dim3 grid_s((N + 255) / 256, B);
  if (!sweep_runs_boundary_passes(e, src)) {
    {
      Timer t(e, st, KI_DETECT);
      hipLaunchKernelGGL((k_boundary_zfit<Source>), grid_s, dim3(256), 0, st, N, src, ws);
      hipLaunchKernelGGL(k_boundary_detect, grid_s, dim3(256), 0, st, N, ws);
    }
    {
      Timer t(e, st, KI_FINAL);
      hipLaunchKernelGGL((k_boundary_final<Source>), grid_s, dim3(256), 0, st, N, src, ws);
    }
  }
  {
    Timer t(e, st, KI_SWEEP);
    const bool fused = launch_sweep(st, B, N, max_loops, src, ws, out, e->force_generic);
    if (epilogue_done) *epilogue_done = fused;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// Cartesian batches with D in {6, 7}: records carry two extra B-only rows.
template <int DD>
void launch_sweep_cartesian(hipStream_t st, int B, int N, int max_loops, const JointSource &src,
                            const Workspace &ws, const tpamd_path_outputs *out) {
  launch_sweep_joint<DD, 2>(B, st, N, max_loops, src, ws, out);
}

// LP boundary points of explicit rows, then the shared tail.
int run_rows(tpamd_engine *e, hipStream_t st, int B, int N, int C, int max_loops, const double *a,
             const double *b, const double *lower, const double *upper,
             const tpamd_path_outputs *out) {
  const Workspace &ws = e->ws;
  {
    Timer t(e, st, KI_SAMPLE_LP);
    const int tpb = 64;
    const size_t lds = 4 * (size_t)C * tpb * 8;
    const dim3 grid((N + tpb - 1) / tpb, B);
    if (C <= 32)
      hipLaunchKernelGGL((k_lp_rows<1>), grid, dim3(tpb), lds, st, N, C, a, b, lower, upper, ws);
    else
      hipLaunchKernelGGL((k_lp_rows<2>), grid, dim3(tpb), lds, st, N, C, a, b, lower, upper, ws);
  }
  GenericSource src;
  src.A = a; src.B = b; src.LO = lower; src.HI = upper; src.C = C;
  return run_boundary_and_sweep(e, st, B, N, max_loops, src, out);
}

}  // namespace

extern "C" {

int tpamd_version(void) { return TPAMD_VERSION; }

const char *tpamd_error_string(int code) {
  switch (code) {
    case 0: return "ok";
    case TPAMD_E_INVALID_ARGUMENT: return "invalid argument";
    case TPAMD_E_HIP: return "HIP runtime error";
    case TPAMD_E_UNSUPPORTED: return "unsupported size";
    case TPAMD_E_NO_DEVICE: return "no HIP device";
    case TPAMD_E_STALE: return "engine state belongs to a different solve";
    case TPAMD_PATH_INFEASIBLE_BOUNDS: return "infeasible bounds: no upper > lower at a sample";
    case TPAMD_PATH_S_RANGE: return "s_start must be < s_end";
    case TPAMD_PATH_SD_START_NEGATIVE: return "sd_start must be >= 0";
    case TPAMD_PATH_LOWER_GE_UPPER: return "constraints must satisfy lower < upper";
    case TPAMD_PATH_TOO_FEW_SAMPLES: return "need at least 2 samples";
    case TPAMD_PATH_NO_CONNECTION: return "could not connect from critical point to initial trajectory portion";
    case TPAMD_PATH_NAN_SD2: return "no solution found (NaN in sd2)";
    case TPAMD_PATH_NONZERO_END: return "non-zero terminal velocity";
    case TPAMD_PATH_CRIT_INDEX_ZERO: return "critical point search degenerated to index 0";
    case TPAMD_PATH_NO_WAYPOINTS: return "path without waypoints";
    case TPAMD_PATH_SWEEP_POLL_EXPIRED: return "internal error: a bounded wait inside the sweep kernel ran out";
    default: return "unknown";
  }
}

int tpamd_device_count(void) {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count < 0) return 0;
  return count;
}

void tpamd_shard_bounds(int num_paths, int num_shards, int32_t *begin) {
  if (!begin || num_shards <= 0) return;
  const int total = num_paths > 0 ? num_paths : 0;
  const int base = total / num_shards, rem = total % num_shards;
  for (int r = 0; r <= num_shards; r++) begin[r] = r * base + (r < rem ? r : rem);
}

void tpamd_shard_bounds_balanced(int num_paths, const double *cost, int num_shards, int32_t *begin) {
  if (!begin || num_shards <= 0) return;
  const int n = (num_paths > 0 && cost) ? num_paths : 0;
  double total = 0.0;
  for (int i = 0; i < n; i++) total += cost[i];
  int k = 1, lo = 0;
  double acc = 0.0;
  begin[0] = 0;
  for (int i = 0; i < n; i++) {
    acc += cost[i];
    const int remaining_items = n - (i + 1), remaining_blocks = num_shards - k;
    if (k < num_shards && (acc >= total * k / num_shards || remaining_items == remaining_blocks)) {
      begin[k] = i + 1;
      lo = i + 1;
      k++;
    }
  }
  (void)lo;
  for (; k <= num_shards; k++) begin[k] = n;
}

int tpamd_engine_create(int device_ordinal, tpamd_engine **out) {
  if (!out) return TPAMD_E_INVALID_ARGUMENT;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
    std::fprintf(stderr, "[tpamd] no HIP device available: the engine has no CPU fallback\n");
    return TPAMD_E_NO_DEVICE;
  }
  if (device_ordinal < 0 || device_ordinal >= count) return TPAMD_E_INVALID_ARGUMENT;
  DeviceScope scope(device_ordinal);
  HIPCHK(scope.err);
  const int rc = configure_kernels_for_device(device_ordinal);
  if (rc) return rc;
  tpamd_engine *e = new (std::nothrow) tpamd_engine();
  if (!e) return TPAMD_E_HIP;
  e->device = device_ordinal;
  {
    const char *fg = std::getenv("TPAMD_FORCE_GENERIC");
    e->force_generic = fg && fg[0] == '1';
    const char *fd = std::getenv("TPAMD_FRONT_DELAY_US");
    if (fd && std::atoi(fd) >= 0 && std::atoi(fd) <= 1000) e->front_delay_us = std::atoi(fd);
    const char *orr = std::getenv("TPAMD_ORDER_RAGGED");
    e->order_ragged = !(orr && orr[0] == '0');
  }
  *out = e;
  return 0;
}

void tpamd_engine_destroy(tpamd_engine *e) {
  if (!e) return;
  DeviceScope scope(e->device);
  for (auto *v : {&e->events, &e->pool})
    for (auto &ev : *v) { (void)hipEventDestroy(ev.start); (void)hipEventDestroy(ev.stop); }
  e->ws_buf.release();
  e->ws_spare.release();
  for (int k = 0; k < 2; k++) {
    if (e->ev_front[k]) (void)hipEventDestroy(e->ev_front[k]);
    if (e->ev_sweep[k]) (void)hipEventDestroy(e->ev_sweep[k]);
    if (e->ev_call[k]) (void)hipEventDestroy(e->ev_call[k]);
    if (e->sweep_stream[k]) (void)hipStreamDestroy(e->sweep_stream[k]);
  }
  if (e->aux) (void)hipStreamDestroy(e->aux);
  for (auto &ln : e->lanes) {
    if (ln.stream) (void)hipStreamDestroy(ln.stream);
    if (ln.done) (void)hipEventDestroy(ln.done);
    if (ln.front) (void)hipEventDestroy(ln.front);
    ln.ws.release();
  }
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_async) (void)hipEventDestroy(e->ev_async);
  e->stage.release();
  e->rows.release();
  e->pose_ints.release();
  e->wp_fit.release();
  e->refine.release();
  e->refine_ws.release();
  if (e->ev_pose) (void)hipEventDestroy(e->ev_pose);
  delete e;
}

int tpamd_engine_reserve(tpamd_engine *e, int B, int N, int C) {
  if (!e || B <= 0 || N <= 0 || C <= 0) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  int rc = ensure_workspace(e, B, N, C);
  if (rc == 0 && e->pipelining) {       // both workspaces of the pipelined mode
    select_slot(e, 1 - e->slot);
    rc = ensure_workspace(e, B, N, C);
  }
  return rc;
}

size_t tpamd_engine_workspace_bytes(const tpamd_engine *e) { return e ? e->ws_buf.bytes : 0; }

}  // extern "C"

namespace {
// The checks of a joint batch (after the null structs and B <= 0), shared with the _host entries.
int joint_args(const tpamd_joint_batch *bt, const tpamd_joint_inputs *in, const tpamd_path_outputs *out) {
  const int D = bt->num_dofs, N = bt->num_samples, P = bt->num_points;
  if (D < 1 || D > 16 || N < 3 || N > 8192 || P < 3) return TPAMD_E_UNSUPPORTED;
  if (!in->knots || !in->control_points || !in->max_velocity || !in->max_acceleration ||
      !in->path_start || !in->delta || !in->sd_start || !in->time_start || !out->time ||
      !out->s || !out->sd || !out->sdd || !out->status)
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// Block size of the sampling/LP kernel and the LDS it then needs for paths of up to P control points.
int sample_lp_block(bool piped, bool ragged, int D) {
  if (piped) return 128;
  return ragged ? 64 : (D <= 7 ? 256 : (D < 14 ? 128 : 64));
}
size_t sample_lp_lds(int P, int D, int tpb) {
  return ((size_t)(P + 3) + (size_t)P * D + 2 * (size_t)(2 * D) + 2 * (size_t)D * tpb) * 8;
}
constexpr size_t kSampleLpLdsLimit = kSampleLpLdsLimitBytes;

// Waypoint batches (tpamd_time_waypoint_paths_*): the splines were fitted on the device into slots
// of p_stride control points; path k has np[k] of them, 0 if it has no waypoints.
struct FittedPaths {
  const int32_t *np;
  int p_stride;
  bool any_empty;
};

// The joint-space solve; `plan` (window chaining, tpamd_plan_joint_windows_host) adds two small
// kernels: skip marks after the set-up kernel, the start-velocity projection after K1. `fitted`
// (waypoint batches) gives every path its own control-point count, as a planner set does, and adds
// one small kernel behind the set-up kernel if a path has no waypoints. `skip_zero_samples` (the rounds
// of a refined call, tpamd_refine.h) adds the same kernel on the sample counts: a path whose count
// is 0 takes no part and its outputs stay as they are.
int solve_joint(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                const tpamd_path_outputs *out, void *hip_stream, const PlanParams *plan,
                bool allow_pipelining = true, const FittedPaths *fitted = nullptr,
                bool skip_zero_samples = false) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  const int B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples, P = bt->num_points;
  if (B <= 0) return B == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = joint_args(bt, in, out)) return rc;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  const int C = 2 * D;
  // Pipelined mode: this solve takes the workspace the previous one did not use, and its front
  // stage goes to the engine's stream, ordered only behind the sweep that last used this
  // workspace -- not behind the caller's stream (see tpamd_engine_set_pipelining). A stream that
  // is being captured into a graph cannot fork into the engine's stream: plain order then.
  bool piped = e->pipelining != 0 && plan == nullptr && allow_pipelining;
  if (piped && stream_is_capturing(st)) piped = false;
  // the block size of the sampling/LP kernel and its LDS: checked before anything is launched or
  // the workspace slot changes
  const int tpb = sample_lp_block(piped, in->num_samples_per_path != nullptr, D);
  const size_t lds = sample_lp_lds(P, D, tpb);
  if (lds > kSampleLpLdsLimit) return TPAMD_E_UNSUPPORTED;
  if (piped) select_slot(e, 1 - e->slot);
  const int slot = e->slot;
  // an unpipelined solve on an engine with streams of its own: ordered against them
  SlotGuard slot_guard(e, st, /*record_after=*/true, /*enable=*/!piped);
  int rc = ensure_workspace(e, B, N, C);
  if (rc) return rc;
  e->last_B = B; e->last_N = N; e->last_time = out->time;
  e->ws.ns = in->num_samples_per_path;
  e->ws.amax = in->max_acceleration;
  // planner sets: paths of their own sizes in arrays of stride P_cap; P is the largest in use
  e->ws.np = plan ? plan->np : nullptr;
  e->ws.p_stride = (plan && plan->np) ? plan->K - 3 : P;
  if (fitted) {
    e->ws.np = fitted->np;
    e->ws.p_stride = fitted->p_stride;
  }
  // ragged batches: sweep workgroups take the paths longest first (k_order_paths, below)
  int32_t *order = const_cast<int32_t *>(e->ws.order);
  const bool ordered = in->num_samples_per_path != nullptr && B > 1 && e->order_ragged && plan == nullptr;
  if (!ordered) e->ws.order = nullptr;
  const Workspace &ws = e->ws;
  const int max_loops = bt->max_solver_loops > 0 ? bt->max_solver_loops : 0;  // 0: per path, max(100, 10 n)
  hipStream_t fs = st;                  // stream of the front stage
  if (piped) {
    fs = e->aux;
    HIPCHK(hipStreamWaitEvent(fs, e->ev_sweep[slot], 0));
  }
  if (piped && e->front_delay_us > 0)
    hipLaunchKernelGGL(k_delay, dim3(1), dim3(64), 0, fs, e->front_delay_us * 100);
  {
    Timer t(e, fs, KI_SETUP);
    hipLaunchKernelGGL(k_setup_joint, dim3((B + 127) / 128), dim3(128), 0, fs, B, N, D,
                       bt->constraint_safety, in->max_velocity, in->max_acceleration,
                       in->path_start, in->delta, in->sd_start, in->sdd_start, in->time_start,
                       ws);
    if (plan)
      hipLaunchKernelGGL(k_plan_mark_skipped, dim3((B + 127) / 128), dim3(128), 0, fs, *plan, ws);
    if (fitted && fitted->any_empty) launch_skip_empty_paths(B, fitted->np, ws.err_bits, fs);
    if (skip_zero_samples && in->num_samples_per_path)
      launch_skip_empty_paths(B, in->num_samples_per_path, ws.err_bits, fs);
    if (ordered)
      hipLaunchKernelGGL(k_order_paths, dim3(1), dim3(1024), 0, fs, B, N, in->num_samples_per_path, order);
  }
  if (e->front_wait) HIPCHK(hipStreamWaitEvent(fs, e->front_wait, 0));
  {
    Timer t(e, fs, KI_SAMPLE_LP);
    // (tpb, above) 128 threads (16 KB of LDS at D = 7) fit next to four resident sweep workgroups
    // of an earlier solve. Otherwise the block size follows the record width (measured, K1 alone:
    // D <= 7 0.166 / 0.174 / 0.186 ms at 256 / 128 / 64 threads; D = 14, N = 4000 0.765 / 0.734 /
    // 0.661 ms) and ragged batches take 64-thread blocks (fewer idle threads behind a path's end:
    // the mixed-DOF share of configs[4] 2.96 -> 2.60 ms).
    const dim3 grid((N + tpb - 1) / tpb, B);
#define TPAMD_K1(DD)                                                                         \
  hipLaunchKernelGGL((k_sample_lp_joint<1, DD>), grid, dim3(tpb), lds, fs, N, D, P, in->knots, \
                     in->control_points, out->q, ws)
    if (D == 7 && !e->force_generic) TPAMD_K1(7);
    else if (D == 6 && !e->force_generic) TPAMD_K1(6);
    else if (D == 14 && !e->force_generic)
      hipLaunchKernelGGL((k_sample_lp_joint_wide<1, 14>), grid, dim3(tpb), lds, fs, N, D, P, in->knots,
                         in->control_points, out->q, ws);
    else if (D == 3 && !e->force_generic) TPAMD_K1(3);
    else if (D == 4 && !e->force_generic) TPAMD_K1(4);
    else if (D == 5 && !e->force_generic) TPAMD_K1(5);
    else if (D == 8 && !e->force_generic) TPAMD_K1(8);
    else TPAMD_K1(0);
#undef TPAMD_K1
    if (plan) hipLaunchKernelGGL(k_plan_project, dim3((B + 127) / 128), dim3(128), 0, fs, *plan, ws);
  }
  if (e->front_record) HIPCHK(hipEventRecord(e->front_record, fs));
  // Mode 2: the sweep goes to one of two engine streams as well, so that it can start while the
  // previous solve's slowest paths are still running; it is ordered behind this call's position
  // in the caller's stream (the output buffers are free) and behind its own front stage. The
  // caller's stream is made to wait for the PREVIOUS solve only (tpamd_engine_fence for the rest).
  const bool deferred = piped && e->pipelining == 2;
  hipStream_t caller = st;
  if (piped) {
    HIPCHK(hipEventRecord(e->ev_front[slot], fs));
    if (deferred) {
      HIPCHK(hipEventRecord(e->ev_call[slot], caller));
      st = e->sweep_stream[slot];
      HIPCHK(hipStreamWaitEvent(st, e->ev_call[slot], 0));
    }
    HIPCHK(hipStreamWaitEvent(st, e->ev_front[slot], 0));
  }
  JointSource src;
  src.q12 = ws.q12; src.lim = ws.lim; src.D = D;
  bool fused = false;
  rc = run_boundary_and_sweep(e, st, B, N, max_loops, src, out, &fused);
  if (rc) {
    if (piped) (void)hipEventRecord(e->ev_sweep[slot], st);   // the slot's next user waits for what was launched
    return rc;
  }
  if (!fused && (out->qd || out->qdd)) {   // the specialised sweep kernels write qd/qdd themselves
    Timer t(e, st, KI_EPILOGUE);
    const size_t total = (size_t)B * N * D;
    hipLaunchKernelGGL(k_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, B, N,
                       D, ws.q12, out->sd, out->sdd, in->max_acceleration, out->status, ws.ns,
                       out->qd, out->qdd);
  }
  if (piped) HIPCHK(hipEventRecord(e->ev_sweep[slot], st));
  if (deferred) HIPCHK(hipStreamWaitEvent(caller, e->ev_sweep[1 - slot], 0));
  HIPCHK(hipGetLastError());
  return 0;
}
}  // namespace

extern "C" {

int tpamd_time_joint_paths_device(tpamd_engine *e, const tpamd_joint_batch *bt,
                                  const tpamd_joint_inputs *in, const tpamd_path_outputs *out,
                                  void *hip_stream) {
  return solve_joint(e, bt, in, out, hip_stream, nullptr);
}

int tpamd_plan_joint_windows_host(tpamd_engine *e, const tpamd_plan_args *a) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_planners <= 0) return a->num_planners == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  const size_t B = a->num_planners, D = a->num_dofs, N = a->num_samples, P = a->num_points,
               cap = a->history_capacity;
  if (D < 1 || D > 16 || N < 3 || N > 8192 || P < 3 || cap < N) return TPAMD_E_UNSUPPORTED;
  if (!a->knots || !a->control_points || !a->max_velocity || !a->max_acceleration || !a->delta ||
      !a->initial_velocity || !a->start_ns || !a->horizon_ns || !a->path_state || !a->planned_to_end ||
      !a->history_count || !a->history_time || !a->history_s || !a->history_sd || !a->history_sdd ||
      !a->history_q || !a->history_qd || !a->history_qdd || !a->path_horizon || !a->final_decel_start_ns ||
      !a->window_time || !a->window_s || !a->window_sd || !a->window_sdd || !a->window_sd2 || !a->window_q ||
      !a->window_q1 || !a->window_q2 || !a->window_path_start || !a->window_sd_start ||
      !a->window_time_start || !a->window_last_extremal_index || !a->window_max_time_increment ||
      !a->status || !a->windows || !a->loop_start_ns || !a->loop_count || !a->looping)
    return TPAMD_E_INVALID_ARGUMENT;
  for (size_t b = 0; b < B; b++)
    if (a->history_count[b] < 0 || (size_t)a->history_count[b] > cap) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  // loop state: a planner loops while it has not planned to the end (:632); nothing solved yet
  std::vector<int> act(B), zero(B, 0);
  int n_active = 0;
  for (size_t b = 0; b < B; b++) {
    act[b] = a->resume ? (a->looping[b] != 0) : (a->planned_to_end[b] ? 0 : 1);
    n_active += act[b];
  }
  PlanParams p{};
  tpamd_joint_inputs din{};
  tpamd_path_outputs dout{};
  double *w_q1 = nullptr, *w_q2 = nullptr;
  HostStage s;
  s.up(&p.knots, a->knots, B * (P + 3));
  s.up(&din.control_points, a->control_points, B * P * D);
  s.up(&din.max_velocity, a->max_velocity, B * D);
  s.up(&din.max_acceleration, a->max_acceleration, B * D);
  s.up(&p.delta, a->delta, B);
  s.up(&p.initial_velocity, a->initial_velocity, B * D);
  s.up(&p.start_ns, a->start_ns, B);
  s.up(&p.horizon_ns, a->horizon_ns, B);
  s.up_down(&p.loop_start_ns, a->resume ? a->loop_start_ns : a->start_ns, a->loop_start_ns, B);   // :630
  s.both(&p.final_decel_start_ns, a->final_decel_start_ns, B);
  s.both(&p.path_state, a->path_state, B);
  s.both(&p.count, a->history_count, B);
  s.both(&p.planned_to_end, a->planned_to_end, B);
  s.both(&p.path_horizon, a->path_horizon, B);
  s.both(&p.h_time, a->history_time, B * cap);
  s.both(&p.h_s, a->history_s, B * cap);
  s.both(&p.h_sd, a->history_sd, B * cap);
  s.both(&p.h_sdd, a->history_sdd, B * cap);
  s.both(&p.h_q, a->history_q, B * cap * D);
  s.both(&p.h_qd, a->history_qd, B * cap * D);
  s.both(&p.h_qdd, a->history_qdd, B * cap * D);
  s.up_down(&p.active, act.data(), act.data(), B);
  s.up(&p.old_state, zero.data(), B);
  s.up(&p.offset, zero.data(), B);
  s.up_down(&p.loop, zero.data(), a->loop_count, B);
  s.up(&p.append, zero.data(), B);
  s.up_down(&p.windows, zero.data(), a->windows, B);
  s.up_down(&p.status, zero.data(), a->status, B);
  s.scratch(&p.num_active, 1);
  s.up_down(&p.path_start, nullptr, a->window_path_start, B, /*zero=*/true);
  s.up_down(&p.sd_start, nullptr, a->window_sd_start, B, /*zero=*/true);
  s.up_down(&p.time_start, nullptr, a->window_time_start, B, /*zero=*/true);
  s.up_or_zero(&din.sdd_start, nullptr, B);
  s.up_down(&dout.time, nullptr, a->window_time, B * N, /*zero=*/true);
  s.down(&dout.s, a->window_s, B * N);
  s.down(&dout.sd, a->window_sd, B * N);
  s.down(&dout.sdd, a->window_sdd, B * N);
  s.down(&dout.sd2, a->window_sd2, B * N);
  s.down(&dout.q, a->window_q, B * N * D);
  s.scratch(&dout.qd, B * N * D);
  s.scratch(&dout.qdd, B * N * D);
  s.down(&w_q1, a->window_q1, B * N * D);
  s.down(&w_q2, a->window_q2, B * N * D);
  s.up_down(&dout.last_extremal_index, nullptr, a->window_last_extremal_index, B, /*zero=*/true);
  s.up_down(&dout.max_time_increment, nullptr, a->window_max_time_increment, B, /*zero=*/true);
  s.scratch(&dout.status, B);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  // resuming: the caller's loop counts replace the zeros
  if (a->resume) HIPCHK(hipMemcpyAsync(p.loop, a->loop_count, B * 4, hipMemcpyHostToDevice, st));
  p.B = (int)B; p.N = (int)N; p.D = (int)D; p.K = (int)P + 3; p.cap = (int)cap;
  p.max_iterations = a->max_planning_iterations;
  p.max_initial_velocity_error = a->max_initial_velocity_error;
  p.w_time = dout.time; p.w_s = dout.s; p.w_sd = dout.sd; p.w_sdd = dout.sdd; p.w_q = dout.q; p.w_qd = dout.qd;
  p.w_qdd = dout.qdd; p.w_status = dout.status; p.w_lei = dout.last_extremal_index;
  din.knots = p.knots; din.path_start = p.path_start; din.delta = p.delta; din.sd_start = p.sd_start;
  din.time_start = p.time_start;
  tpamd_joint_batch bt{(int)B, (int)D, (int)N, (int)P, 0, 0, a->constraint_safety};
  const unsigned gb = (unsigned)((B + 127) / 128);
  bool any_window = false;
  {
    bool full = false;
    for (size_t b = 0; b < B; b++)
      if (act[b] && (size_t)a->history_count[b] + N > cap) full = true;
    if (full) n_active = 0;           // reported as TPAMD_PLAN_MORE below (p.active is untouched)
  }
  while (n_active > 0) {
    // every planner's history must be able to take one more window wherever it connects
    hipLaunchKernelGGL(k_plan_begin, dim3(gb), dim3(128), 0, st, p, e->ws);
    rc = solve_joint(e, &bt, &din, &dout, st, &p);
    if (rc) return rc;
    any_window = true;
    HIPCHK(hipMemsetAsync(p.num_active, 0, 4, st));
    hipLaunchKernelGGL(k_plan_end, dim3(gb), dim3(128), 0, st, p);
    hipLaunchKernelGGL(k_plan_append, dim3((unsigned)((N + 127) / 128), (unsigned)B), dim3(128), 0, st, p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n_active, p.num_active, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_active > 0) {
      // capacity for the next round: count + N must fit for every looping planner
      std::vector<int> cnt(B), actv(B);
      HIPCHK(hipMemcpy(cnt.data(), p.count, B * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(actv.data(), p.active, B * 4, hipMemcpyDeviceToHost));
      bool full = false;
      for (size_t b = 0; b < B; b++)
        if (actv[b] && (size_t)cnt[b] + N > cap) full = true;
      if (full) break;      // the caller continues with a larger history (status stays 0, planners stay looping)
    }
  }
  if (any_window) {
    const size_t total = B * N * D;
    hipLaunchKernelGGL(k_unpack_records, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (int)B, (int)N,
                       (int)D, e->ws.q12, w_q1, w_q2);
    HIPCHK(hipGetLastError());
  } else {
    HIPCHK(hipMemsetAsync(w_q1, 0, B * N * D * 8, st));
    HIPCHK(hipMemsetAsync(w_q2, 0, B * N * D * 8, st));
  }
  rc = s.download(st);
  if (rc) return rc;
  // planners that are still looping stopped because a history is full
  for (size_t b = 0; b < B; b++) {
    a->looping[b] = act[b];
    if (a->status[b] == 0 && act[b]) a->status[b] = TPAMD_PLAN_MORE;
  }
  return 0;
}

int tpamd_engine_fence(tpamd_engine *e, void *hip_stream) {
  if (!e) return TPAMD_E_INVALID_ARGUMENT;
  if (!e->aux) return 0;
  TPAMD_ON_DEVICE(e);
  for (int k = 0; k < 2; k++) HIPCHK(hipStreamWaitEvent((hipStream_t)hip_stream, e->ev_sweep[k], 0));
  return 0;
}

int tpamd_engine_set_pipelining(tpamd_engine *e, int on) {
  if (!e || on < 0 || on > 2) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  if (on && !e->aux) {
    // lowest priority: the front stage of the NEXT solve fills what the running sweep leaves
    // free; it must not take workgroup slots from a sweep that is being dispatched
    int least = 0, greatest = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
    HIPCHK(hipStreamCreateWithPriority(&e->aux, hipStreamNonBlocking, least));
    for (int k = 0; k < 2; k++) {
      HIPCHK(hipEventCreateWithFlags(&e->ev_front[k], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&e->ev_sweep[k], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&e->ev_call[k], hipEventDisableTiming));
    }
  }
  // The sweep streams exist only once mode 2 is asked for: the runtime multiplexes streams onto a
  // few hardware queues, and one more idle stream was measured to put the engine's stream on the
  // caller's queue -- serialising exactly the two things mode 1 overlaps (0.66 -> 0.93 ms per step).
  if (on == 2)
    for (int k = 0; k < 2; k++)
      if (!e->sweep_stream[k]) HIPCHK(hipStreamCreateWithFlags(&e->sweep_stream[k], hipStreamNonBlocking));
  if (e->pipelining && on != e->pipelining) {   // leave the old mode with nothing in flight
    HIPCHK(hipStreamSynchronize(e->aux));
    for (int k = 0; k < 2; k++)
      if (e->sweep_stream[k]) HIPCHK(hipStreamSynchronize(e->sweep_stream[k]));
  }
  e->pipelining = on;
  return 0;
}

}  // extern "C"

namespace {
// The outputs of one solve in `s`; dout receives their device addresses. Every _host solve
// entry stages its outputs this way.
// `keep`: the per-sample arrays travel up first, so that entries the solve does not write (beyond a
// ragged path's count) come back as the caller had them.
void stage_path_outputs(HostStage &s, size_t B, size_t N, size_t D, const tpamd_path_outputs *out,
                        tpamd_path_outputs *dout, bool keep = false) {
  if (keep) {
    s.both(&dout->time, out->time, B * N);
    s.both(&dout->s, out->s, B * N);
    s.both(&dout->sd, out->sd, B * N);
    s.both(&dout->sdd, out->sdd, B * N);
    s.both(&dout->q, out->q, B * N * D);
    s.both(&dout->qd, out->qd, B * N * D);
    s.both(&dout->qdd, out->qdd, B * N * D);
  } else {
    s.down(&dout->time, out->time, B * N);
    s.down(&dout->s, out->s, B * N);
    s.down(&dout->sd, out->sd, B * N);
    s.down(&dout->sdd, out->sdd, B * N);
    s.down(&dout->q, out->q, B * N * D);
    s.down(&dout->qd, out->qd, B * N * D);
    s.down(&dout->qdd, out->qdd, B * N * D);
  }
  s.down_or_scratch(&dout->last_extremal_index, out->last_extremal_index, B);
  s.down_or_scratch(&dout->max_time_increment, out->max_time_increment, B);
  s.down(&dout->status, out->status, B);
  if (keep) s.both(&dout->sd2, out->sd2, B * N);
  else s.down(&dout->sd2, out->sd2, B * N);
}

// The checks of a rows batch after the null structs and B <= 0 (both entries).
int rows_args(const tpamd_rows_batch *bt, const tpamd_rows_inputs *in, const tpamd_path_outputs *out) {
  const int N = bt->num_samples, C = bt->num_rows;
  if (C < 1 || C > 64 || N < 3 || N > 8192) return TPAMD_E_UNSUPPORTED;
  if (!in->a || !in->b || !in->lower || !in->upper || !in->s_start || !in->s_end ||
      !in->sd_start || !in->time_start || !out->time || !out->s || !out->sd || !out->sdd ||
      !out->status)
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// The checks of a Cartesian batch after the null structs and B <= 0 (both entries).
int cartesian_args(const tpamd_cartesian_batch *bt, const tpamd_cartesian_inputs *in,
                   const tpamd_path_outputs *out) {
  const int D = bt->num_dofs, N = bt->num_samples;
  if (D < 1 || D > 16 || N < 3 || N > 8192) return TPAMD_E_UNSUPPORTED;
  if (!in->ik_positions || !in->jacobians || !in->max_velocity || !in->max_acceleration ||
      !in->max_translational_velocity || !in->max_rotational_velocity || !in->path_start ||
      !in->delta || !in->sd_start || !in->time_start || !out->time || !out->s || !out->sd ||
      !out->sdd || !out->status)
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// The Cartesian solve. The batch entry reads [B][N] rows of IK positions and Jacobians. The window
// loop of a Cartesian planner set (`plan`) reads, in place, N rows of each planner's IK table
// ([B][table_stride] rows) from row plan->first[b] on, and adds what solve_joint adds: skip marks
// after the set-up kernel, the start-velocity projection after K1 (q'(0) is the first record's
// finite-difference derivative); out->q is then a gather of the table segments. Planners that are
// not looping keep the outputs of the sweep (time, s, sd, sdd, status); on the generic route
// k_epilogue rewrites their qd / qdd from their last records, which nothing reads.
// A ragged batch entry (`ns` given, no plan) gives path b ns[b] samples in arrays of stride N and
// reads its rows from first_row[b] of the row tables on, or from [b][0] of a [B][N] batch without
// first_row; it takes the ragged forms of the set-up kernel and of K1 / k_cartesian_rows, orders
// the sweep longest path first as solve_joint does, and out->q is a gather. Everything behind
// those kernels reads the counts through ws.ns.
int solve_cartesian(tpamd_engine *e, const tpamd_cartesian_batch *bt, const tpamd_cartesian_inputs *in,
                    const tpamd_path_outputs *out, void *hip_stream, const PlanParams *plan, int table_stride,
                    const int32_t *ns = nullptr, const int32_t *first_row = nullptr) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  const int B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  if (B <= 0) return B == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = cartesian_args(bt, in, out)) return rc;
  const bool ragged = ns != nullptr;
  if (ragged && plan) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  const int C = 2 * D + 2;
  const int max_loops = bt->max_solver_loops > 0 ? bt->max_solver_loops : 0;
  const bool fused = (D == 6 || D == 7) && !e->force_generic;
  const int stride = plan ? table_stride : N;
  const int *first = plan ? plan->first : nullptr;
  const unsigned gb = (unsigned)((B + 127) / 128);
  PlanParams pp{};
  if (plan) {
    pp = *plan;
    pp.rec_stride = fused ? C + 2 : 2 * D + 2;
  }
  SlotGuard slot_guard(e, st);
  int rc = ensure_workspace(e, B, N, C);
  if (rc) return rc;
  e->last_B = B; e->last_N = N; e->last_time = out->time;
  e->ws.ns = ns;
  // ragged batches: sweep workgroups take the paths longest first (k_order_paths), as in solve_joint
  int32_t *order = const_cast<int32_t *>(e->ws.order);
  const bool ordered = ragged && B > 1 && e->order_ragged;
  if (!ordered) e->ws.order = nullptr;
  e->ws.amax = in->max_acceleration;
  {
    Timer t(e, st, KI_SETUP);
    if (ragged)
      hipLaunchKernelGGL(k_setup_cartesian_ragged, dim3((B + 127) / 128), dim3(128), 0, st, B, N, D,
                         bt->constraint_safety, in->max_velocity, in->max_acceleration,
                         in->max_translational_velocity, in->max_rotational_velocity,
                         in->path_start, in->delta, in->sd_start, in->sdd_start, in->time_start,
                         e->ws);
    else
      hipLaunchKernelGGL(k_setup_cartesian, dim3((B + 127) / 128), dim3(128), 0, st, B, N, D,
                         bt->constraint_safety, in->max_velocity, in->max_acceleration,
                         in->max_translational_velocity, in->max_rotational_velocity,
                         in->path_start, in->delta, in->sd_start, in->sdd_start, in->time_start,
                         e->ws);
    if (plan) hipLaunchKernelGGL(k_plan_mark_skipped, dim3(gb), dim3(128), 0, st, pp, e->ws);
    if (ordered) hipLaunchKernelGGL(k_order_paths, dim3(1), dim3(1024), 0, st, B, N, ns, order);
  }
  if (fused) {
    // rows never materialised: K1 writes records, the joint-structured kernels do the rest
    const Workspace &ws = e->ws;
    {
      Timer t(e, st, KI_SAMPLE_LP);
      // Ragged batches take 64-thread blocks: fewer threads idle behind a path's end (measured,
      // 1024 paths of 500..4000 samples, K1 alone: 0.24 / 0.36 / 0.34 ms at 64 / 128 / 256 threads;
      // profiles/cartesian_ragged_ab.md).
      const int tpb = ragged ? 64 : 256;
      const size_t lds = (2 * (size_t)C + (2 * (size_t)D + 2) * tpb) * 8;
      const dim3 grid((N + tpb - 1) / tpb, B);
      if (ragged && D == 6)
        hipLaunchKernelGGL((k_cartesian_lp<1, 6, true>), grid, dim3(tpb), lds, st, N, in->ik_positions,
                           in->jacobians, ws, 0, first_row);
      else if (ragged)
        hipLaunchKernelGGL((k_cartesian_lp<1, 7, true>), grid, dim3(tpb), lds, st, N, in->ik_positions,
                           in->jacobians, ws, 0, first_row);
      else if (D == 6)
        hipLaunchKernelGGL((k_cartesian_lp<1, 6>), grid, dim3(tpb), lds, st, N, in->ik_positions,
                           in->jacobians, ws, stride, first);
      else
        hipLaunchKernelGGL((k_cartesian_lp<1, 7>), grid, dim3(tpb), lds, st, N, in->ik_positions,
                           in->jacobians, ws, stride, first);
      if (plan) hipLaunchKernelGGL(k_plan_project, dim3(gb), dim3(128), 0, st, pp, ws);
    }
    JointSource src;
    src.q12 = ws.q12; src.lim = ws.lim; src.D = D; src.E = 2;
    e->ws.sd2_out = out->sd2;
    {
      Timer t(e, st, KI_SWEEP);
      if (D == 6) launch_sweep_cartesian<6>(st, B, N, max_loops, src, e->ws, out);
      else launch_sweep_cartesian<7>(st, B, N, max_loops, src, e->ws, out);
    }
  } else {
    const size_t nrow = align_up((size_t)B * N * C * 8, 256);
    if (4 * nrow > e->rows.bytes) e->rows_for_plan = false;
    if (e->rows.reserve(4 * nrow)) return TPAMD_E_HIP;
    // window chaining: planners that do not loop have no rows written, and the LP kernel still reads
    // theirs (its results for them are dropped). They read zeros or an earlier window's rows, never
    // what a new allocation or a batch solve left there.
    if (plan && !e->rows_for_plan) HIPCHK(hipMemsetAsync(e->rows.p, 0, 4 * nrow, st));
    e->rows_for_plan = plan != nullptr;
    const Workspace &ws = e->ws;
    double *A = (double *)e->rows.p, *Bm = (double *)((char *)e->rows.p + nrow),
           *LO = (double *)((char *)e->rows.p + 2 * nrow),
           *HI = (double *)((char *)e->rows.p + 3 * nrow);
    {
      Timer t(e, st, KI_SETUP);
      if (ragged)
        hipLaunchKernelGGL(k_cartesian_rows_ragged, dim3((N + 127) / 128, B), dim3(128), 0, st, N, D,
                           bt->constraint_safety, in->ik_positions, in->jacobians, in->max_velocity,
                           in->max_acceleration, in->max_translational_velocity,
                           in->max_rotational_velocity, A, Bm, LO, HI, ws, first_row);
      else
        hipLaunchKernelGGL(k_cartesian_rows, dim3((N + 127) / 128, B), dim3(128), 0, st, N, D,
                           bt->constraint_safety, in->ik_positions, in->jacobians, in->max_velocity,
                           in->max_acceleration, in->max_translational_velocity,
                           in->max_rotational_velocity, A, Bm, LO, HI, ws, stride, first);
      if (plan) hipLaunchKernelGGL(k_plan_project, dim3(gb), dim3(128), 0, st, pp, ws);
    }
    rc = run_rows(e, st, B, N, C, max_loops, A, Bm, LO, HI, out);
    if (rc) return rc;
    if (out->qd || out->qdd) {
      Timer t(e, st, KI_EPILOGUE);
      const size_t total = (size_t)B * N * D;
      hipLaunchKernelGGL(k_epilogue, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, B, N,
                         D, ws.q12, out->sd, out->sdd, in->max_acceleration, out->status, ws.ns,
                         out->qd, out->qdd);
    }
  }
  if (out->q) {
    if (plan)
      hipLaunchKernelGGL(k_gather_window_q, dim3((unsigned)((N * D + 255) / 256), (unsigned)B), dim3(256), 0, st, N,
                         D, in->ik_positions, stride, first, pp.active, out->q);
    else if (ragged)
      hipLaunchKernelGGL(k_gather_ragged_q, dim3((unsigned)((N * D + 255) / 256), (unsigned)B), dim3(256), 0, st, N,
                         D, in->ik_positions, ns, first_row, out->q);
    else
      HIPCHK(hipMemcpyAsync(out->q, in->ik_positions, (size_t)B * N * D * 8, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// The explicit-rows solve; `ns` (tpamd_optimize_rows_ragged_*) gives path b ns[b] samples in arrays
// of stride N: the ragged set-up kernel, then what a uniform batch runs (k_lp_rows and everything
// behind it read the counts through ws.ns), the sweep longest path first.
int solve_rows(tpamd_engine *e, const tpamd_rows_batch *bt, const tpamd_rows_inputs *in, const int32_t *ns,
               const tpamd_path_outputs *out, void *hip_stream) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  const int B = bt->num_paths, N = bt->num_samples, C = bt->num_rows;
  if (B <= 0) return B == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = rows_args(bt, in, out)) return rc;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  SlotGuard slot_guard(e, st);
  int rc = ensure_workspace(e, B, N, 1);
  if (rc) return rc;
  e->last_B = B; e->last_N = N; e->last_time = out->time;
  e->ws.ns = ns;
  int32_t *order = const_cast<int32_t *>(e->ws.order);
  const bool ordered = ns != nullptr && B > 1 && e->order_ragged;
  if (!ordered) e->ws.order = nullptr;
  const Workspace &ws = e->ws;
  const int max_loops = bt->max_solver_loops > 0 ? bt->max_solver_loops : 100;
  {
    Timer t(e, st, KI_SETUP);
    if (ns)
      hipLaunchKernelGGL(k_setup_rows_ragged, dim3((B + 127) / 128), dim3(128), 0, st, B, N, in->s_start,
                         in->s_end, in->sd_start, in->sdd_start, in->time_start, ws);
    else
      hipLaunchKernelGGL(k_setup_rows, dim3((B + 127) / 128), dim3(128), 0, st, B, N, in->s_start,
                         in->s_end, in->sd_start, in->sdd_start, in->time_start, ws);
    if (ordered) hipLaunchKernelGGL(k_order_paths, dim3(1), dim3(1024), 0, st, B, N, ns, order);
  }
  return run_rows(e, st, B, N, C, max_loops, in->a, in->b, in->lower, in->upper, out);
}
}  // namespace

extern "C" {

int tpamd_optimize_rows_device(tpamd_engine *e, const tpamd_rows_batch *bt,
                               const tpamd_rows_inputs *in, const tpamd_path_outputs *out,
                               void *hip_stream) {
  return solve_rows(e, bt, in, nullptr, out, hip_stream);
}

int tpamd_optimize_rows_ragged_device(tpamd_engine *e, const tpamd_rows_batch *bt, const tpamd_rows_inputs *in,
                                      const int32_t *num_samples_per_path, const tpamd_path_outputs *out,
                                      void *hip_stream) {
  if (!num_samples_per_path) return TPAMD_E_INVALID_ARGUMENT;
  return solve_rows(e, bt, in, num_samples_per_path, out, hip_stream);
}

int tpamd_time_cartesian_paths_ragged_device(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                             const tpamd_cartesian_inputs *in,
                                             const int32_t *num_samples_per_path, const int32_t *first_row,
                                             const tpamd_path_outputs *out, void *hip_stream) {
  if (!num_samples_per_path) return TPAMD_E_INVALID_ARGUMENT;
  return solve_cartesian(e, bt, in, out, hip_stream, nullptr, 0, num_samples_per_path, first_row);
}

int tpamd_time_cartesian_paths_device(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                      const tpamd_cartesian_inputs *in,
                                      const tpamd_path_outputs *out, void *hip_stream) {
  return solve_cartesian(e, bt, in, out, hip_stream, nullptr, 0);
}

int tpamd_time_cartesian_paths_host(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                    const tpamd_cartesian_inputs *in,
                                    const tpamd_path_outputs *out) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = cartesian_args(bt, in, out)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_cartesian_inputs din{};
  tpamd_path_outputs dout{}, staged = *out;
  staged.q = nullptr;   // q is the caller's ik_positions: copied on the host below
  HostStage s;
  s.up(&din.ik_positions, in->ik_positions, B * N * D);
  s.up(&din.jacobians, in->jacobians, B * N * 6 * D);
  s.up(&din.max_velocity, in->max_velocity, B * D);
  s.up(&din.max_acceleration, in->max_acceleration, B * D);
  s.up(&din.max_translational_velocity, in->max_translational_velocity, B);
  s.up(&din.max_rotational_velocity, in->max_rotational_velocity, B);
  s.up(&din.path_start, in->path_start, B);
  s.up(&din.delta, in->delta, B);
  s.up(&din.sd_start, in->sd_start, B);
  s.up_or_zero(&din.sdd_start, in->sdd_start, B);
  s.up(&din.time_start, in->time_start, B);
  stage_path_outputs(s, B, N, D, &staged, &dout);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_time_cartesian_paths_device(e, bt, &din, &dout, st);
  if (!rc) rc = s.download(st);
  if (rc) return rc;
  if (out->q && out->q != in->ik_positions) std::memcpy(out->q, in->ik_positions, B * N * D * 8);
  return 0;
}

int tpamd_time_cartesian_paths_ragged_host(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                           const tpamd_cartesian_inputs *in,
                                           const int32_t *num_samples_per_path, const int32_t *first_row,
                                           int64_t num_rows, const tpamd_path_outputs *out) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  if (!num_samples_per_path) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = cartesian_args(bt, in, out)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  if (first_row && (num_rows < 1 || num_rows >= ((int64_t)1 << 31))) return TPAMD_E_INVALID_ARGUMENT;
  const size_t rows = first_row ? (size_t)num_rows : B * N;
  // the rows of a path with a usable count must lie inside what is staged
  if (first_row)
    for (size_t b = 0; b < B; b++) {
      const int64_t n = num_samples_per_path[b];
      if (n < 2 || n > (int64_t)N) continue;
      if (first_row[b] < 0 || (int64_t)first_row[b] + n > num_rows) return TPAMD_E_INVALID_ARGUMENT;
    }
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_cartesian_inputs din{};
  tpamd_path_outputs dout{}, staged = *out;
  staged.q = nullptr;   // q is a gather of the caller's ik_positions: copied on the host below
  const int32_t *d_ns = nullptr, *d_first = nullptr;
  HostStage s;
  s.up(&din.ik_positions, in->ik_positions, rows * D);
  s.up(&din.jacobians, in->jacobians, rows * 6 * D);
  s.up(&din.max_velocity, in->max_velocity, B * D);
  s.up(&din.max_acceleration, in->max_acceleration, B * D);
  s.up(&din.max_translational_velocity, in->max_translational_velocity, B);
  s.up(&din.max_rotational_velocity, in->max_rotational_velocity, B);
  s.up(&din.path_start, in->path_start, B);
  s.up(&din.delta, in->delta, B);
  s.up(&din.sd_start, in->sd_start, B);
  s.up_or_zero(&din.sdd_start, in->sdd_start, B);
  s.up(&din.time_start, in->time_start, B);
  s.up(&d_ns, num_samples_per_path, B);
  s.up(&d_first, first_row, B);
  stage_path_outputs(s, B, N, D, &staged, &dout, /*keep=*/true);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_time_cartesian_paths_ragged_device(e, bt, &din, d_ns, d_first, &dout, st);
  if (!rc) rc = s.download(st);
  if (rc) return rc;
  if (out->q)
    for (size_t b = 0; b < B; b++) {
      const int64_t n = num_samples_per_path[b];
      if (n < 2 || n > (int64_t)N) continue;
      const size_t row0 = first_row ? (size_t)first_row[b] : b * N;
      std::memmove(out->q + b * N * D, in->ik_positions + row0 * D, (size_t)n * D * 8);
    }
  return 0;
}

// ---- host-buffer convenience paths ---------------------------------------

}  // extern "C"

namespace {
// One joint batch's host arrays in `s`.
void stage_joint(HostStage &s, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                 const tpamd_path_outputs *out, tpamd_joint_inputs *din, tpamd_path_outputs *dout) {
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples, P = bt->num_points;
  s.up(&din->knots, in->knots, B * (P + 3));
  s.up(&din->control_points, in->control_points, B * P * D);
  s.up(&din->max_velocity, in->max_velocity, B * D);
  s.up(&din->max_acceleration, in->max_acceleration, B * D);
  s.up(&din->path_start, in->path_start, B);
  s.up(&din->delta, in->delta, B);
  s.up(&din->sd_start, in->sd_start, B);
  s.up_or_zero(&din->sdd_start, in->sdd_start, B);
  s.up(&din->time_start, in->time_start, B);
  s.up(&din->num_samples_per_path, in->num_samples_per_path, B);
  stage_path_outputs(s, B, N, D, out, dout);
}

// The _host joint entries: sizes below 1 are invalid arguments, then the checks of solve_joint.
int joint_host_args(const tpamd_joint_batch *bt, const tpamd_joint_inputs *in, const tpamd_path_outputs *out) {
  if (bt->num_dofs < 1 || bt->num_samples < 1 || bt->num_points < 1) return TPAMD_E_INVALID_ARGUMENT;
  return joint_args(bt, in, out);
}

// Lane k of the engine: created on first use. Lane 0 gets the highest stream priority (it is
// given the group with the longest critical path, see tpamd_time_joint_groups_device).
int ensure_lane(tpamd_engine *e, int k) {
  tpamd_engine::Lane &ln = e->lanes[k];
  if (ln.stream) return 0;
  int least = 0, greatest = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&least, &greatest));
  HIPCHK(hipStreamCreateWithPriority(&ln.stream, hipStreamNonBlocking, k == 0 ? greatest : 0));
  HIPCHK(hipEventCreateWithFlags(&ln.done, hipEventDisableTiming));
  HIPCHK(hipEventCreateWithFlags(&ln.front, hipEventDisableTiming));
  if (!e->ev_fork) HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  return 0;
}

// Run `fn` with lane k's workspace in place of the engine's current one.
template <class F>
int with_lane_workspace(tpamd_engine *e, int k, F fn) {
  tpamd_engine::Lane &ln = e->lanes[k];
  std::swap(e->ws_buf, ln.ws);
  const Workspace saved = e->ws;
  e->in_lane = true;
  const int rc = fn(ln.stream);
  e->in_lane = false;
  e->ws = saved;
  std::swap(e->ws_buf, ln.ws);
  return rc;
}
}  // namespace

extern "C" {

int tpamd_time_joint_groups_device(tpamd_engine *e, int num_groups, const tpamd_joint_batch *batches,
                                   const tpamd_joint_inputs *inputs, const tpamd_path_outputs *outputs,
                                   void *hip_stream) {
  if (!e || num_groups < 0 || (num_groups > 0 && (!batches || !inputs || !outputs)))
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_groups == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t caller = (hipStream_t)hip_stream;
  // heaviest first: the group whose longest path has the longest sweep (about stride x joints)
  std::vector<int> idx(num_groups);
  for (int g = 0; g < num_groups; g++) idx[g] = g;
  std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
    return (long long)batches[a].num_samples * batches[a].num_dofs >
           (long long)batches[b].num_samples * batches[b].num_dofs;
  });
  if (num_groups == 1 || stream_is_capturing(caller)) {
    // nothing to overlap / a captured stream cannot fork into the engine's lanes: in order
    for (int g : idx) {
      const int rc = solve_joint(e, &batches[g], &inputs[g], &outputs[g], caller, nullptr, false);
      if (rc) return rc;
    }
    return 0;
  }
  const int nl = std::min(num_groups, tpamd_engine::kLanes);
  for (int k = 0; k < nl; k++) {
    const int rc = ensure_lane(e, k);
    if (rc) return rc;
  }
  // this call uses the lanes' workspaces only, but an unpipelined solve that is still running on
  // the caller's stream owns nothing of theirs: fork the lanes from the caller's position
  HIPCHK(hipEventRecord(e->ev_fork, caller));
  for (int k = 0; k < nl; k++) HIPCHK(hipStreamWaitEvent(e->lanes[k].stream, e->ev_fork, 0));
  // The sampling/LP kernels of the groups run one after another in weight order, each with the
  // whole machine to itself, so that the heaviest group's sweep -- whose longest path is the
  // call's critical path -- starts as early as it can; the sweeps then overlap each other and the
  // later groups' sampling/LP kernels (every later front stage waits for the heaviest group's).
  int rc_all = 0;
  hipEvent_t heaviest_front = nullptr;
  for (int n = 0; n < num_groups && rc_all == 0; n++) {
    const int g = idx[n];
    if (batches[g].num_paths <= 0) continue;
    const int k = n % nl;
    e->front_wait = heaviest_front;
    e->front_record = e->lanes[k].front;
    rc_all = with_lane_workspace(e, k, [&](hipStream_t st) {
      return solve_joint(e, &batches[g], &inputs[g], &outputs[g], st, nullptr, false);
    });
    if (heaviest_front == nullptr) heaviest_front = e->lanes[k].front;
  }
  e->front_wait = nullptr;
  e->front_record = nullptr;
  // join (also after an error: whatever was launched is ordered before the caller goes on)
  for (int k = 0; k < nl; k++) {
    HIPCHK(hipEventRecord(e->lanes[k].done, e->lanes[k].stream));
    HIPCHK(hipStreamWaitEvent(caller, e->lanes[k].done, 0));
  }
  e->last_B = 0; e->last_N = 0; e->last_time = nullptr;   // no single "last solve" to query
  return rc_all;
}

int tpamd_time_joint_groups_host(tpamd_engine *e, int num_groups, const tpamd_joint_batch *batches,
                                 const tpamd_joint_inputs *inputs, const tpamd_path_outputs *outputs) {
  if (!e || num_groups < 0 || (num_groups > 0 && (!batches || !inputs || !outputs)))
    return TPAMD_E_INVALID_ARGUMENT;
  std::vector<int> live;
  for (int g = 0; g < num_groups; g++) {
    if (batches[g].num_paths < 0) return TPAMD_E_INVALID_ARGUMENT;
    if (batches[g].num_paths == 0) continue;
    if (int rc = joint_host_args(&batches[g], &inputs[g], &outputs[g])) return rc;
    live.push_back(g);
  }
  if (live.empty()) return 0;
  TPAMD_ON_DEVICE(e);
  const size_t G = live.size();
  hipStream_t st = nullptr;
  std::vector<tpamd_joint_batch> bts(G);
  std::vector<tpamd_joint_inputs> dins(G);
  std::vector<tpamd_path_outputs> douts(G);
  HostStage s;
  for (size_t k = 0; k < G; k++) {
    bts[k] = batches[live[k]];
    stage_joint(s, &bts[k], &inputs[live[k]], &outputs[live[k]], &dins[k], &douts[k]);
  }
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_time_joint_groups_device(e, (int)G, bts.data(), dins.data(), douts.data(), st);
  return rc ? rc : s.download(st);
}

int tpamd_time_joint_paths_host(tpamd_engine *e, const tpamd_joint_batch *bt,
                                const tpamd_joint_inputs *in, const tpamd_path_outputs *out) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = joint_host_args(bt, in, out)) return rc;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_joint_inputs din{};
  tpamd_path_outputs dout{};
  HostStage s;
  stage_joint(s, bt, in, out, &din, &dout);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  // never pipelined: the inputs were just queued on this stream, the outputs are copied back
  // right behind the solve, and the staging buffer is reused by the next _host call
  rc = solve_joint(e, bt, &din, &dout, st, nullptr, /*allow_pipelining=*/false);
  return rc ? rc : s.download(st);
}

int tpamd_sample_joint_paths_host(tpamd_engine *e, int num_paths, int num_dofs, int num_samples,
                                  int num_points, const double *knots,
                                  const double *control_points, const double *path_start,
                                  const double *delta, double *q, double *q1, double *q2) {
  if (!e || !knots || !control_points || !path_start || !delta || !q || !q1 || !q2)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths <= 0) return num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (num_dofs < 1 || num_samples < 1 || num_points < 3) return TPAMD_E_UNSUPPORTED;
  const size_t B = num_paths, D = num_dofs, N = num_samples, P = num_points;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const double *d_knots, *d_cp, *d_ps, *d_dl;
  double *d_q, *d_q1, *d_q2;
  HostStage s;
  s.up(&d_knots, knots, B * (P + 3));
  s.up(&d_cp, control_points, B * P * D);
  s.up(&d_ps, path_start, B);
  s.up(&d_dl, delta, B);
  s.down(&d_q, q, B * N * D);
  s.down(&d_q1, q1, B * N * D);
  s.down(&d_q2, q2, B * N * D);
  if (int rc = s.upload(e->stage, st)) return rc;
  const size_t lds = (P + 3 + P * D) * 8;
  hipLaunchKernelGGL(k_sample_only, dim3((unsigned)((N + 255) / 256), (unsigned)B), dim3(256),
                     lds, st, (int)N, (int)D, (int)P, d_knots, d_cp, d_ps, d_dl, d_q, d_q1, d_q2);
  HIPCHK(hipGetLastError());
  return s.download(st);
}

}  // extern "C"

namespace {
// The sizes both pose-spline entries refuse (after their null and num_paths checks).
int pose_spline_sizes(int num_samples, int num_points) {
  if (num_samples < 1 || num_points < 3) return TPAMD_E_UNSUPPORTED;
  const size_t lds = ((size_t)(num_points + 3) + 7 * (size_t)num_points) * 8;
  return lds > 64 * 1024 ? TPAMD_E_UNSUPPORTED : 0;
}
}  // namespace

extern "C" {

int tpamd_sample_pose_splines_device(tpamd_engine *e, int num_paths, int num_samples, int num_points,
                                     const double *knots, const double *translation_points,
                                     const double *rotation_points, const double *path_start,
                                     const double *delta, double *poses, void *hip_stream) {
  if (!e || !knots || !translation_points || !rotation_points || !path_start || !delta || !poses)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths <= 0) return num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = pose_spline_sizes(num_samples, num_points)) return rc;
  const size_t lds = ((size_t)(num_points + 3) + 7 * (size_t)num_points) * 8;
  TPAMD_ON_DEVICE(e);
  hipLaunchKernelGGL(k_sample_pose_splines, dim3((num_samples + 255) / 256, num_paths), dim3(256), lds,
                     (hipStream_t)hip_stream, num_samples, num_points, knots, translation_points,
                     rotation_points, path_start, delta, poses);
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_sample_pose_splines_host(tpamd_engine *e, int num_paths, int num_samples, int num_points,
                                   const double *knots, const double *translation_points,
                                   const double *rotation_points, const double *path_start,
                                   const double *delta, double *poses) {
  if (!e || !knots || !translation_points || !rotation_points || !path_start || !delta || !poses)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths <= 0) return num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = pose_spline_sizes(num_samples, num_points)) return rc;
  const size_t B = num_paths, N = num_samples, P = num_points;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const double *d_k, *d_t, *d_r, *d_ps, *d_dl;
  double *d_out;
  HostStage s;
  s.up(&d_k, knots, B * (P + 3));
  s.up(&d_t, translation_points, B * P * 3);
  s.up(&d_r, rotation_points, B * P * 4);
  s.up(&d_ps, path_start, B);
  s.up(&d_dl, delta, B);
  s.down(&d_out, poses, B * N * 7);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_sample_pose_splines_device(e, num_paths, num_samples, num_points, d_k, d_t, d_r, d_ps, d_dl, d_out, st);
  return rc ? rc : s.download(st);
}

}  // extern "C"

// ------------------------------------------------------- Cartesian goals: pose fit and IK targets
namespace {

constexpr int kMaxPosePaths = 65535;      // the target kernel's grid has one row of blocks per path

// The packing of a ragged batch of fitted paths: path k's control points start at point[k], its knots
// at knot[k] = point[k] + 3 (paths with points before k). A path without points takes no slots.
struct PosePacking {
  std::vector<int32_t> point, knot;       // [n + 1]
  bool build(int n, const int32_t *num_points) {
    point.assign((size_t)n + 1, 0);
    knot.assign((size_t)n + 1, 0);
    long long pts = 0, kn = 0;
    for (int k = 0; k < n; k++) {
      pts += num_points[k];
      kn += num_points[k] > 0 ? num_points[k] + 3 : 0;
      if (kn * 16 > INT32_MAX) return false;      // [points][D <= 16] stays below 2^31 elements
      point[k + 1] = (int32_t)pts;
      knot[k + 1] = (int32_t)kn;
    }
    return true;
  }
  size_t points() const { return (size_t)point.back(); }
  size_t knots() const { return (size_t)knot.back(); }
};

// The call-level checks of the two fit entries; fills the control-point count of every path.
int pose_fit_args(const tpamd_engine *e, int num_paths, int num_dofs, const int32_t *offsets, const double *pose_wps,
                  const double *joint_wps, const double *tround, const double *rround, const double *knots,
                  const double *trans, const double *rot, const double *jcp, const int32_t *num_points,
                  const double *path_end, const int32_t *status, std::vector<int32_t> *np, PosePacking *pk) {
  if (!e || num_paths < 0 || !offsets || !tround || !rround || !num_points || !path_end || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_dofs < 1 || num_dofs > 16 || offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths > kMaxPosePaths) return TPAMD_E_UNSUPPORTED;
  np->resize(num_paths);
  for (int k = 0; k < num_paths; k++) {
    if (offsets[k + 1] < offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
    const long long W = (long long)offsets[k + 1] - offsets[k];
    if (W > (1 << 24)) return TPAMD_E_UNSUPPORTED;
    (*np)[k] = W < 1 ? 0 : fit_points((int)W);
  }
  if (!pk->build(num_paths, np->data())) return TPAMD_E_UNSUPPORTED;
  if (num_paths && offsets[num_paths] > 0 && (!pose_wps || !joint_wps || !knots || !trans || !rot || !jcp))
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// The call-level checks of the two target entries (delta is checked by the host entry itself).
int ik_target_args(const tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                   const int32_t *row_offsets, const double *knots, const double *trans, const double *rot,
                   const double *jcp, const double *delta, const double *pose_targets, const double *joint_targets,
                   PosePacking *pk, int *max_rows) {
  if (!e || num_paths < 0 || !num_points || !row_offsets || !knots || !trans || !rot || !jcp || !delta ||
      !pose_targets || !joint_targets)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_dofs < 1 || num_dofs > 16 || row_offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths > kMaxPosePaths) return TPAMD_E_UNSUPPORTED;
  int most = 0;
  for (int k = 0; k < num_paths; k++) {
    if (num_points[k] < 3 || row_offsets[k + 1] < row_offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
    most = std::max(most, row_offsets[k + 1] - row_offsets[k]);
  }
  if (!pk->build(num_paths, num_points)) return TPAMD_E_UNSUPPORTED;
  *max_rows = most;
  return 0;
}

// The int arrays of a _device call go up on `st` into the engine's pose_ints (from pageable memory:
// the copy has left `ints` when the call returns). The previous call's kernel may still read the
// buffer on another stream: `st` waits for it; if the buffer has to grow, the host does.
int stage_pose_ints(tpamd_engine *e, const std::vector<int32_t> &ints, hipStream_t st, const int32_t **dev) {
  const size_t bytes = ints.size() * sizeof(int32_t);
  if (!e->ev_pose) HIPCHK(hipEventCreateWithFlags(&e->ev_pose, hipEventDisableTiming));
  if (e->pose_busy) {
    if (bytes > e->pose_ints.bytes) {
      HIPCHK(hipEventSynchronize(e->ev_pose));
      e->pose_busy = false;
    } else {
      HIPCHK(hipStreamWaitEvent(st, e->ev_pose, 0));
    }
  }
  if (e->pose_ints.reserve(std::max(bytes, (size_t)4096))) return TPAMD_E_HIP;
  HIPCHK(hipMemcpyAsync(e->pose_ints.p, ints.data(), bytes, hipMemcpyHostToDevice, st));
  *dev = (const int32_t *)e->pose_ints.p;
  return 0;
}
int pose_ints_done(tpamd_engine *e, hipStream_t st) {
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(e->ev_pose, st));
  e->pose_busy = true;
  return 0;
}

}  // namespace

extern "C" {

int tpamd_ik_table_rows(double path_end, double delta, int num_samples) {
  if (!(delta > 0.0) || num_samples < 1) return -1;
  return (int)std::round(path_end / delta) + num_samples + 1;     // PathIkIndex(knots.back()) + N + 1
}

int tpamd_fit_pose_waypoints_device(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *waypoint_offsets,
                                    const double *pose_waypoints, const double *joint_waypoints,
                                    const double *translation_rounding, const double *rotation_rounding,
                                    double *knots, double *translation_points, double *rotation_points,
                                    double *joint_control_points, int32_t *num_points, int32_t *point_offsets,
                                    double *path_end, int32_t *status, void *hip_stream) {
  std::vector<int32_t> np;
  PosePacking pk;
  if (int rc = pose_fit_args(e, num_paths, num_dofs, waypoint_offsets, pose_waypoints, joint_waypoints,
                             translation_rounding, rotation_rounding, knots, translation_points, rotation_points,
                             joint_control_points, num_points, path_end, status, &np, &pk))
    return rc;
  const size_t n = (size_t)num_paths;
  if (point_offsets) std::memcpy(point_offsets, pk.point.data(), (n + 1) * sizeof(int32_t));
  if (num_paths == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> ints(waypoint_offsets, waypoint_offsets + n + 1);
  ints.insert(ints.end(), pk.point.begin(), pk.point.end());
  ints.insert(ints.end(), pk.knot.begin(), pk.knot.end());
  const int32_t *d = nullptr;
  if (int rc = stage_pose_ints(e, ints, st, &d)) return rc;
  PoseFitParams p{};
  p.Q = num_paths; p.D = num_dofs;
  p.offsets = d; p.point_offsets = d + (n + 1); p.knot_offsets = d + 2 * (n + 1);
  p.pose_wps = pose_waypoints; p.joint_wps = joint_waypoints;
  p.translation_rounding = translation_rounding; p.rotation_rounding = rotation_rounding;
  p.knots = knots; p.trans = translation_points; p.rot = rotation_points; p.joint_cp = joint_control_points;
  p.num_points = num_points; p.path_end = path_end; p.status = status;
  launch_fit_pose_waypoints(p, st);
  return pose_ints_done(e, st);
}

int tpamd_fit_pose_waypoints_host(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *waypoint_offsets,
                                  const double *pose_waypoints, const double *joint_waypoints,
                                  const double *translation_rounding, const double *rotation_rounding,
                                  double *knots, double *translation_points, double *rotation_points,
                                  double *joint_control_points, int32_t *num_points, int32_t *point_offsets,
                                  double *path_end, int32_t *status) {
  std::vector<int32_t> np;
  PosePacking pk;
  if (int rc = pose_fit_args(e, num_paths, num_dofs, waypoint_offsets, pose_waypoints, joint_waypoints,
                             translation_rounding, rotation_rounding, knots, translation_points, rotation_points,
                             joint_control_points, num_points, path_end, status, &np, &pk))
    return rc;
  const size_t n = (size_t)num_paths, D = (size_t)num_dofs;
  if (num_paths == 0) {
    if (point_offsets) point_offsets[0] = 0;
    return 0;
  }
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const size_t rows = (size_t)waypoint_offsets[n], P = pk.points();
  const double *d_pw, *d_jw, *d_tr, *d_rr;
  double *d_k, *d_t, *d_r, *d_j, *d_pe;
  int32_t *d_np, *d_st;
  HostStage s;
  s.up(&d_pw, pose_waypoints, rows * 7);
  s.up(&d_jw, joint_waypoints, rows * D);
  s.up(&d_tr, translation_rounding, n);
  s.up(&d_rr, rotation_rounding, n);
  s.down(&d_k, knots, pk.knots());
  s.down(&d_t, translation_points, P * 3);
  s.down(&d_r, rotation_points, P * 4);
  s.down(&d_j, joint_control_points, P * D);
  s.down(&d_np, num_points, n);
  s.down(&d_pe, path_end, n);
  s.down(&d_st, status, n);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = tpamd_fit_pose_waypoints_device(e, num_paths, num_dofs, waypoint_offsets, d_pw, d_jw, d_tr, d_rr, d_k, d_t,
                                           d_r, d_j, d_np, point_offsets, d_pe, d_st, st);
  return rc ? rc : s.download(st);
}

// first_row (host, may be null: 0): path k's rows are first_row[k] .. first_row[k] + n_k - 1 of its table
static int sample_ik_targets_device(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                    const int32_t *row_offsets, const int32_t *first_row, const double *knots,
                                    const double *translation_points, const double *rotation_points,
                                    const double *joint_control_points, const double *delta, double *pose_targets,
                                    double *joint_targets, void *hip_stream) {
  PosePacking pk;
  int max_rows = 0;
  if (int rc = ik_target_args(e, num_paths, num_dofs, num_points, row_offsets, knots, translation_points,
                              rotation_points, joint_control_points, delta, pose_targets, joint_targets, &pk,
                              &max_rows))
    return rc;
  if (first_row)
    for (int k = 0; k < num_paths; k++)
      if (first_row[k] < 0 || (long long)first_row[k] + (row_offsets[k + 1] - row_offsets[k]) > (1LL << 30))
        return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths == 0 || max_rows == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = (size_t)num_paths;
  std::vector<int32_t> ints(num_points, num_points + n);
  ints.push_back(0);
  ints.insert(ints.end(), pk.point.begin(), pk.point.end());
  ints.insert(ints.end(), pk.knot.begin(), pk.knot.end());
  ints.insert(ints.end(), row_offsets, row_offsets + n + 1);
  if (first_row) ints.insert(ints.end(), first_row, first_row + n);
  const int32_t *d = nullptr;
  if (int rc = stage_pose_ints(e, ints, st, &d)) return rc;
  IkTargetParams p{};
  p.Q = num_paths; p.D = num_dofs;
  p.num_points = d; p.point_offsets = d + (n + 1); p.knot_offsets = d + 2 * (n + 1); p.row_offsets = d + 3 * (n + 1);
  p.first_row = first_row ? d + 4 * (n + 1) : nullptr;
  p.knots = knots; p.trans = translation_points; p.rot = rotation_points; p.joint_cp = joint_control_points;
  p.delta = delta; p.pose_targets = pose_targets; p.joint_targets = joint_targets;
  launch_sample_ik_targets(p, max_rows, st);
  return pose_ints_done(e, st);
}

int tpamd_sample_ik_targets_device(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                   const int32_t *row_offsets, const double *knots,
                                   const double *translation_points, const double *rotation_points,
                                   const double *joint_control_points, const double *delta, double *pose_targets,
                                   double *joint_targets, void *hip_stream) {
  return sample_ik_targets_device(e, num_paths, num_dofs, num_points, row_offsets, nullptr, knots, translation_points,
                                  rotation_points, joint_control_points, delta, pose_targets, joint_targets, hip_stream);
}

int tpamd_sample_ik_target_rows_device(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                       const int32_t *row_offsets, const int32_t *first_row, const double *knots,
                                       const double *translation_points, const double *rotation_points,
                                       const double *joint_control_points, const double *delta, double *pose_targets,
                                       double *joint_targets, void *hip_stream) {
  if (!first_row) return TPAMD_E_INVALID_ARGUMENT;
  return sample_ik_targets_device(e, num_paths, num_dofs, num_points, row_offsets, first_row, knots, translation_points,
                                  rotation_points, joint_control_points, delta, pose_targets, joint_targets, hip_stream);
}

static int sample_ik_targets_host(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                  const int32_t *row_offsets, const int32_t *first_row, const double *knots,
                                  const double *translation_points, const double *rotation_points,
                                  const double *joint_control_points, const double *delta, double *pose_targets,
                                  double *joint_targets) {
  PosePacking pk;
  int max_rows = 0;
  if (int rc = ik_target_args(e, num_paths, num_dofs, num_points, row_offsets, knots, translation_points,
                              rotation_points, joint_control_points, delta, pose_targets, joint_targets, &pk,
                              &max_rows))
    return rc;
  for (int k = 0; k < num_paths; k++)
    if (!(delta[k] > 0.0)) return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths == 0 || max_rows == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)num_paths, D = (size_t)num_dofs, P = pk.points(), rows = (size_t)row_offsets[n];
  const double *d_k, *d_t, *d_r, *d_j, *d_dl;
  double *d_pose, *d_joint;
  HostStage s;
  s.up(&d_k, knots, pk.knots());
  s.up(&d_t, translation_points, P * 3);
  s.up(&d_r, rotation_points, P * 4);
  s.up(&d_j, joint_control_points, P * D);
  s.up(&d_dl, delta, n);
  s.down(&d_pose, pose_targets, rows * 7);
  s.down(&d_joint, joint_targets, rows * D);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = sample_ik_targets_device(e, num_paths, num_dofs, num_points, row_offsets, first_row, d_k, d_t, d_r, d_j,
                                    d_dl, d_pose, d_joint, st);
  return rc ? rc : s.download(st);
}

int tpamd_sample_ik_targets_host(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                 const int32_t *row_offsets, const double *knots, const double *translation_points,
                                 const double *rotation_points, const double *joint_control_points,
                                 const double *delta, double *pose_targets, double *joint_targets) {
  return sample_ik_targets_host(e, num_paths, num_dofs, num_points, row_offsets, nullptr, knots, translation_points,
                                rotation_points, joint_control_points, delta, pose_targets, joint_targets);
}

int tpamd_sample_ik_target_rows_host(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *num_points,
                                     const int32_t *row_offsets, const int32_t *first_row, const double *knots,
                                     const double *translation_points, const double *rotation_points,
                                     const double *joint_control_points, const double *delta, double *pose_targets,
                                     double *joint_targets) {
  if (!first_row) return TPAMD_E_INVALID_ARGUMENT;
  return sample_ik_targets_host(e, num_paths, num_dofs, num_points, row_offsets, first_row, knots, translation_points,
                                rotation_points, joint_control_points, delta, pose_targets, joint_targets);
}

int tpamd_optimize_rows_host(tpamd_engine *e, const tpamd_rows_batch *bt,
                             const tpamd_rows_inputs *in, const tpamd_path_outputs *out) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = rows_args(bt, in, out)) return rc;
  const size_t B = bt->num_paths, N = bt->num_samples, C = bt->num_rows;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_rows_inputs din{};
  tpamd_path_outputs dout{}, staged = *out;
  staged.q = staged.qd = staged.qdd = nullptr;   // a rows solve has no joint values
  HostStage s;
  s.up(&din.a, in->a, B * N * C);
  s.up(&din.b, in->b, B * N * C);
  s.up(&din.lower, in->lower, B * N * C);
  s.up(&din.upper, in->upper, B * N * C);
  s.up(&din.s_start, in->s_start, B);
  s.up(&din.s_end, in->s_end, B);
  s.up(&din.sd_start, in->sd_start, B);
  s.up_or_zero(&din.sdd_start, in->sdd_start, B);
  s.up(&din.time_start, in->time_start, B);
  stage_path_outputs(s, B, N, 0, &staged, &dout);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_optimize_rows_device(e, bt, &din, &dout, st);
  return rc ? rc : s.download(st);
}

int tpamd_optimize_rows_ragged_host(tpamd_engine *e, const tpamd_rows_batch *bt, const tpamd_rows_inputs *in,
                                    const int32_t *num_samples_per_path, const tpamd_path_outputs *out) {
  if (!e || !bt || !in || !out) return TPAMD_E_INVALID_ARGUMENT;
  if (!num_samples_per_path) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = rows_args(bt, in, out)) return rc;
  const size_t B = bt->num_paths, N = bt->num_samples, C = bt->num_rows;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_rows_inputs din{};
  tpamd_path_outputs dout{}, staged = *out;
  staged.q = staged.qd = staged.qdd = nullptr;   // a rows solve has no joint values
  const int32_t *d_ns = nullptr;
  HostStage s;
  s.up(&din.a, in->a, B * N * C);
  s.up(&din.b, in->b, B * N * C);
  s.up(&din.lower, in->lower, B * N * C);
  s.up(&din.upper, in->upper, B * N * C);
  s.up(&din.s_start, in->s_start, B);
  s.up(&din.s_end, in->s_end, B);
  s.up(&din.sd_start, in->sd_start, B);
  s.up_or_zero(&din.sdd_start, in->sdd_start, B);
  s.up(&din.time_start, in->time_start, B);
  s.up(&d_ns, num_samples_per_path, B);
  stage_path_outputs(s, B, N, 0, &staged, &dout, /*keep=*/true);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_optimize_rows_ragged_device(e, bt, &din, d_ns, &dout, st);
  return rc ? rc : s.download(st);
}

int tpamd_find_max_sd2_host(tpamd_engine *e, int num, int C, const double *a, const double *b,
                            const double *lower, const double *upper, double *sd2max,
                            double *sddmax, double *sd2zero) {
  if (!e || num < 0 || !a || !b || !lower || !upper || !sd2max || !sddmax || !sd2zero)
    return TPAMD_E_INVALID_ARGUMENT;
  if (num == 0) return 0;
  if (C < 1 || C > 64) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(e);
  const size_t n = (size_t)num, nc = n * C;
  hipStream_t st = nullptr;
  const double *d_a, *d_b, *d_lo, *d_hi;
  double *d_o0, *d_o1, *d_o2;
  HostStage s;
  s.up(&d_a, a, nc);
  s.up(&d_b, b, nc);
  s.up(&d_lo, lower, nc);
  s.up(&d_hi, upper, nc);
  s.down(&d_o0, sd2max, n);
  s.down(&d_o1, sddmax, n);
  s.down(&d_o2, sd2zero, n);
  if (int rc = s.upload(e->stage, st)) return rc;
  const dim3 grid((num + 63) / 64);
  if (C <= 32)
    hipLaunchKernelGGL((k_lp_only<1>), grid, dim3(64), 0, st, num, C, d_a, d_b, d_lo, d_hi, d_o0,
                       d_o1, d_o2);
  else
    hipLaunchKernelGGL((k_lp_only<2>), grid, dim3(64), 0, st, num, C, d_a, d_b, d_lo, d_hi, d_o0,
                       d_o1, d_o2);
  HIPCHK(hipGetLastError());
  return s.download(st);
}

int tpamd_rebuild_time_device(tpamd_engine *e, int num_shards, int paths_per_shard, int N,
                              size_t shard_stride, const double *sd, const double *ds,
                              const double *time_start, const int32_t *ns, double *time_out,
                              void *hip_stream) {
  if (!e || !sd || !ds || !time_start || !time_out) return TPAMD_E_INVALID_ARGUMENT;
  if (num_shards < 0 || paths_per_shard < 0 || N < 2) return TPAMD_E_INVALID_ARGUMENT;
  const long long total = (long long)num_shards * paths_per_shard;
  if (total == 0) return 0;
  if (total > 0x7fffffffLL) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(e);
  hipLaunchKernelGGL(k_rebuild_time, dim3((unsigned)total), dim3(64), 0, (hipStream_t)hip_stream, N,
                     paths_per_shard, shard_stride, sd, ds, time_start, ns, time_out);
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_query_device(tpamd_engine *e, int B, int N, int K, const double *time, const double *s,
                       const double *sd, const double *sd2, const int32_t *status,
                       const double *t_query, double *os, double *osd, double *osdd, int32_t *ok,
                       void *hip_stream) {
  if (!e || !time || !s || !sd || !t_query || !os || !osd || !osdd) return TPAMD_E_INVALID_ARGUMENT;
  if (B < 0 || K < 0 || N < 2) return TPAMD_E_INVALID_ARGUMENT;
  if (!sd2) {
    // fall back to the copy of sd2_ the engine keeps from its last solve -- only if that is
    // the solve these rows came from
    if (B != e->last_B || N != e->last_N || time != e->last_time) return TPAMD_E_STALE;
    sd2 = e->ws.sd2;
  }
  if (B == 0 || K == 0) return 0;
  TPAMD_ON_DEVICE(e);
  // the engine's copy of sd2_ sits in the current workspace slot: its sweep may be running on an
  // engine stream (mode 2), and the slot's next front stage must not overwrite it under this kernel
  SlotGuard slot_guard(e, (hipStream_t)hip_stream, /*record_after=*/true, /*enable=*/sd2 == e->ws.sd2);
  const size_t total = (size_t)B * K;
  hipLaunchKernelGGL(k_query, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)hip_stream, B, N, K, time, s, sd, sd2, status, t_query, os,
                     osd, osdd, ok);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"

// ------------------------------------------------------- waypoint batches: fit and timing in one call
namespace {

// The call-level checks on the waypoint rows of a batch; fills the control-point count of every path.
int waypoint_rows_args(int num_paths, const int32_t *offsets, std::vector<int32_t> *np) {
  if (num_paths < 0 || !offsets || offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  if (num_paths > kMaxPosePaths) return TPAMD_E_UNSUPPORTED;
  np->resize(num_paths);
  for (int k = 0; k < num_paths; k++) {
    if (offsets[k + 1] < offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
    const long long W = (long long)offsets[k + 1] - offsets[k];
    if (W > (1 << 24)) return TPAMD_E_UNSUPPORTED;
    (*np)[k] = W < 1 ? 0 : fit_points((int)W);
  }
  return 0;
}

int joint_fit_args(const tpamd_engine *e, int num_paths, int num_dofs, const int32_t *offsets, const double *wps,
                   const double *knots, const double *cps, const int32_t *num_points, const double *path_end,
                   const int32_t *status, std::vector<int32_t> *np, PosePacking *pk) {
  if (!e || !num_points || !path_end || !status || num_dofs < 1 || num_dofs > 16) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = waypoint_rows_args(num_paths, offsets, np)) return rc;
  if (!pk->build(num_paths, np->data())) return TPAMD_E_UNSUPPORTED;
  if (num_paths && offsets[num_paths] > 0 && (!wps || !knots || !cps)) return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// The engine's scratch of a waypoint batch: B slots of S control points, and what the fit knows per path.
struct WaypointScratch {
  double *knots, *cps, *path_end, *delta, *zero;
  int32_t *np, *ns;
};
size_t carve_waypoint_scratch(char *base, size_t B, size_t S, size_t D, WaypointScratch *w) {
  Stage s(base);
  w->knots = s.take<double>(B * (S + 3));
  w->cps = s.take<double>(B * S * D);
  w->path_end = s.take<double>(B);
  w->delta = s.take<double>(B);
  w->zero = s.take<double>(B);
  w->np = s.take<int32_t>(B);
  w->ns = s.take<int32_t>(B);
  return s.off;
}

// What both timing entries check before anything is written; *slot = the largest control-point count
// (at least 4: the slot size of the scratch and of the optional spline outputs).
int waypoint_timing_args(const tpamd_engine *e, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                         const tpamd_path_outputs *out, std::vector<int32_t> *np, int *slot, bool *any_empty) {
  if (!e || !bt || !in || !out || bt->num_paths < 0) return TPAMD_E_INVALID_ARGUMENT;
  const int B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  if (D < 1 || D > 16 || N < 3 || N > 8192) return TPAMD_E_UNSUPPORTED;
  if (!in->waypoint_offsets || !in->max_velocity || !in->max_acceleration || !out->time || !out->s || !out->sd ||
      !out->sdd || !out->status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = waypoint_rows_args(B, in->waypoint_offsets, np)) return rc;
  if (B && in->waypoint_offsets[B] > 0 && !in->waypoints) return TPAMD_E_INVALID_ARGUMENT;
  int S = 4;
  bool empty = false;
  for (int k = 0; k < B; k++) {
    S = std::max(S, (*np)[k]);
    empty = empty || (*np)[k] == 0;
  }
  // the sampling/LP kernel stages a path's knots and control points in LDS: sized by the largest P
  const bool ragged = in->num_samples_per_path != nullptr || empty;
  if (sample_lp_lds(S, D, sample_lp_block(false, ragged, D)) > kSampleLpLdsLimit) return TPAMD_E_UNSUPPORTED;
  *slot = S;
  *any_empty = empty;
  return 0;
}

// What a waypoint solve leaves on the device for the call that goes on with it (the refined entry):
// the batch as the joint form describes it, in the engine's scratch.
struct WaypointSolved {
  tpamd_joint_batch jb;           // num_points = S, the slot size
  tpamd_joint_inputs ji;          // knots [B][S + 3], control points [B][S][D]; num_samples_per_path null: uniform
  const int32_t *np;              // [B] control points of each path
};
// The host arrays of a waypoint batch in `s` (both _host timing entries). S: the slot size of the fit
// outputs. A path without waypoints, and a path's rows behind its own sample count, keep what the
// caller's arrays hold: those go up as well then.
void stage_waypoint(HostStage &s, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                    const tpamd_path_outputs *out, const tpamd_waypoint_fit_outputs *fit, size_t S, bool any_empty,
                    tpamd_waypoint_inputs *din, tpamd_path_outputs *dout, tpamd_waypoint_fit_outputs *dfit) {
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  din->waypoint_offsets = in->waypoint_offsets;
  s.up(&din->waypoints, in->waypoints, (size_t)in->waypoint_offsets[B] * D);
  s.up(&din->rounding, in->rounding, B);
  s.up(&din->max_velocity, in->max_velocity, B * D);
  s.up(&din->max_acceleration, in->max_acceleration, B * D);
  s.up(&din->num_samples_per_path, in->num_samples_per_path, B);
  s.up(&din->delta, in->delta, B);
  s.up(&din->sd_start, in->sd_start, B);
  s.up(&din->time_start, in->time_start, B);
  stage_path_outputs(s, B, N, D, out, dout, /*keep=*/any_empty || in->num_samples_per_path != nullptr);
  if (fit) {
    s.down(&dfit->num_points, fit->num_points, B);
    s.down(&dfit->path_end, fit->path_end, B);
    s.down(&dfit->delta_used, fit->delta_used, B);
    s.down(&dfit->knots, fit->knots, B * (S + 3));
    s.down(&dfit->control_points, fit->control_points, B * S * D);
  }
}
// Behind the upload: the two per-path outputs that are staged either way keep the caller's values for a
// path without waypoints.
int upload_kept_path_outputs(size_t B, bool any_empty, const tpamd_path_outputs *out, const tpamd_path_outputs *dout,
                             hipStream_t st) {
  if (!any_empty) return 0;
  if (out->last_extremal_index)
    HIPCHK(hipMemcpyAsync(dout->last_extremal_index, out->last_extremal_index, B * 4, hipMemcpyHostToDevice, st));
  if (out->max_time_increment)
    HIPCHK(hipMemcpyAsync(dout->max_time_increment, out->max_time_increment, B * 8, hipMemcpyHostToDevice, st));
  return 0;
}
}  // namespace

extern "C" {

int tpamd_fit_joint_waypoints_device(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *waypoint_offsets,
                                     const double *waypoints, const double *rounding, double *knots,
                                     double *control_points, int32_t *num_points, int32_t *point_offsets,
                                     double *path_end, int32_t *status, void *hip_stream) {
  std::vector<int32_t> np;
  PosePacking pk;
  if (int rc = joint_fit_args(e, num_paths, num_dofs, waypoint_offsets, waypoints, knots, control_points, num_points,
                              path_end, status, &np, &pk))
    return rc;
  const size_t n = (size_t)num_paths;
  if (point_offsets) std::memcpy(point_offsets, pk.point.data(), (n + 1) * sizeof(int32_t));
  if (num_paths == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  std::vector<int32_t> ints(waypoint_offsets, waypoint_offsets + n + 1);
  ints.insert(ints.end(), pk.point.begin(), pk.point.end());
  ints.insert(ints.end(), pk.knot.begin(), pk.knot.end());
  const int32_t *d = nullptr;
  if (int rc = stage_pose_ints(e, ints, st, &d)) return rc;
  JointFitParams p{};
  p.Q = num_paths; p.D = num_dofs;
  p.offsets = d; p.point_offsets = d + (n + 1); p.knot_offsets = d + 2 * (n + 1);
  p.wps = waypoints; p.rounding = rounding;
  p.knots = knots; p.cps = control_points;
  p.num_points = num_points; p.path_end = path_end;
  p.status = status; p.status_empty = TPAMD_PLAN_INVALID_ARGUMENT; p.status_all = 1;
  launch_fit_joint_waypoints(p, st);
  return pose_ints_done(e, st);
}

int tpamd_fit_joint_waypoints_host(tpamd_engine *e, int num_paths, int num_dofs, const int32_t *waypoint_offsets,
                                   const double *waypoints, const double *rounding, double *knots,
                                   double *control_points, int32_t *num_points, int32_t *point_offsets,
                                   double *path_end, int32_t *status) {
  std::vector<int32_t> np;
  PosePacking pk;
  if (int rc = joint_fit_args(e, num_paths, num_dofs, waypoint_offsets, waypoints, knots, control_points, num_points,
                              path_end, status, &np, &pk))
    return rc;
  const size_t n = (size_t)num_paths, D = (size_t)num_dofs;
  if (num_paths == 0) {
    if (point_offsets) point_offsets[0] = 0;
    return 0;
  }
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const double *d_w, *d_r;
  double *d_k, *d_c, *d_pe;
  int32_t *d_np, *d_st;
  HostStage s;
  s.up(&d_w, waypoints, (size_t)waypoint_offsets[n] * D);
  s.up(&d_r, rounding, n);
  s.down(&d_k, knots, pk.knots());
  s.down(&d_c, control_points, pk.points() * D);
  s.down(&d_np, num_points, n);
  s.down(&d_pe, path_end, n);
  s.down(&d_st, status, n);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = tpamd_fit_joint_waypoints_device(e, num_paths, num_dofs, waypoint_offsets, d_w, d_r, d_k, d_c, d_np,
                                            point_offsets, d_pe, d_st, st);
  return rc ? rc : s.download(st);
}

// tpamd_time_waypoint_paths_device; `solved` (may be null) receives where the batch lies afterwards.
static int waypoint_solve(tpamd_engine *e, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                          const tpamd_path_outputs *out, const tpamd_waypoint_fit_outputs *fit, void *hip_stream,
                          WaypointSolved *solved) {
  std::vector<int32_t> np;
  int S = 0;
  bool any_empty = false;
  if (int rc = waypoint_timing_args(e, bt, in, out, &np, &S, &any_empty)) return rc;
  const int B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  if (B == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  // the scratch: an earlier call's kernels may still read it (on any stream) when it has to move
  WaypointScratch w{};
  const size_t need = carve_waypoint_scratch(nullptr, B, S, D, &w);
  if (need > e->wp_fit.bytes) {
    HIPCHK(hipDeviceSynchronize());
    if (e->wp_fit.reserve(need)) return TPAMD_E_HIP;
  }
  carve_waypoint_scratch((char *)e->wp_fit.p, B, S, D, &w);
  const std::vector<int32_t> ints(in->waypoint_offsets, in->waypoint_offsets + B + 1);
  const int32_t *d_off = nullptr;
  if (int rc = stage_pose_ints(e, ints, st, &d_off)) return rc;
  // a path without waypoints leaves the solve through its sample count (0), so such a batch is ragged
  const bool ragged = in->num_samples_per_path != nullptr || any_empty;
  JointFitParams p{};
  p.Q = B; p.D = D;
  p.offsets = d_off; p.wps = in->waypoints; p.rounding = in->rounding;
  p.p_stride = S; p.knots = w.knots; p.cps = w.cps;
  p.num_points = (fit && fit->num_points) ? fit->num_points : w.np;
  p.path_end = (fit && fit->path_end) ? fit->path_end : w.path_end;
  p.status = out->status; p.status_empty = TPAMD_PATH_NO_WAYPOINTS; p.status_all = 0;
  p.N = N; p.samples_in = in->num_samples_per_path; p.delta_in = in->delta;
  p.delta = (fit && fit->delta_used) ? fit->delta_used : w.delta;
  p.samples = ragged ? w.ns : nullptr;
  p.zero = w.zero;
  launch_fit_joint_waypoints(p, st);
  if (int rc = pose_ints_done(e, st)) return rc;
  const tpamd_joint_batch jb{B, D, N, S, bt->max_solver_loops, 0, bt->constraint_safety};
  tpamd_joint_inputs ji{};
  ji.knots = w.knots; ji.control_points = w.cps;
  ji.max_velocity = in->max_velocity; ji.max_acceleration = in->max_acceleration;
  ji.path_start = w.zero; ji.delta = p.delta;
  ji.sd_start = in->sd_start ? in->sd_start : w.zero;
  ji.time_start = in->time_start ? in->time_start : w.zero;
  ji.num_samples_per_path = p.samples;
  const FittedPaths fitted{p.num_points, S, any_empty};
  // never pipelined: the front stage reads what the fit, just enqueued on this stream, writes
  if (int rc = solve_joint(e, &jb, &ji, out, st, nullptr, /*allow_pipelining=*/false, &fitted)) return rc;
  if (fit && fit->knots)
    HIPCHK(hipMemcpyAsync(fit->knots, w.knots, (size_t)B * (S + 3) * 8, hipMemcpyDeviceToDevice, st));
  if (fit && fit->control_points)
    HIPCHK(hipMemcpyAsync(fit->control_points, w.cps, (size_t)B * S * D * 8, hipMemcpyDeviceToDevice, st));
  if (solved) {
    solved->jb = jb;
    solved->ji = ji;
    solved->np = p.num_points;
  }
  return 0;
}

int tpamd_time_waypoint_paths_device(tpamd_engine *e, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                                     const tpamd_path_outputs *out, const tpamd_waypoint_fit_outputs *fit,
                                     void *hip_stream) {
  return waypoint_solve(e, bt, in, out, fit, hip_stream, nullptr);
}

int tpamd_time_waypoint_paths_host(tpamd_engine *e, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                                   const tpamd_path_outputs *out, const tpamd_waypoint_fit_outputs *fit) {
  std::vector<int32_t> np;
  int slot = 0;
  bool any_empty = false;
  if (int rc = waypoint_timing_args(e, bt, in, out, &np, &slot, &any_empty)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples, S = slot;
  if (in->num_samples_per_path)
    for (size_t k = 0; k < B; k++)
      if (in->num_samples_per_path[k] > bt->num_samples) return TPAMD_E_INVALID_ARGUMENT;
  if (B == 0) return 0;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_waypoint_inputs din{};
  tpamd_path_outputs dout{};
  tpamd_waypoint_fit_outputs dfit{};
  HostStage s;
  stage_waypoint(s, bt, in, out, fit, S, any_empty, &din, &dout, &dfit);
  if (int rc = s.upload(e->stage, st)) return rc;
  if (int rc = upload_kept_path_outputs(B, any_empty, out, &dout, st)) return rc;
  int rc = tpamd_time_waypoint_paths_device(e, bt, &din, &dout, &dfit, st);
  return rc ? rc : s.download(st);
}

}  // extern "C"

// ---- checking solutions against their constraint rows (tpamd_check.h) ----------------------------
namespace {
constexpr int kMaxCheckPaths = 65535;

// What the three forms check of the solution and the outputs.
int check_io_args(const tpamd_solution *sol, const tpamd_check_outputs *out) {
  if (!sol || !out || !sol->sdd || (!sol->sd2 && !sol->sd) || !out->violations) return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}
CheckSolution check_solution(const tpamd_solution *sol) {
  return CheckSolution{sol->sd2, sol->sd2 ? nullptr : sol->sd, sol->sdd, sol->status};
}
CheckOutputs check_outputs(const tpamd_check_outputs *out) {
  return CheckOutputs{out->violations, out->worst_excess, out->worst_sample, out->worst_row, out->first_sample};
}

// The checks of the three forms behind the null structs and num_paths <= 0: the sizes as the solve
// entry refuses them, then the arrays the check reads.
int check_rows_args(const tpamd_rows_batch *bt, const tpamd_rows_inputs *in) {
  const int N = bt->num_samples, C = bt->num_rows;
  if (C < 1 || C > 64 || N < 3 || N > 8192 || bt->num_paths > kMaxCheckPaths) return TPAMD_E_UNSUPPORTED;
  if (!in->a || !in->b || !in->lower || !in->upper) return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}
int check_joint_args(const tpamd_joint_batch *bt, const tpamd_joint_inputs *in) {
  const int D = bt->num_dofs, N = bt->num_samples, P = bt->num_points;
  if (D < 1 || D > 16 || N < 3 || N > 8192 || P < 3 || bt->num_paths > kMaxCheckPaths) return TPAMD_E_UNSUPPORTED;
  if (!in->knots || !in->control_points || !in->max_velocity || !in->max_acceleration || !in->path_start ||
      !in->delta)
    return TPAMD_E_INVALID_ARGUMENT;
  // the solve's limit: the sampling/LP kernel's LDS at the block size it takes for this batch
  if (sample_lp_lds(P, D, sample_lp_block(false, in->num_samples_per_path != nullptr, D)) > kSampleLpLdsLimit)
    return TPAMD_E_UNSUPPORTED;
  return 0;
}
int check_cartesian_args(const tpamd_cartesian_batch *bt, const tpamd_cartesian_inputs *in) {
  const int D = bt->num_dofs, N = bt->num_samples;
  if (D < 1 || D > 16 || N < 3 || N > 8192 || bt->num_paths > kMaxCheckPaths) return TPAMD_E_UNSUPPORTED;
  if (!in->ik_positions || !in->jacobians || !in->max_velocity || !in->max_acceleration ||
      !in->max_translational_velocity || !in->max_rotational_velocity || !in->delta)
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

// The solution and the record arrays of a _host check in `s`.
void stage_check_io(HostStage &s, size_t B, size_t N, const tpamd_solution *sol, const tpamd_check_outputs *out,
                    tpamd_solution *dsol, tpamd_check_outputs *dout) {
  s.up(&dsol->sd2, sol->sd2, B * N);
  s.up(&dsol->sd, sol->sd2 ? nullptr : sol->sd, B * N);
  s.up(&dsol->sdd, sol->sdd, B * N);
  s.up(&dsol->status, sol->status, B);
  s.down(&dout->violations, out->violations, B);
  s.down(&dout->worst_excess, out->worst_excess, B);
  s.down(&dout->worst_sample, out->worst_sample, B);
  s.down(&dout->worst_row, out->worst_row, B);
  s.down(&dout->first_sample, out->first_sample, B);
}
}  // namespace

extern "C" {

int tpamd_check_rows_device(tpamd_engine *e, const tpamd_rows_batch *bt, const tpamd_rows_inputs *in,
                            const int32_t *num_samples_per_path, const tpamd_solution *sol,
                            const tpamd_check_outputs *out, void *hip_stream) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_rows_args(bt, in)) return rc;
  TPAMD_ON_DEVICE(e);
  hipLaunchKernelGGL(k_check_rows, dim3(bt->num_paths), dim3(kCheckThreads), 0, (hipStream_t)hip_stream,
                     bt->num_samples, bt->num_rows, in->a, in->b, in->lower, in->upper, num_samples_per_path,
                     check_solution(sol), check_outputs(out));
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_check_rows_host(tpamd_engine *e, const tpamd_rows_batch *bt, const tpamd_rows_inputs *in,
                          const int32_t *num_samples_per_path, const tpamd_solution *sol,
                          const tpamd_check_outputs *out) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_rows_args(bt, in)) return rc;
  const size_t B = bt->num_paths, N = bt->num_samples, C = bt->num_rows;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_rows_inputs din{};
  tpamd_solution dsol{};
  tpamd_check_outputs dout{};
  const int32_t *d_ns = nullptr;
  HostStage s;
  s.up(&din.a, in->a, B * N * C);
  s.up(&din.b, in->b, B * N * C);
  s.up(&din.lower, in->lower, B * N * C);
  s.up(&din.upper, in->upper, B * N * C);
  s.up(&d_ns, num_samples_per_path, B);
  stage_check_io(s, B, N, sol, out, &dsol, &dout);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = tpamd_check_rows_device(e, bt, &din, d_ns, &dsol, &dout, st);
  return rc ? rc : s.download(st);
}

int tpamd_check_joint_paths_device(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                                   const int32_t *num_points_per_path, const tpamd_solution *sol,
                                   const tpamd_check_outputs *out, void *hip_stream) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_joint_args(bt, in)) return rc;
  TPAMD_ON_DEVICE(e);
  hipLaunchKernelGGL(k_check_joint, dim3(bt->num_paths), dim3(kCheckThreads),
                     check_joint_lds(bt->num_points, bt->num_dofs), (hipStream_t)hip_stream, bt->num_samples,
                     bt->num_dofs, bt->num_points, bt->constraint_safety, in->knots, in->control_points,
                     in->max_velocity, in->max_acceleration, in->path_start, in->delta, in->num_samples_per_path,
                     num_points_per_path, check_solution(sol), check_outputs(out));
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_check_joint_paths_host(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                                 const int32_t *num_points_per_path, const tpamd_solution *sol,
                                 const tpamd_check_outputs *out) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_dofs < 1 || bt->num_samples < 1 || bt->num_points < 1) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_joint_args(bt, in)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples, P = bt->num_points;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_joint_inputs din{};
  tpamd_solution dsol{};
  tpamd_check_outputs dout{};
  const int32_t *d_np = nullptr;
  HostStage s;
  s.up(&din.knots, in->knots, B * (P + 3));
  s.up(&din.control_points, in->control_points, B * P * D);
  s.up(&din.max_velocity, in->max_velocity, B * D);
  s.up(&din.max_acceleration, in->max_acceleration, B * D);
  s.up(&din.path_start, in->path_start, B);
  s.up(&din.delta, in->delta, B);
  s.up(&din.num_samples_per_path, in->num_samples_per_path, B);
  s.up(&d_np, num_points_per_path, B);
  stage_check_io(s, B, N, sol, out, &dsol, &dout);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = tpamd_check_joint_paths_device(e, bt, &din, d_np, &dsol, &dout, st);
  return rc ? rc : s.download(st);
}

int tpamd_check_cartesian_paths_device(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                       const tpamd_cartesian_inputs *in, const int32_t *num_samples_per_path,
                                       const int32_t *first_row, const tpamd_solution *sol,
                                       const tpamd_check_outputs *out, void *hip_stream) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_cartesian_args(bt, in)) return rc;
  TPAMD_ON_DEVICE(e);
  hipLaunchKernelGGL(k_check_cartesian, dim3(bt->num_paths), dim3(kCheckThreads), 0, (hipStream_t)hip_stream,
                     bt->num_samples, bt->num_dofs, bt->constraint_safety, in->ik_positions, in->jacobians,
                     in->max_velocity, in->max_acceleration, in->max_translational_velocity,
                     in->max_rotational_velocity, in->delta, num_samples_per_path, first_row, check_solution(sol),
                     check_outputs(out));
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_check_cartesian_paths_host(tpamd_engine *e, const tpamd_cartesian_batch *bt,
                                     const tpamd_cartesian_inputs *in, const int32_t *num_samples_per_path,
                                     const int32_t *first_row, int64_t num_rows, const tpamd_solution *sol,
                                     const tpamd_check_outputs *out) {
  if (!e || !bt || !in) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_io_args(sol, out)) return rc;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = check_cartesian_args(bt, in)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples;
  if (first_row && (num_rows < 1 || num_rows >= ((int64_t)1 << 31))) return TPAMD_E_INVALID_ARGUMENT;
  const size_t rows = first_row ? (size_t)num_rows : B * N;
  // the rows of a path with a usable count must lie inside what is staged
  if (first_row)
    for (size_t b = 0; b < B; b++) {
      const int64_t n = num_samples_per_path ? num_samples_per_path[b] : (int64_t)N;
      if (n < 2 || n > (int64_t)N) continue;
      if (first_row[b] < 0 || (int64_t)first_row[b] + n > num_rows) return TPAMD_E_INVALID_ARGUMENT;
    }
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_cartesian_inputs din{};
  tpamd_solution dsol{};
  tpamd_check_outputs dout{};
  const int32_t *d_ns = nullptr, *d_first = nullptr;
  HostStage s;
  s.up(&din.ik_positions, in->ik_positions, rows * D);
  s.up(&din.jacobians, in->jacobians, rows * 6 * D);
  s.up(&din.max_velocity, in->max_velocity, B * D);
  s.up(&din.max_acceleration, in->max_acceleration, B * D);
  s.up(&din.max_translational_velocity, in->max_translational_velocity, B);
  s.up(&din.max_rotational_velocity, in->max_rotational_velocity, B);
  s.up(&din.delta, in->delta, B);
  s.up(&d_ns, num_samples_per_path, B);
  s.up(&d_first, first_row, B);
  stage_check_io(s, B, N, sol, out, &dsol, &dout);
  if (int rc = s.upload(e->stage, st)) return rc;
  int rc = tpamd_check_cartesian_paths_device(e, bt, &din, d_ns, d_first, &dsol, &dout, st);
  return rc ? rc : s.download(st);
}

}  // extern "C"

// ---- refining violating paths on the device (tpamd_refine.h) -------------------------------------
namespace {

// What both forms check of the options and the refine outputs, behind the plain entry's own checks.
int refine_args(const tpamd_refine_options *opt, const tpamd_refine_outputs *ref, int B, int N) {
  const tpamd_path_outputs &r = ref->refined;
  if (!ref->check.violations || !ref->slot || !ref->slot_path || !ref->num_refined || !r.time || !r.s || !r.sd ||
      !r.sdd || !r.status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (opt->max_rounds < 1 || opt->max_rounds > 8 || opt->max_samples < 3 || opt->max_samples > 8192 ||
      opt->max_samples < N || opt->max_refined < 1 || opt->max_refined > kMaxCheckPaths ||
      !(opt->tolerance >= 0.0) || B > kMaxCheckPaths)
    return TPAMD_E_UNSUPPORTED;
  return 0;
}

// The engine's scratch of a refined call: what round 0 needs beside the caller's arrays, the
// sub-batch of M slots (splines in slots of P control points), the slots' state and the record of
// the round just checked. Whatever the caller passes takes the place of its entry here.
struct RefineScratch {
  double *sd2_0, *excess_0;                  // [B][N], [B]
  double *knots, *cps, *vmax, *amax, *path_start, *sd_start, *sdd_start, *time_start;
  int32_t *np;                               // [M]
  int32_t *next_samples, *rounds, *num_samples, *live;
  double *next_delta, *delta;
  int32_t *made_violations, *made_sample, *made_row, *made_first;
  double *made_excess;
  double *sd2_r;                             // [M][max_samples]
};
size_t carve_refine_scratch(char *base, size_t B, size_t N, size_t M, size_t NS, size_t D, size_t P, bool sd2_0,
                            bool sd2_r, RefineScratch *w) {
  Stage s(base);
  w->sd2_0 = s.take<double>(sd2_0 ? B * N : 0);
  w->excess_0 = s.take<double>(B);
  w->knots = s.take<double>(M * (P + 3));
  w->cps = s.take<double>(M * P * D);
  w->vmax = s.take<double>(M * D);
  w->amax = s.take<double>(M * D);
  w->path_start = s.take<double>(M);
  w->sd_start = s.take<double>(M);
  w->sdd_start = s.take<double>(M);
  w->time_start = s.take<double>(M);
  w->np = s.take<int32_t>(M);
  w->next_samples = s.take<int32_t>(M);
  w->rounds = s.take<int32_t>(M);
  w->num_samples = s.take<int32_t>(M);
  w->live = s.take<int32_t>(1);
  w->next_delta = s.take<double>(M);
  w->delta = s.take<double>(M);
  w->made_violations = s.take<int32_t>(M);
  w->made_sample = s.take<int32_t>(M);
  w->made_row = s.take<int32_t>(M);
  w->made_first = s.take<int32_t>(M);
  w->made_excess = s.take<double>(M);
  w->sd2_r = s.take<double>(sd2_r ? M * NS : 0);
  return s.off;
}

// An earlier refined call's kernels may still read the scratch (on any stream) when it has to move.
int ensure_refine_scratch(tpamd_engine *e, int B, int N, int D, int P, const tpamd_path_outputs *out,
                          const tpamd_refine_options *opt, const tpamd_refine_outputs *ref, RefineScratch *w) {
  const size_t M = opt->max_refined, NS = opt->max_samples;
  const bool sd2_0 = out->sd2 == nullptr, sd2_r = ref->refined.sd2 == nullptr;
  const size_t need = carve_refine_scratch(nullptr, B, N, M, NS, D, P, sd2_0, sd2_r, w);
  if (need > e->refine.bytes) {
    HIPCHK(hipDeviceSynchronize());
    if (e->refine.reserve(need)) return TPAMD_E_HIP;
  }
  carve_refine_scratch((char *)e->refine.p, B, N, M, NS, D, P, sd2_0, sd2_r, w);
  return 0;
}

// Run `fn` with the refinement workspace in place of the engine's current one, and keep what the
// engine remembers of its last solve (tpamd_query_device): the rounds leave round 0 as it is.
template <class F>
int with_refine_workspace(tpamd_engine *e, F fn) {
  std::swap(e->ws_buf, e->refine_ws);
  const Workspace saved = e->ws;
  const int last_B = e->last_B, last_N = e->last_N;
  const double *last_time = e->last_time;
  const bool in_lane = e->in_lane;
  e->in_lane = true;                       // not a pipelining slot: no slot bookkeeping
  const int rc = fn();
  e->in_lane = in_lane;
  e->last_B = last_B; e->last_N = last_N; e->last_time = last_time;
  e->ws = saved;
  std::swap(e->ws_buf, e->refine_ws);
  return rc;
}

// Everything behind round 0's solve: its check, the slot map, the sub-batch and the rounds. `jb`,
// `ji` describe the batch on the device in the joint form (waypoint form: `np` = the control points
// of each path in slots of jb.num_points); out0 = round 0's outputs with sd2 set. stop_early (the
// _host entries): the count of live slots is read after every round.
int refine_rounds(tpamd_engine *e, const tpamd_joint_batch &jb, const tpamd_joint_inputs &ji, const int32_t *np,
                  const tpamd_path_outputs &out0, const tpamd_refine_options &opt, const tpamd_refine_outputs &ref,
                  const RefineScratch &w, hipStream_t st, bool stop_early) {
  const int B = jb.num_paths, D = jb.num_dofs, N = jb.num_samples, P = jb.num_points;
  const int M = opt.max_refined, NS = opt.max_samples;
  const tpamd_solution sol0{out0.sd2, nullptr, out0.sdd, out0.status};
  tpamd_check_outputs chk0 = ref.check;
  if (!chk0.worst_excess) chk0.worst_excess = w.excess_0;
  if (int rc = tpamd_check_joint_paths_device(e, &jb, &ji, np, &sol0, &chk0, st)) return rc;

  int32_t *rounds = ref.rounds ? ref.rounds : w.rounds;
  int32_t *num_samples = ref.num_samples ? ref.num_samples : w.num_samples;
  double *delta = ref.delta ? ref.delta : w.delta;
  const RefineRecord record{ref.refined_check.violations, ref.refined_check.worst_excess,
                            ref.refined_check.worst_sample, ref.refined_check.worst_row,
                            ref.refined_check.first_sample};
  RefineSelectParams sp{};
  sp.B = B; sp.M = M; sp.N = N; sp.max_samples = NS; sp.tolerance = opt.tolerance;
  sp.violations = chk0.violations; sp.worst_excess = chk0.worst_excess;
  sp.ns = ji.num_samples_per_path; sp.delta = ji.delta;
  sp.slot = ref.slot; sp.slot_path = ref.slot_path; sp.num_refined = ref.num_refined; sp.live = w.live;
  sp.rounds = rounds; sp.num_samples = num_samples; sp.delta_out = delta;
  sp.next_samples = w.next_samples; sp.next_delta = w.next_delta;
  sp.record = record;
  launch_refine_select(sp, st);

  RefineGatherParams gp{};
  gp.M = M; gp.D = D; gp.knots_per_path = P + 3; gp.points_per_path = P;
  gp.slot_path = ref.slot_path;
  gp.knots = ji.knots; gp.cps = ji.control_points; gp.vmax = ji.max_velocity; gp.amax = ji.max_acceleration;
  gp.path_start = ji.path_start; gp.sd_start = ji.sd_start; gp.sdd_start = ji.sdd_start; gp.time_start = ji.time_start;
  gp.np = np;
  gp.knots_out = w.knots; gp.cps_out = w.cps; gp.vmax_out = w.vmax; gp.amax_out = w.amax;
  gp.path_start_out = w.path_start; gp.sd_start_out = w.sd_start; gp.sdd_start_out = w.sdd_start;
  gp.time_start_out = w.time_start;
  gp.np_out = np ? w.np : nullptr;
  launch_refine_gather(gp, st);
  HIPCHK(hipGetLastError());

  const tpamd_joint_batch sb{M, D, NS, P, jb.max_solver_loops, 0, jb.constraint_safety};
  tpamd_joint_inputs si{};
  si.knots = w.knots; si.control_points = w.cps; si.max_velocity = w.vmax; si.max_acceleration = w.amax;
  si.path_start = w.path_start; si.delta = w.next_delta; si.sd_start = w.sd_start; si.sdd_start = w.sdd_start;
  si.time_start = w.time_start; si.num_samples_per_path = w.next_samples;
  tpamd_path_outputs so = ref.refined;
  if (!so.sd2) so.sd2 = w.sd2_r;
  const tpamd_solution sol{so.sd2, nullptr, so.sdd, so.status};
  const tpamd_check_outputs made{w.made_violations, w.made_excess, w.made_sample, w.made_row, w.made_first};
  const FittedPaths fitted{w.np, P, /*any_empty=*/true};
  RefineStepParams tp{};
  tp.M = M; tp.max_rounds = opt.max_rounds; tp.max_samples = NS; tp.tolerance = opt.tolerance;
  tp.made = RefineRecord{w.made_violations, w.made_excess, w.made_sample, w.made_row, w.made_first};
  tp.out = record;
  tp.rounds = rounds; tp.num_samples = num_samples; tp.delta_out = delta;
  tp.next_samples = w.next_samples; tp.next_delta = w.next_delta; tp.live = w.live;
  for (int r = 1; r <= opt.max_rounds; r++) {
    if (stop_early) {
      int live = 0;
      HIPCHK(hipMemcpyAsync(&live, w.live, sizeof live, hipMemcpyDeviceToHost, st));
      HIPCHK(hipStreamSynchronize(st));
      if (live == 0) break;
    }
    // a settled or unused slot has the count 0: skipped, its outputs stay
    const int rc = with_refine_workspace(e, [&]() {
      return solve_joint(e, &sb, &si, &so, st, nullptr, /*allow_pipelining=*/false, np ? &fitted : nullptr,
                         /*skip_zero_samples=*/true);
    });
    if (rc) return rc;
    if (int rc2 = tpamd_check_joint_paths_device(e, &sb, &si, np ? w.np : nullptr, &sol, &made, st)) return rc2;
    launch_refine_step(tp, st);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int joint_refined(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                  const tpamd_path_outputs *out, const tpamd_refine_options *opt, const tpamd_refine_outputs *ref,
                  hipStream_t st, bool stop_early) {
  TPAMD_ON_DEVICE(e);
  RefineScratch w{};
  if (int rc = ensure_refine_scratch(e, bt->num_paths, bt->num_samples, bt->num_dofs, bt->num_points, out, opt, ref, &w))
    return rc;
  tpamd_path_outputs out0 = *out;
  if (!out0.sd2) out0.sd2 = w.sd2_0;
  // round 0: the plain solve (never pipelined: its check reads the outputs directly behind it)
  if (int rc = solve_joint(e, bt, in, &out0, st, nullptr, /*allow_pipelining=*/false)) return rc;
  return refine_rounds(e, *bt, *in, nullptr, out0, *opt, *ref, w, st, stop_early);
}

// The refine outputs of a _host call in `s`. The refined solution travels up first: the entries a
// round does not write (behind a slot's count, unused slots) come back as the caller had them.
void stage_refine_outputs(HostStage &s, size_t B, size_t M, size_t NS, size_t D, const tpamd_refine_outputs *r,
                          tpamd_refine_outputs *d) {
  s.down(&d->check.violations, r->check.violations, B);
  s.down(&d->check.worst_excess, r->check.worst_excess, B);
  s.down(&d->check.worst_sample, r->check.worst_sample, B);
  s.down(&d->check.worst_row, r->check.worst_row, B);
  s.down(&d->check.first_sample, r->check.first_sample, B);
  s.down(&d->slot, r->slot, B);
  s.down(&d->slot_path, r->slot_path, M);
  s.down(&d->num_refined, r->num_refined, 1);
  s.down(&d->rounds, r->rounds, M);
  s.down(&d->num_samples, r->num_samples, M);
  s.down(&d->delta, r->delta, M);
  const tpamd_path_outputs &o = r->refined;
  tpamd_path_outputs &t = d->refined;
  s.both(&t.time, o.time, M * NS);
  s.both(&t.s, o.s, M * NS);
  s.both(&t.sd, o.sd, M * NS);
  s.both(&t.sdd, o.sdd, M * NS);
  s.both(&t.q, o.q, M * NS * D);
  s.both(&t.qd, o.qd, M * NS * D);
  s.both(&t.qdd, o.qdd, M * NS * D);
  s.both(&t.last_extremal_index, o.last_extremal_index, M);
  s.both(&t.max_time_increment, o.max_time_increment, M);
  s.both(&t.status, o.status, M);
  s.both(&t.sd2, o.sd2, M * NS);
  s.down(&d->refined_check.violations, r->refined_check.violations, M);
  s.down(&d->refined_check.worst_excess, r->refined_check.worst_excess, M);
  s.down(&d->refined_check.worst_sample, r->refined_check.worst_sample, M);
  s.down(&d->refined_check.worst_row, r->refined_check.worst_row, M);
  s.down(&d->refined_check.first_sample, r->refined_check.first_sample, M);
}

int waypoint_refined(tpamd_engine *e, const tpamd_waypoint_batch *bt, const tpamd_waypoint_inputs *in,
                     const tpamd_path_outputs *out, const tpamd_waypoint_fit_outputs *fit,
                     const tpamd_refine_options *opt, const tpamd_refine_outputs *ref, int slot_points, hipStream_t st,
                     bool stop_early) {
  TPAMD_ON_DEVICE(e);
  RefineScratch w{};
  if (int rc = ensure_refine_scratch(e, bt->num_paths, bt->num_samples, bt->num_dofs, slot_points, out, opt, ref, &w))
    return rc;
  tpamd_path_outputs out0 = *out;
  if (!out0.sd2) out0.sd2 = w.sd2_0;
  WaypointSolved solved{};
  if (int rc = waypoint_solve(e, bt, in, &out0, fit, st, &solved)) return rc;
  return refine_rounds(e, solved.jb, solved.ji, solved.np, out0, *opt, *ref, w, st, stop_early);
}

}  // namespace

extern "C" {

int tpamd_time_joint_paths_refined_device(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                                          const tpamd_path_outputs *out, const tpamd_refine_options *opt,
                                          const tpamd_refine_outputs *ref, void *hip_stream) {
  if (!e || !bt || !in || !out || !opt || !ref) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = joint_args(bt, in, out)) return rc;
  if (int rc = refine_args(opt, ref, bt->num_paths, bt->num_samples)) return rc;
  if (sample_lp_lds(bt->num_points, bt->num_dofs, sample_lp_block(false, in->num_samples_per_path != nullptr,
                                                                  bt->num_dofs)) > kSampleLpLdsLimit)
    return TPAMD_E_UNSUPPORTED;
  return joint_refined(e, bt, in, out, opt, ref, (hipStream_t)hip_stream, /*stop_early=*/false);
}

int tpamd_time_joint_paths_refined_host(tpamd_engine *e, const tpamd_joint_batch *bt, const tpamd_joint_inputs *in,
                                        const tpamd_path_outputs *out, const tpamd_refine_options *opt,
                                        const tpamd_refine_outputs *ref) {
  if (!e || !bt || !in || !out || !opt || !ref) return TPAMD_E_INVALID_ARGUMENT;
  if (bt->num_paths <= 0) return bt->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = joint_host_args(bt, in, out)) return rc;
  if (int rc = refine_args(opt, ref, bt->num_paths, bt->num_samples)) return rc;
  if (sample_lp_lds(bt->num_points, bt->num_dofs, sample_lp_block(false, in->num_samples_per_path != nullptr,
                                                                  bt->num_dofs)) > kSampleLpLdsLimit)
    return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_joint_inputs din{};
  tpamd_path_outputs dout{};
  tpamd_refine_outputs dref{};
  HostStage s;
  stage_joint(s, bt, in, out, &din, &dout);
  stage_refine_outputs(s, bt->num_paths, opt->max_refined, opt->max_samples, bt->num_dofs, ref, &dref);
  if (int rc = s.upload(e->stage, st)) return rc;
  const int rc = joint_refined(e, bt, &din, &dout, opt, &dref, st, /*stop_early=*/true);
  return rc ? rc : s.download(st);
}

int tpamd_time_waypoint_paths_refined_device(tpamd_engine *e, const tpamd_waypoint_batch *bt,
                                             const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                             const tpamd_waypoint_fit_outputs *fit, const tpamd_refine_options *opt,
                                             const tpamd_refine_outputs *ref, void *hip_stream) {
  if (!opt || !ref) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<int32_t> np;
  int S = 0;
  bool any_empty = false;
  if (int rc = waypoint_timing_args(e, bt, in, out, &np, &S, &any_empty)) return rc;
  if (bt->num_paths == 0) return 0;
  if (int rc = refine_args(opt, ref, bt->num_paths, bt->num_samples)) return rc;
  return waypoint_refined(e, bt, in, out, fit, opt, ref, S, (hipStream_t)hip_stream, /*stop_early=*/false);
}

int tpamd_time_waypoint_paths_refined_host(tpamd_engine *e, const tpamd_waypoint_batch *bt,
                                           const tpamd_waypoint_inputs *in, const tpamd_path_outputs *out,
                                           const tpamd_waypoint_fit_outputs *fit, const tpamd_refine_options *opt,
                                           const tpamd_refine_outputs *ref) {
  if (!opt || !ref) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<int32_t> np;
  int slot = 0;
  bool any_empty = false;
  if (int rc = waypoint_timing_args(e, bt, in, out, &np, &slot, &any_empty)) return rc;
  const size_t B = bt->num_paths, D = bt->num_dofs, N = bt->num_samples, S = slot;
  if (in->num_samples_per_path)
    for (size_t k = 0; k < B; k++)
      if (in->num_samples_per_path[k] > bt->num_samples) return TPAMD_E_INVALID_ARGUMENT;
  if (B == 0) return 0;
  if (int rc = refine_args(opt, ref, bt->num_paths, bt->num_samples)) return rc;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_waypoint_inputs din{};
  tpamd_path_outputs dout{};
  tpamd_waypoint_fit_outputs dfit{};
  tpamd_refine_outputs dref{};
  HostStage s;
  stage_waypoint(s, bt, in, out, fit, S, any_empty, &din, &dout, &dfit);
  stage_refine_outputs(s, B, opt->max_refined, opt->max_samples, D, ref, &dref);
  if (int rc = s.upload(e->stage, st)) return rc;
  if (int rc = upload_kept_path_outputs(B, any_empty, out, &dout, st)) return rc;
  const int rc = waypoint_refined(e, bt, &din, &dout, &dfit, opt, &dref, slot, st, /*stop_early=*/true);
  return rc ? rc : s.download(st);
}

}  // extern "C"

namespace {
// The checks of both resample entries after the null structs and num_paths <= 0.
int resample_args(const tpamd_resample_args *a) {
  if (a->num_samples < 2 || a->num_dofs < 1 || a->max_out < 1 || !(a->time_step > 0))
    return TPAMD_E_INVALID_ARGUMENT;
  if (!a->time || !a->s || !a->sd || !a->sdd || !a->q || !a->qd || !a->qdd ||
      !a->max_acceleration || !a->start_sec || !a->out_time || !a->out_s || !a->out_sd ||
      !a->out_sdd || !a->out_q || !a->out_qd || !a->out_qdd || !a->count)
    return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}

int resample_device(tpamd_engine *e, const tpamd_resample_args *a, void *hip_stream, bool skip_mode) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = resample_args(a)) return rc;
  TPAMD_ON_DEVICE(e);
  ResampleParams p;
  p.B = a->num_paths; p.N = a->num_samples; p.D = a->num_dofs; p.max_out = a->max_out;
  p.time = a->time; p.s = a->s; p.sd = a->sd; p.sdd = a->sdd;
  p.q = a->q; p.qd = a->qd; p.qdd = a->qdd; p.amax = a->max_acceleration;
  p.start_sec = a->start_sec; p.time_step = a->time_step; p.status = a->status;
  p.ot = a->out_time; p.os = a->out_s; p.osd = a->out_sd; p.osdd = a->out_sdd;
  p.oq = a->out_q; p.oqd = a->out_qd; p.oqdd = a->out_qdd; p.count = a->count;
  if (skip_mode) {
    p.time_step = 0.95 * a->time_step;   // GetMinTimeDeltaToKeep, path_timing_trajectory.cc:893-900
    hipLaunchKernelGGL(k_resample_skip, dim3(a->num_paths), dim3(64), 0, (hipStream_t)hip_stream, p);
  } else {
    hipLaunchKernelGGL(k_resample, dim3((a->max_out + 255) / 256, a->num_paths), dim3(256), 0,
                       (hipStream_t)hip_stream, p);
  }
  HIPCHK(hipGetLastError());
  return 0;
}

int resample_host(tpamd_engine *e, const tpamd_resample_args *a, bool skip_mode) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (int rc = resample_args(a)) return rc;
  const size_t B = a->num_paths, N = a->num_samples, D = a->num_dofs, M = a->max_out;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_resample_args da = *a;
  HostStage s;
  s.up(&da.time, a->time, B * N);
  s.up(&da.s, a->s, B * N);
  s.up(&da.sd, a->sd, B * N);
  s.up(&da.sdd, a->sdd, B * N);
  s.up(&da.q, a->q, B * N * D);
  s.up(&da.qd, a->qd, B * N * D);
  s.up(&da.qdd, a->qdd, B * N * D);
  s.up(&da.max_acceleration, a->max_acceleration, B * D);
  s.up(&da.start_sec, a->start_sec, B);
  s.up(&da.status, a->status, B);
  s.down(&da.out_time, a->out_time, B * M);
  s.down(&da.out_s, a->out_s, B * M);
  s.down(&da.out_sd, a->out_sd, B * M);
  s.down(&da.out_sdd, a->out_sdd, B * M);
  s.down(&da.out_q, a->out_q, B * M * D);
  s.down(&da.out_qd, a->out_qd, B * M * D);
  s.down(&da.out_qdd, a->out_qdd, B * M * D);
  s.down(&da.count, a->count, B);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = resample_device(e, &da, st, skip_mode);
  return rc ? rc : s.download(st);
}
}  // namespace

extern "C" {

int tpamd_resample_uniform_device(tpamd_engine *e, const tpamd_resample_args *a, void *hip_stream) {
  return resample_device(e, a, hip_stream, false);
}
int tpamd_resample_uniform_host(tpamd_engine *e, const tpamd_resample_args *a) {
  return resample_host(e, a, false);
}
int tpamd_resample_skip_device(tpamd_engine *e, const tpamd_resample_args *a, void *hip_stream) {
  return resample_device(e, a, hip_stream, true);
}
int tpamd_resample_skip_host(tpamd_engine *e, const tpamd_resample_args *a) {
  return resample_host(e, a, true);
}

}  // extern "C"

// The checks of both fastest-stop entries after the null structs and num_paths <= 0.
static bool fastest_stop_args_ok(const tpamd_fastest_stop_args *a) {
  if (a->stride < 1 || a->num_dofs < 1 || a->num_dofs > 16) return false;
  if (!a->time || !a->s || !a->qd || !a->qdd || !a->max_acceleration || !a->query_time ||
      !a->stop_parameter || !a->stop_index || !a->duration || !a->status)
    return false;
  const int np = (a->profile_time != nullptr) + (a->profile_rate2 != nullptr) + (a->profile_drate2 != nullptr);
  return np == 0 || np == 3;
}

extern "C" {

int tpamd_fastest_stop_device(tpamd_engine *e, const tpamd_fastest_stop_args *a, void *hip_stream) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (!fastest_stop_args_ok(a)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  FastestStopParams p{};
  p.Q = a->num_paths; p.stride = a->stride;
  p.time = a->time; p.s = a->s; p.qd = a->qd; p.qdd = a->qdd; p.count = a->count;
  p.amax = a->max_acceleration; p.query_sec = a->query_time;
  p.stop_s = a->stop_parameter; p.stop_index = a->stop_index; p.duration = a->duration; p.status = a->status;
  p.p_time = a->profile_time; p.p_rate2 = a->profile_rate2; p.p_drate2 = a->profile_drate2;
  if (!launch_fastest_stop(a->num_dofs, p, (hipStream_t)hip_stream)) return TPAMD_E_INVALID_ARGUMENT;
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_fastest_stop_host(tpamd_engine *e, const tpamd_fastest_stop_args *a) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (!fastest_stop_args_ok(a)) return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = a->num_paths, M = a->stride, D = a->num_dofs;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_fastest_stop_args da = *a;
  HostStage s;
  s.up(&da.time, a->time, B * M);
  s.up(&da.s, a->s, B * M);
  s.up(&da.qd, a->qd, B * M * D);
  s.up(&da.qdd, a->qdd, B * M * D);
  s.up(&da.count, a->count, B);
  s.up(&da.max_acceleration, a->max_acceleration, B * D);
  s.up(&da.query_time, a->query_time, B);
  s.down(&da.stop_parameter, a->stop_parameter, B);
  s.down(&da.stop_index, a->stop_index, B);
  s.down(&da.duration, a->duration, B);
  s.down(&da.status, a->status, B);
  // the kernel writes a prefix of each profile row; the rest must come back as the caller
  // had it (as with the device entry), not as an earlier host call left the staging buffer
  s.both(&da.profile_time, a->profile_time, B * M);
  s.both(&da.profile_rate2, a->profile_rate2, B * M);
  s.both(&da.profile_drate2, a->profile_drate2, B * M);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  rc = tpamd_fastest_stop_device(e, &da, st);
  return rc ? rc : s.download(st);
}

int tpamd_debug_copy_boundary(tpamd_engine *e, int B, int N, double *sd2_max, double *sdd_max,
                              double *sdd_min, double *sd2_zero, uint8_t *type, double *sd2) {
  if (!e || B != e->last_B || N != e->last_N) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  HIPCHK(hipDeviceSynchronize());
  const size_t n = (size_t)B * N;
  if (sd2_max) HIPCHK(hipMemcpy(sd2_max, e->ws.m, n * 8, hipMemcpyDeviceToHost));
  if (sdd_max) HIPCHK(hipMemcpy(sdd_max, e->ws.X, n * 8, hipMemcpyDeviceToHost));
  if (sdd_min) HIPCHK(hipMemcpy(sdd_min, e->ws.Y, n * 8, hipMemcpyDeviceToHost));
  if (sd2_zero) HIPCHK(hipMemcpy(sd2_zero, e->ws.z0, n * 8, hipMemcpyDeviceToHost));
  if (type) {
    HIPCHK(hipMemcpy(type, e->ws.type, n, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < n; i++) type[i] &= kBndTypeMask;  // drop the engine-internal cache bit
  }
  if (sd2) HIPCHK(hipMemcpy(sd2, e->ws.sd2, n * 8, hipMemcpyDeviceToHost));
  return 0;
}

void tpamd_debug_keep_boundary(tpamd_engine *e, int on) {
  if (e) e->keep_boundary = on != 0;
}

int tpamd_debug_kernel_vgprs(tpamd_engine *e, int which) {
  if (!e || which < 0 || which > 1) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipFuncAttributes attr;
  if (which == 0)
    HIPCHK(hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&k_sample_lp_joint<1, 7>)));
  else
    HIPCHK((sweep_joint_attributes<7, 0>(&attr)));
  return attr.numRegs;
}

int tpamd_debug_copy_diag(tpamd_engine *e, int B, long long *out) {
  if (!e || !out || B != e->last_B) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy2D(out, 64 * 8, e->ws.diag, kDiagRow * 8, 64 * 8, (size_t)B, hipMemcpyDeviceToHost));
  return 0;
}

int tpamd_debug_copy_diag_ext(tpamd_engine *e, int B, long long *out) {
  if (!e || !out || B != e->last_B) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy2D(out, 2 * kDiagExt * 8, e->ws.diag + 64, kDiagRow * 8, 2 * kDiagExt * 8, (size_t)B,
                     hipMemcpyDeviceToHost));
  return 0;
}

void tpamd_profile_enable(tpamd_engine *e, int enable) {
  if (e) e->profile = (enable == 2) ? 2 : (enable != 0 ? 1 : 0);
}

void tpamd_profile_reset(tpamd_engine *e) {
  if (!e) return;
  DeviceScope scope(e->device);
  fold_events(e);   // recycles the events
  for (int k = 0; k < KI_COUNT; k++) { e->acc_ms[k] = 0.0; e->acc_n[k] = 0; }
}

double tpamd_profile_mean_ms(tpamd_engine *e, int kernel_index, int *num_launches) {
  if (num_launches) *num_launches = 0;
  if (!e || kernel_index < 0 || kernel_index >= KI_COUNT) return 0.0;
  DeviceScope scope(e->device);
  fold_events(e);
  const int n = e->acc_n[kernel_index];
  if (num_launches) *num_launches = n;
  return n ? e->acc_ms[kernel_index] / n : 0.0;
}

const char *tpamd_profile_kernel_name(int k) { return (k >= 0 && k < KI_COUNT) ? kKernelNames[k] : ""; }
int tpamd_profile_num_kernels(void) { return KI_COUNT; }

}  // extern "C"

static bool stop_batch_args_ok(const tpamd_stop_trajectory_args *a) {
  if (a->stride < 1 || a->num_dofs < 1 || a->num_dofs > 16) return false;
  return a->time && a->qd && a->qdd && a->max_acceleration && (a->stop_time || a->stop_index) && a->status &&
         a->keep && a->first && a->last && a->out_time && a->out_qd && a->out_qdd;
}

int tpamd_stop_trajectories_device(tpamd_engine *e, const tpamd_stop_trajectory_args *a, void *hip_stream) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (!stop_batch_args_ok(a)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  StopTrajParams p{};
  p.Q = p.B = a->num_paths; p.stride = a->stride; p.mode = kRsBatch;
  p.time = a->time; p.qd = a->qd; p.qdd = a->qdd; p.count = a->count;
  p.amax = a->max_acceleration; p.time_step = a->time_step;
  p.stop_sec = a->stop_time; p.stop_index = a->stop_index;
  p.status = a->status; p.keep = a->keep; p.seg_first = a->first; p.seg_last = a->last;
  p.o_time = a->out_time; p.o_qd = a->out_qd; p.o_qdd = a->out_qdd;
  if (!launch_stop_trajectories(a->num_dofs, p, (hipStream_t)hip_stream)) return TPAMD_E_INVALID_ARGUMENT;
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_stop_trajectories_host(tpamd_engine *e, const tpamd_stop_trajectory_args *a) {
  if (!e || !a) return TPAMD_E_INVALID_ARGUMENT;
  if (a->num_paths <= 0) return a->num_paths == 0 ? 0 : TPAMD_E_INVALID_ARGUMENT;
  if (!stop_batch_args_ok(a)) return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = a->num_paths, M = a->stride, D = a->num_dofs;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  tpamd_stop_trajectory_args da = *a;
  std::vector<int32_t> res(4 * B);   // status, keep, first, last: one copy down
  int32_t *d_res = nullptr;
  HostStage s;
  s.up(&da.time, a->time, B * M);
  s.up(&da.qd, a->qd, B * M * D);
  s.up(&da.qdd, a->qdd, B * M * D);
  s.up(&da.count, a->count, B);
  s.up(&da.max_acceleration, a->max_acceleration, B * D);
  s.up(&da.stop_time, a->stop_index ? nullptr : a->stop_time, B);
  s.up(&da.stop_index, a->stop_index, B);
  s.down(&d_res, res.data(), 4 * B);
  // only the segments' rows are written; the rest must come back as the caller had it
  s.both(&da.out_time, a->out_time, B * M);
  s.both(&da.out_qd, a->out_qd, B * M * D);
  s.both(&da.out_qdd, a->out_qdd, B * M * D);
  int rc = s.upload(e->stage, st);
  if (rc) return rc;
  da.status = d_res; da.keep = d_res + B; da.first = d_res + 2 * B; da.last = d_res + 3 * B;
  rc = tpamd_stop_trajectories_device(e, &da, st);
  if (!rc) rc = s.download(st);
  if (rc) return rc;
  std::memcpy(a->status, res.data(), 4 * B);
  std::memcpy(a->keep, res.data() + B, 4 * B);
  std::memcpy(a->first, res.data() + 2 * B, 4 * B);
  std::memcpy(a->last, res.data() + 3 * B, 4 * B);
  return 0;
}


// ---------------------------------------------------------------- planner sets
struct tpamd_planner_set {
  tpamd_engine *e = nullptr;
  tpamd_planner_set_config cfg{};
  int cap = 0, tcap = 0;
  int pcap = 0;                         // control points per planner the path arrays hold (P_cap)
  // fixed-size state (one allocation); paths, history and trajectory (one allocation each: they grow)
  void *fixed = nullptr, *hist = nullptr, *traj = nullptr, *path = nullptr;
  size_t fixed_bytes = 0, hist_bytes = 0, traj_bytes = 0, path_bytes = 0;
  // host copies of S.np and S.has_path: they change only through uploads, switches and resets
  std::vector<int> h_np;
  mutable std::vector<char> h_has;     // (mutable: refresh_table_counts fills the cache from a const entry)
  // a device retarget's outcome is known on the device only: h_np holds an upper bound until
  // refresh_path_counts reads the planner's count back
  std::vector<char> h_stale;
  DeviceBuffer sw_buf;                  // switch calls: inputs, outputs and the edit's scratch
  PlannerSetState S{};
  PlanParams P{};
  // device arrays that are not part of S / P
  double *d_cp = nullptr, *d_vmax = nullptr, *d_delta = nullptr, *d_iv = nullptr, *d_sdd0 = nullptr;
  double *w_s = nullptr, *w_sd = nullptr, *w_sdd = nullptr, *w_q = nullptr, *w_qd = nullptr, *w_qdd = nullptr,
         *w_dtm = nullptr, *w_time = nullptr;
  int32_t *w_lei = nullptr, *w_st = nullptr;
  int *d_windows = nullptr;
  long long *d_start = nullptr, *d_horizon = nullptr, *d_loop_start = nullptr;
  PlannerSummaryDev *d_summary = nullptr;
  int *d_need_cap = nullptr;            // plan_device: [2][B] history / trajectory samples a planner lacked
  char *d_stop_in = nullptr, *d_stop_out = nullptr;   // stop queries: [time_ns][ids], [s][duration][status]
  size_t last_h2d = 0, last_d2h = 0;
  // staging of the host readouts (inputs and offsets | packed rows or tick values); they grow
  DeviceBuffer rd_in, rd_out;
  // device readouts run on the caller's stream: ev_set orders them after the set's last change,
  // ev_read (recorded after each of them) orders the next change after them
  hipEvent_t ev_set = nullptr, ev_read = nullptr;
  bool read_pending = false;
  // stopping trajectories: per-listed-planner scratch (segment rows, shift, length; host variant:
  // status, keep, offsets as well)
  DeviceBuffer stop_buf;
  // set_waypoints calls: device inputs and outputs; the _device variant stages ids and offsets in
  // pinned memory, which ev_wp (recorded after their copy) guards against the next call
  DeviceBuffer wp_buf;
  void *wp_pin = nullptr;
  size_t wp_pin_bytes = 0;
  hipEvent_t ev_wp = nullptr;
  bool wp_pin_busy = false;
  // Cartesian sets: the IK tables [B][table_cap][D] | [B][table_cap][6][D] (one allocation; it
  // grows), a host copy of the row counts and of the first resident rows (slot 0 of planner b's
  // table holds path row first_row[b]; rows below it were discarded), and the per-planner Cartesian
  // limits and path ends (part of `fixed`). The upload entries share wp_buf / wp_pin with set_waypoints.
  bool cartesian = false;
  int table_cap = 0;
  void *table = nullptr;
  size_t table_bytes = 0;
  double *d_tq = nullptr, *d_tJ = nullptr;
  mutable std::vector<int> h_rows, h_first_row;
  double *d_vtrans = nullptr, *d_vrot = nullptr, *d_path_end = nullptr;
  int *d_rows = nullptr, *d_first = nullptr, *d_first_row = nullptr;
  // streaming Plan: the planners that wait for rows (device flags and host copy), what they lack
  // ([need_first[B]][need_count[B]], one copy down per call) and whether P carries the arrays
  int *d_suspended = nullptr, *d_need = nullptr;
  std::vector<char> h_wait;
  std::vector<int32_t> h_need;
  int num_waiting = 0;
  bool streaming = false;
  // tpamd_planner_set_set_checking: the solver's sd2 of the window being solved [B][N] and the
  // per-planner records [B] (one allocation, made when checking is first switched on and kept)
  bool checking = false;
  DeviceBuffer check_buf;
  // state records (tpamd_state.h): the host entries' staging, the layout kernel's per-planner
  // scratch, and "a device import may have changed row counts that h_rows / h_first_row do not show"
  DeviceBuffer state_buf, state_items;
  mutable bool table_stale = false;
  double *d_sd2 = nullptr;
  PlannerCheckDev *d_check = nullptr;
};

namespace {

// knots [B][pcap + 3] | control points [B][pcap][D]
size_t carve_paths(char *base, size_t B, size_t pcap, size_t D, tpamd_planner_set *ps) {
  Stage st(base);
  double *k = st.take<double>(B * (pcap + 3)), *cp = st.take<double>(B * pcap * D);
  if (ps) { ps->S.knots = k; ps->d_cp = cp; ps->S.K = (int)pcap + 3; }
  return st.off;
}
size_t carve_history(char *base, size_t B, size_t cap, size_t D, tpamd_planner_set *ps) {
  Stage st(base);
  double *t = st.take<double>(B * cap), *s = st.take<double>(B * cap), *sd = st.take<double>(B * cap),
         *sdd = st.take<double>(B * cap);
  double *q = st.take<double>(B * cap * D), *qd = st.take<double>(B * cap * D), *qdd = st.take<double>(B * cap * D);
  if (ps) {
    ps->S.h_time = t; ps->S.h_s = s; ps->S.h_sd = sd; ps->S.h_sdd = sdd; ps->S.h_q = q; ps->S.h_qd = qd; ps->S.h_qdd = qdd;
  }
  return st.off;
}
size_t carve_trajectory(char *base, size_t B, size_t tcap, size_t D, tpamd_planner_set *ps) {
  Stage st(base);
  double *t = st.take<double>(B * tcap), *s = st.take<double>(B * tcap), *sd = st.take<double>(B * tcap),
         *sdd = st.take<double>(B * tcap);
  double *q = st.take<double>(B * tcap * D), *qd = st.take<double>(B * tcap * D), *qdd = st.take<double>(B * tcap * D);
  if (ps) {
    ps->S.t_time = t; ps->S.t_s = s; ps->S.t_sd = sd; ps->S.t_sdd = sdd; ps->S.t_q = q; ps->S.t_qd = qd; ps->S.t_qdd = qdd;
  }
  return st.off;
}

// IK positions [B][rows][D] | Jacobians [B][rows][6][D]
size_t carve_table(char *base, size_t B, size_t rows, size_t D, tpamd_planner_set *ps) {
  Stage st(base);
  double *q = st.take<double>(B * rows * D), *J = st.take<double>(B * rows * 6 * D);
  if (ps) { ps->d_tq = q; ps->d_tJ = J; }
  return st.off;
}

// PlanParams view of the set (the window-loop kernels of tpamd_kernels.h)
void refresh_plan_params(tpamd_planner_set *ps) {
  PlannerSetState &S = ps->S;
  PlanParams &p = ps->P;
  S.path_end = ps->cartesian ? ps->d_path_end : nullptr;
  p.path_end = S.path_end;
  p.rows = ps->cartesian ? ps->d_rows : nullptr;
  p.first_row = ps->cartesian ? ps->d_first_row : nullptr;
  p.first = ps->d_first;
  p.rec_stride = 0;
  p.suspended = ps->streaming ? ps->d_suspended : nullptr;
  p.need_first = ps->streaming ? ps->d_need : nullptr;
  p.need_count = ps->streaming ? ps->d_need + S.B : nullptr;
  p.B = S.B; p.N = S.N; p.D = S.D; p.K = S.K; p.cap = ps->cap; p.np = S.np;
  p.max_iterations = ps->cfg.max_planning_iterations;
  p.max_initial_velocity_error = ps->cfg.max_initial_velocity_error;
  p.knots = S.knots; p.delta = ps->d_delta; p.initial_velocity = ps->d_iv;
  p.start_ns = ps->d_start; p.horizon_ns = ps->d_horizon;
  p.path_state = S.path_state; p.count = S.count;
  p.h_time = S.h_time; p.h_s = S.h_s; p.h_sd = S.h_sd; p.h_sdd = S.h_sdd; p.h_q = S.h_q; p.h_qd = S.h_qd; p.h_qdd = S.h_qdd;
  p.planned_to_end = S.planned_to_end; p.path_horizon = S.path_horizon; p.final_decel_start_ns = S.final_decel_start_ns;
  p.active = S.active; p.status = S.status; p.windows = ps->d_windows; p.loop_start_ns = ps->d_loop_start;
  p.num_active = S.num_active;
  p.path_start = S.path_start; p.sd_start = S.path_start_velocity; p.time_start = S.path_time_start;
  p.w_time = ps->w_time; p.w_s = ps->w_s; p.w_sd = ps->w_sd; p.w_sdd = ps->w_sdd; p.w_q = ps->w_q; p.w_qd = ps->w_qd;
  p.w_qdd = ps->w_qdd; p.w_status = ps->w_st; p.w_lei = ps->w_lei;
  S.cap = ps->cap; S.tcap = ps->tcap;
}

// Move the histories (or trajectories) to buffers with a larger per-planner capacity.
int grow_rows(tpamd_planner_set *ps, bool history, int new_cap, hipStream_t st) {
  const size_t B = ps->S.B, D = ps->S.D;
  PlannerSetState old = ps->S;
  void *old_base = history ? ps->hist : ps->traj;
  const int old_cap = history ? ps->cap : ps->tcap;
  const size_t need = history ? carve_history(nullptr, B, new_cap, D, nullptr) : carve_trajectory(nullptr, B, new_cap, D, nullptr);
  void *fresh = nullptr;
  HIPCHK(hipMalloc(&fresh, need));
  if (history) { carve_history((char *)fresh, B, new_cap, D, ps); ps->hist = fresh; ps->hist_bytes = need; ps->cap = new_cap; }
  else { carve_trajectory((char *)fresh, B, new_cap, D, ps); ps->traj = fresh; ps->traj_bytes = need; ps->tcap = new_cap; }
  const int *first = history ? nullptr : old.t_first;
  const int *count = history ? old.count : old.t_count;
  const dim3 g1((old_cap + 255) / 256, (unsigned)B), gD((unsigned)(((size_t)old_cap * D + 255) / 256), (unsigned)B);
  const double *src1[4] = {history ? old.h_time : old.t_time, history ? old.h_s : old.t_s, history ? old.h_sd : old.t_sd,
                           history ? old.h_sdd : old.t_sdd};
  double *dst1[4] = {history ? ps->S.h_time : ps->S.t_time, history ? ps->S.h_s : ps->S.t_s,
                     history ? ps->S.h_sd : ps->S.t_sd, history ? ps->S.h_sdd : ps->S.t_sdd};
  const double *srcD[3] = {history ? old.h_q : old.t_q, history ? old.h_qd : old.t_qd, history ? old.h_qdd : old.t_qdd};
  double *dstD[3] = {history ? ps->S.h_q : ps->S.t_q, history ? ps->S.h_qd : ps->S.t_qd, history ? ps->S.h_qdd : ps->S.t_qdd};
  for (int k = 0; k < 4; k++)
    hipLaunchKernelGGL(k_pset_regrow, g1, dim3(256), 0, st, (int)B, old_cap, new_cap, 1, first, count, src1[k], dst1[k]);
  for (int k = 0; k < 3; k++)
    hipLaunchKernelGGL(k_pset_regrow, gD, dim3(256), 0, st, (int)B, old_cap, new_cap, (int)D, first, count, srcD[k], dstD[k]);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(old_base));
  refresh_plan_params(ps);
  return 0;
}

// Move the paths to arrays of a larger per-planner capacity (P_cap); contents unchanged.
int grow_paths(tpamd_planner_set *ps, int new_pcap, hipStream_t st) {
  const size_t B = ps->S.B, D = ps->S.D, old_p = ps->pcap, new_p = new_pcap;
  const double *old_k = ps->S.knots, *old_cp = ps->d_cp;
  void *old_base = ps->path;
  const size_t need = carve_paths(nullptr, B, new_p, D, nullptr);
  void *fresh = nullptr;
  HIPCHK(hipMalloc(&fresh, need));
  carve_paths((char *)fresh, B, new_p, D, ps);
  ps->path = fresh; ps->path_bytes = need; ps->pcap = new_pcap;
  HIPCHK(hipMemcpy2DAsync((double *)ps->S.knots, (new_p + 3) * 8, old_k, (old_p + 3) * 8, (old_p + 3) * 8, B,
                          hipMemcpyDeviceToDevice, st));
  HIPCHK(hipMemcpy2DAsync(ps->d_cp, new_p * D * 8, old_cp, old_p * D * 8, old_p * D * 8, B,
                          hipMemcpyDeviceToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(old_base));
  refresh_plan_params(ps);
  return 0;
}

// P_cap by doubling until `need` points fit
int ensure_pcap(tpamd_planner_set *ps, int need, hipStream_t st) {
  if (need <= ps->pcap) return 0;
  int p = ps->pcap;
  while (p < need) p *= 2;
  return grow_paths(ps, p, st);
}

// Move the IK tables to arrays of a larger per-planner capacity (rows): the live rows (slots 0 ..
// rows - first_row - 1 of every planner, as the host counts them) are copied, first_row stays.
int refresh_table_counts(const tpamd_planner_set *ps);
int grow_table(tpamd_planner_set *ps, int new_cap, hipStream_t st) {
  if (int rc = refresh_table_counts(ps)) return rc;
  const size_t B = ps->S.B, D = ps->S.D, old_r = ps->table_cap, new_r = new_cap;
  const double *old_q = ps->d_tq, *old_J = ps->d_tJ;
  void *old_base = ps->table;
  const size_t need = carve_table(nullptr, B, new_r, D, nullptr);
  void *fresh = nullptr;
  HIPCHK(hipMalloc(&fresh, need));
  carve_table((char *)fresh, B, new_r, D, ps);
  ps->table = fresh; ps->table_bytes = need; ps->table_cap = new_cap;
  HIPCHK(hipMemsetAsync(fresh, 0, need, st));
  size_t live = 0;
  for (size_t b = 0; b < B; b++) live = std::max(live, (size_t)std::max(ps->h_rows[b] - ps->h_first_row[b], 0));
  live = std::min(live, old_r);
  if (live > 0) {
    HIPCHK(hipMemcpy2DAsync(ps->d_tq, new_r * D * 8, old_q, old_r * D * 8, live * D * 8, B, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpy2DAsync(ps->d_tJ, new_r * 6 * D * 8, old_J, old_r * 6 * D * 8, live * 6 * D * 8, B,
                            hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(old_base));
  refresh_plan_params(ps);
  return 0;
}

// table capacity by doubling until `need` rows fit
int ensure_table_cap(tpamd_planner_set *ps, int need, hipStream_t st) {
  if (need <= ps->table_cap) return 0;
  long long r = ps->table_cap;
  while (r < need) r *= 2;
  if (r > (1 << 28)) return TPAMD_E_UNSUPPORTED;
  return grow_table(ps, (int)r, st);
}

// The host copies of np / has_path of a planner that a device retarget touched (h_stale), read
// back after that call has finished.
int refresh_path_counts(tpamd_planner_set *ps, int b) {
  if (!ps->h_stale[b]) return 0;
  TPAMD_ON_DEVICE(ps->e);
  if (ps->read_pending) HIPCHK(hipEventSynchronize(ps->ev_read));
  int np = 0, has = 0;
  HIPCHK(hipMemcpy(&np, ps->S.np + b, 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&has, ps->S.has_path + b, 4, hipMemcpyDeviceToHost));
  ps->h_np[b] = np;
  ps->h_has[b] = (char)has;
  ps->h_stale[b] = 0;
  return 0;
}

// The host copies of the row counts of a Cartesian set after a device import
// (tpamd_planner_set_import_state_device), read back once that call has finished.
int refresh_table_counts(const tpamd_planner_set *ps) {
  if (!ps->table_stale) return 0;
  TPAMD_ON_DEVICE(ps->e);
  if (ps->read_pending) HIPCHK(hipEventSynchronize(ps->ev_read));
  const size_t B = ps->S.B;
  std::vector<int> has(B);
  HIPCHK(hipMemcpy(ps->h_rows.data(), ps->d_rows, B * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(ps->h_first_row.data(), ps->d_first_row, B * 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(has.data(), ps->S.has_path, B * 4, hipMemcpyDeviceToHost));
  for (size_t b = 0; b < B; b++) ps->h_has[b] = (char)has[b];
  ps->table_stale = false;
  return 0;
}

int largest_points(const tpamd_planner_set *ps) {
  int m = 3;
  for (int v : ps->h_np) m = std::max(m, v);
  return m;
}

// A planner that waits for rows (streaming Plan) stops waiting: its table is replaced or it is reset.
int drop_suspension(tpamd_planner_set *ps, int b, hipStream_t st) {
  if (!ps->num_waiting || !ps->h_wait[b]) return 0;
  HIPCHK(hipMemsetAsync(ps->d_suspended + b, 0, 4, st));
  ps->h_wait[b] = 0;
  ps->num_waiting--;
  return 0;
}

// Called by every call that changes planner state, before its first copy or launch (all of them
// run on the null stream): the device readouts still in flight on other streams finish first.
int order_after_readouts(tpamd_planner_set *ps) {
  if (!ps->read_pending) return 0;
  HIPCHK(hipStreamWaitEvent(nullptr, ps->ev_read, 0));
  ps->read_pending = false;
  return 0;
}

// A device readout on `st`: it starts after everything enqueued on the null stream so far (the
// set's changes; they also synchronise before they return, except on an error path) and after the
// previous device readout (so that ev_read, recorded after this one, covers both).
int readout_begin(tpamd_planner_set *ps, hipStream_t st) {
  HIPCHK(hipEventRecord(ps->ev_set, nullptr));
  HIPCHK(hipStreamWaitEvent(st, ps->ev_set, 0));
  if (ps->read_pending) HIPCHK(hipStreamWaitEvent(st, ps->ev_read, 0));
  return 0;
}
int readout_end(tpamd_planner_set *ps, hipStream_t st) {
  HIPCHK(hipEventRecord(ps->ev_read, st));
  ps->read_pending = true;
  return 0;
}

// ReadoutParams view of the set's resident trajectories
ReadoutParams readout_params(const tpamd_planner_set *ps) {
  const PlannerSetState &S = ps->S;
  ReadoutParams p{};
  p.B = S.B; p.D = S.D; p.tcap = ps->tcap;
  p.t_first = S.t_first; p.t_count = S.t_count;
  p.t_time = S.t_time; p.t_s = S.t_s; p.t_sd = S.t_sd; p.t_sdd = S.t_sdd;
  p.t_q = S.t_q; p.t_qd = S.t_qd; p.t_qdd = S.t_qdd;
  return p;
}

// The call-level checks of the four readouts; host_ids: every id is checked here too.
bool sample_args_ok(const tpamd_planner_set *ps, int count, const int32_t *ids, bool host_ids, const int64_t *start_ns,
                    int64_t step_ns, int num_ticks, const int32_t *status) {
  if (!ps || count < 0 || !start_ns || !status || step_ns <= 0 || num_ticks < 1) return false;
  if (!ids && count > ps->S.B) return false;
  if (ids && host_ids)
    for (int k = 0; k < count; k++)
      if (ids[k] < 0 || ids[k] >= ps->S.B) return false;
  return true;
}
bool pack_args_ok(const tpamd_planner_set *ps, int count, const int32_t *ids, bool host_ids, const int64_t *offsets,
                  int64_t capacity) {
  if (!ps || count < 0 || !offsets || capacity < 0) return false;
  if (!ids && count > ps->S.B) return false;
  if (ids && host_ids)
    for (int k = 0; k < count; k++)
      if (ids[k] < 0 || ids[k] >= ps->S.B) return false;
  return true;
}

bool stop_args_ok(const tpamd_planner_set *ps, int count, const int32_t *ids, bool host_ids, const int64_t *time_ns,
                  const double *amax, const int32_t *status, const int32_t *keep, const int64_t *offsets,
                  int64_t capacity) {
  if (!time_ns || !amax || !status || !keep) return false;
  return pack_args_ok(ps, count, ids, host_ids, offsets, capacity);
}

// Grow the stop scratch; a device stop still in flight may be using the old one.
int ensure_stop_buf(tpamd_planner_set *ps, size_t bytes) {
  if (bytes <= ps->stop_buf.bytes) return 0;
  if (ps->read_pending) HIPCHK(hipEventSynchronize(ps->ev_read));
  return ps->stop_buf.reserve(bytes);
}

// StopTrajParams view of the set's resident trajectories
StopTrajParams stop_params(const tpamd_planner_set *ps) {
  const PlannerSetState &S = ps->S;
  StopTrajParams p{};
  p.B = S.B; p.stride = ps->tcap;
  p.time = S.t_time; p.q = S.t_q; p.qd = S.t_qd; p.qdd = S.t_qdd;
  p.count = S.t_count; p.first = S.t_first;
  return p;
}

// tpamd_planner_set_upload_paths(_ragged): num_points null = every path has the config's P
int upload_paths_common(tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *num_points,
                        const double *knots, const double *cps, const double *vmax, const double *amax,
                        const double *delta, const double *iv, const int32_t *path_state) {
  if (!ps || count < 0 || !knots || !cps || !vmax || !amax || !delta || !path_state) return TPAMD_E_INVALID_ARGUMENT;
  if (ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;     // a Cartesian set's paths are IK tables
  const size_t B = ps->S.B, D = ps->S.D, P0 = ps->cfg.num_points;
  if ((size_t)count > B) return TPAMD_E_INVALID_ARGUMENT;
  // every id, state and size is checked before the first copy
  int need = 0;
  for (int k = 0; k < count; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || (path_state[k] != 1 && path_state[k] != 2)) return TPAMD_E_INVALID_ARGUMENT;
    const int P = num_points ? num_points[k] : (int)P0;
    if (P < 3) return TPAMD_E_INVALID_ARGUMENT;
    need = std::max(need, P);
  }
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  const int grc = ensure_pcap(ps, need, st);
  if (grc) return grc;
  const size_t Pc = ps->pcap, Kc = Pc + 3, n = (size_t)count;
  std::vector<double> zeros(iv ? 0 : n * D, 0.0);
  const double *ivp = iv ? iv : zeros.data();
  std::vector<int> ones(n, 1), np(n);
  for (size_t k = 0; k < n; k++) np[k] = num_points ? num_points[k] : (int)P0;
  if (!ids) {     // planners 0 .. count-1: the paths staged at the device stride, one copy per array
    std::vector<double> hk(n * Kc, 0.0), hc(n * Pc * D, 0.0);
    size_t ok = 0, oc = 0;
    for (size_t k = 0; k < n; k++) {
      const size_t P = np[k];
      std::memcpy(hk.data() + k * Kc, knots + ok, (P + 3) * 8);
      std::memcpy(hc.data() + k * Pc * D, cps + oc, P * D * 8);
      ok += P + 3; oc += P * D;
    }
    HIPCHK(hipMemcpyAsync((double *)ps->S.knots, hk.data(), n * Kc * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_cp, hc.data(), n * Pc * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_vmax, vmax, n * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync((double *)ps->S.amax, amax, n * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_delta, delta, n * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_iv, ivp, n * D * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->S.path_state, path_state, n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->S.has_path, ones.data(), n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->S.np, np.data(), n * 4, hipMemcpyHostToDevice, st));
  } else {
    size_t ok = 0, oc = 0;
    for (size_t k = 0; k < n; k++) {
      const size_t b = (size_t)ids[k], P = np[k];
      HIPCHK(hipMemcpyAsync((double *)ps->S.knots + b * Kc, knots + ok, (P + 3) * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->d_cp + b * Pc * D, cps + oc, P * D * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->d_vmax + b * D, vmax + k * D, D * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync((double *)ps->S.amax + b * D, amax + k * D, D * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->d_delta + b, delta + k, 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->d_iv + b * D, ivp + k * D, D * 8, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->S.path_state + b, path_state + k, 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->S.has_path + b, &ones[k], 4, hipMemcpyHostToDevice, st));
      HIPCHK(hipMemcpyAsync(ps->S.np + b, &np[k], 4, hipMemcpyHostToDevice, st));
      ok += P + 3; oc += P * D;
    }
  }
  HIPCHK(hipStreamSynchronize(st));
  for (size_t k = 0; k < n; k++) {
    const size_t b = ids ? (size_t)ids[k] : k;
    ps->h_np[b] = np[k];
    ps->h_stale[b] = 0;
    ps->h_has[b] = 1;
  }
  return 0;
}

// Both kinds of set. A Cartesian set keeps the (unused) spline arrays at their smallest size.
int create_planner_set(tpamd_engine *e, const tpamd_planner_set_config *cfg_in, bool cartesian, int table_capacity,
                       tpamd_planner_set **out) {
  if (!e || !cfg_in || !out) return TPAMD_E_INVALID_ARGUMENT;
  *out = nullptr;
  tpamd_planner_set_config config = *cfg_in;
  if (cartesian) config.num_points = 3;
  if (cartesian && (table_capacity < 1 || table_capacity > (1 << 28))) return TPAMD_E_INVALID_ARGUMENT;
  const tpamd_planner_set_config *cfg = &config;
  const size_t B = cfg->num_planners, D = cfg->num_dofs, N = cfg->num_samples, P = cfg->num_points;
  if (cfg->num_planners <= 0 || cfg->time_step_ns <= 0) return TPAMD_E_INVALID_ARGUMENT;
  if (D < 1 || D > 16 || N < 3 || N > 8192 || P < 3) return TPAMD_E_UNSUPPORTED;
  if (cfg->sampling_method != 0 && cfg->sampling_method != 1) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  tpamd_planner_set *ps = new (std::nothrow) tpamd_planner_set();
  if (!ps) return TPAMD_E_HIP;
  ps->e = e;
  ps->cfg = *cfg;
  ps->cap = cfg->history_capacity > 0 ? std::max<int>(cfg->history_capacity, 2 * (int)N) : 8 * (int)N;
  ps->tcap = cfg->trajectory_capacity > 0 ? cfg->trajectory_capacity : 4096;
  ps->pcap = (int)P;
  ps->h_np.assign(B, (int)P);
  ps->h_has.assign(B, 0);
  ps->h_stale.assign(B, 0);
  ps->cartesian = cartesian;
  ps->h_rows.assign(B, 0);
  ps->h_first_row.assign(B, 0);
  ps->h_wait.assign(B, 0);
  ps->h_need.assign(2 * B, 0);
  PlannerSetState &S = ps->S;
  for (int pass = 0; pass < 2; pass++) {
    Stage s(pass ? ps->fixed : nullptr);
    S.np = s.take<int>(B);
    ps->d_vmax = s.take<double>(B * D); S.amax = s.take<double>(B * D);
    ps->d_delta = s.take<double>(B); ps->d_iv = s.take<double>(B * D); ps->d_sdd0 = s.take<double>(B);
    S.path_state = s.take<int>(B); S.has_path = s.take<int>(B); S.count = s.take<int>(B);
    S.initial_plan = s.take<int>(B); S.planned_to_end = s.take<int>(B); S.target_reached = s.take<int>(B);
    S.path_horizon = s.take<double>(B); S.path_start = s.take<double>(B); S.path_start_velocity = s.take<double>(B);
    S.path_time_start = s.take<double>(B);
    S.start_time_ns = s.take<long long>(B); S.end_time_ns = s.take<long long>(B); S.final_decel_start_ns = s.take<long long>(B);
    ps->w_time = s.take<double>(B * N); ps->w_s = s.take<double>(B * N); ps->w_sd = s.take<double>(B * N);
    ps->w_sdd = s.take<double>(B * N); ps->w_q = s.take<double>(B * N * D); ps->w_qd = s.take<double>(B * N * D);
    ps->w_qdd = s.take<double>(B * N * D); ps->w_dtm = s.take<double>(B);
    ps->w_lei = s.take<int32_t>(B); ps->w_st = s.take<int32_t>(B);
    S.t_first = s.take<int>(B); S.t_count = s.take<int>(B);
    ps->d_start = s.take<long long>(B); ps->d_horizon = s.take<long long>(B); ps->d_loop_start = s.take<long long>(B);
    S.mode = s.take<int>(B); S.status = s.take<int>(B); S.active = s.take<int>(B); S.finish = s.take<int>(B);
    S.num_active = s.take<int>(2); S.resample_skip = s.take<int>(B); S.start_sec = s.take<double>(B);
    S.resample_count = s.take<int>(B);
    ps->d_windows = s.take<int>(B);
    ps->P.old_state = s.take<int>(B); ps->P.offset = s.take<int>(B); ps->P.loop = s.take<int>(B); ps->P.append = s.take<int>(B);
    ps->d_summary = s.take<PlannerSummaryDev>(B);
    ps->d_need_cap = s.take<int>(2 * B);
    ps->d_stop_in = s.take<char>(B * 12); ps->d_stop_out = s.take<char>(B * 20);
    if (cartesian) {
      ps->d_vtrans = s.take<double>(B); ps->d_vrot = s.take<double>(B); ps->d_path_end = s.take<double>(B);
      ps->d_rows = s.take<int>(B); ps->d_first = s.take<int>(B);
      ps->d_first_row = s.take<int>(B);
      ps->d_suspended = s.take<int>(B); ps->d_need = s.take<int>(2 * B);
    }
    if (!pass) {
      ps->fixed_bytes = s.off;
      if (hipMalloc(&ps->fixed, s.off) != hipSuccess) { delete ps; return TPAMD_E_HIP; }
    }
  }
  S.w_time = ps->w_time; S.w_lei = ps->w_lei;
  S.start_ns = ps->d_start; S.horizon_ns = ps->d_horizon;
  S.B = (int)B; S.N = (int)N; S.D = (int)D;
  S.method = cfg->sampling_method; S.max_iterations = cfg->max_planning_iterations;
  S.time_step_sec = (double)cfg->time_step_ns / 1e9;                    // path_timing_trajectory.cc:206-211
  S.time_step_duration_ns = (long long)llround(S.time_step_sec * 1e9);  // absl::Seconds(time_step_sec_)
  ps->hist_bytes = carve_history(nullptr, B, ps->cap, D, nullptr);
  ps->traj_bytes = carve_trajectory(nullptr, B, ps->tcap, D, nullptr);
  ps->path_bytes = carve_paths(nullptr, B, ps->pcap, D, nullptr);
  if (hipMalloc(&ps->hist, ps->hist_bytes) != hipSuccess || hipMalloc(&ps->traj, ps->traj_bytes) != hipSuccess ||
      hipMalloc(&ps->path, ps->path_bytes) != hipSuccess) {
    tpamd_planner_set_destroy(ps);
    return TPAMD_E_HIP;
  }
  carve_history((char *)ps->hist, B, ps->cap, D, ps);
  carve_trajectory((char *)ps->traj, B, ps->tcap, D, ps);
  carve_paths((char *)ps->path, B, ps->pcap, D, ps);
  if (hipMemset(ps->fixed, 0, ps->fixed_bytes) != hipSuccess || hipMemset(ps->path, 0, ps->path_bytes) != hipSuccess) {
    tpamd_planner_set_destroy(ps);
    return TPAMD_E_HIP;
  }
  if (cartesian) {
    ps->table_cap = table_capacity;
    ps->table_bytes = carve_table(nullptr, B, ps->table_cap, D, nullptr);
    if (hipMalloc(&ps->table, ps->table_bytes) != hipSuccess || hipMemset(ps->table, 0, ps->table_bytes) != hipSuccess) {
      tpamd_planner_set_destroy(ps);
      return TPAMD_E_HIP;
    }
    carve_table((char *)ps->table, B, ps->table_cap, D, ps);
  }
  // a planner without a path still has a count the sampling kernel can read (its knots are zero)
  if (hipMemcpy(S.np, ps->h_np.data(), B * 4, hipMemcpyHostToDevice) != hipSuccess) {
    tpamd_planner_set_destroy(ps);
    return TPAMD_E_HIP;
  }
  refresh_plan_params(ps);
  if (hipEventCreateWithFlags(&ps->ev_set, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ps->ev_read, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&ps->ev_wp, hipEventDisableTiming) != hipSuccess) {
    tpamd_planner_set_destroy(ps);
    return TPAMD_E_HIP;
  }
  // ResetDerived :213-227: planned_to_end_ = true (all other scalars zero)
  std::vector<int> ones(B, 1);
  if (hipMemcpy(S.planned_to_end, ones.data(), B * 4, hipMemcpyHostToDevice) != hipSuccess) {
    tpamd_planner_set_destroy(ps);
    return TPAMD_E_HIP;
  }
  *out = ps;
  return 0;
}
}  // namespace

extern "C" {

int tpamd_planner_set_create(tpamd_engine *e, const tpamd_planner_set_config *cfg, tpamd_planner_set **out) {
  return create_planner_set(e, cfg, /*cartesian=*/false, 0, out);
}

int tpamd_planner_set_create_cartesian(tpamd_engine *e, const tpamd_planner_set_config *cfg, int table_capacity,
                                       tpamd_planner_set **out) {
  return create_planner_set(e, cfg, /*cartesian=*/true, table_capacity, out);
}

void tpamd_planner_set_destroy(tpamd_planner_set *ps) {
  if (!ps) return;
  DeviceScope scope(ps->e->device);
  if (ps->read_pending) (void)hipEventSynchronize(ps->ev_read);   // a device readout may still read the set
  if (ps->ev_set) (void)hipEventDestroy(ps->ev_set);
  if (ps->ev_read) (void)hipEventDestroy(ps->ev_read);
  ps->rd_in.release();
  ps->rd_out.release();
  ps->stop_buf.release();
  ps->check_buf.release();
  ps->state_buf.release();
  ps->state_items.release();
  if (ps->fixed) (void)hipFree(ps->fixed);
  if (ps->hist) (void)hipFree(ps->hist);
  if (ps->traj) (void)hipFree(ps->traj);
  if (ps->path) (void)hipFree(ps->path);
  if (ps->table) (void)hipFree(ps->table);
  ps->sw_buf.release();
  ps->wp_buf.release();
  if (ps->wp_pin) (void)hipHostFree(ps->wp_pin);
  if (ps->ev_wp) (void)hipEventDestroy(ps->ev_wp);
  delete ps;
}

size_t tpamd_planner_set_device_bytes(const tpamd_planner_set *ps) {
  return ps ? ps->fixed_bytes + ps->hist_bytes + ps->traj_bytes + ps->path_bytes + ps->table_bytes + ps->sw_buf.bytes +
                   ps->rd_in.bytes + ps->rd_out.bytes + ps->stop_buf.bytes + ps->wp_buf.bytes + ps->check_buf.bytes +
                   ps->state_buf.bytes + ps->state_items.bytes
            : 0;
}

void tpamd_planner_set_last_plan_bytes(const tpamd_planner_set *ps, size_t *h2d, size_t *d2h) {
  if (h2d) *h2d = ps ? ps->last_h2d : 0;
  if (d2h) *d2h = ps ? ps->last_d2h : 0;
}

int tpamd_planner_set_upload_paths(tpamd_planner_set *ps, int count, const int32_t *ids, const double *knots,
                                   const double *cps, const double *vmax, const double *amax, const double *delta,
                                   const double *iv, const int32_t *path_state) {
  return upload_paths_common(ps, count, ids, nullptr, knots, cps, vmax, amax, delta, iv, path_state);
}

int tpamd_planner_set_upload_paths_ragged(tpamd_planner_set *ps, int count, const int32_t *ids,
                                          const int32_t *num_points, const double *knots, const double *cps,
                                          const double *vmax, const double *amax, const double *delta,
                                          const double *iv, const int32_t *path_state) {
  if (!num_points) return TPAMD_E_INVALID_ARGUMENT;
  return upload_paths_common(ps, count, ids, num_points, knots, cps, vmax, amax, delta, iv, path_state);
}

int tpamd_planner_set_download_path(tpamd_planner_set *ps, int planner, int32_t *num_points, double *knots,
                                    double *cps, int capacity) {
  if (!ps || !num_points || planner < 0 || planner >= ps->S.B || ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_path_counts(ps, planner)) return rc;
  const int P = ps->h_has[planner] ? ps->h_np[planner] : 0;
  *num_points = P;
  if (P == 0 || (!knots && !cps)) return 0;
  if (P > capacity) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;      // a device set_waypoints may still be writing
  const size_t D = ps->S.D, b = planner;
  if (knots) HIPCHK(hipMemcpy(knots, ps->S.knots + b * ps->S.K, (size_t)(P + 3) * 8, hipMemcpyDeviceToHost));
  if (cps) HIPCHK(hipMemcpy(cps, ps->d_cp + b * ps->pcap * D, (size_t)P * D * 8, hipMemcpyDeviceToHost));
  return 0;
}

int tpamd_planner_set_reset(tpamd_planner_set *ps, int count, const int32_t *ids) {
  if (!ps || count < 0) return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = ps->S.B;
  TPAMD_ON_DEVICE(ps->e);
  PlannerSetState &S = ps->S;
  const int one = 1;
  const int n = ids ? count : (int)B;
  for (int k = 0; k < n; k++)
    if (ids && (ids[k] < 0 || (size_t)ids[k] >= B)) return TPAMD_E_INVALID_ARGUMENT;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  for (int k = 0; k < n; k++) {
    const size_t b = ids ? (size_t)ids[k] : (size_t)k;
    for (int *a : {S.path_state, S.has_path, S.count, S.initial_plan, S.target_reached, S.t_first, S.t_count})
      HIPCHK(hipMemsetAsync(a + b, 0, 4, nullptr));
    for (double *a : {S.path_horizon, S.path_start, S.path_start_velocity, S.path_time_start})
      HIPCHK(hipMemsetAsync(a + b, 0, 8, nullptr));
    for (long long *a : {S.start_time_ns, S.end_time_ns, S.final_decel_start_ns})
      HIPCHK(hipMemsetAsync(a + b, 0, 8, nullptr));
    HIPCHK(hipMemcpyAsync(S.planned_to_end + b, &one, 4, hipMemcpyHostToDevice, nullptr));
    if (ps->cartesian) HIPCHK(hipMemsetAsync(ps->d_first_row + b, 0, 4, nullptr));
    if (drop_suspension(ps, (int)b, nullptr)) return TPAMD_E_HIP;
  }
  HIPCHK(hipStreamSynchronize(nullptr));
  for (int k = 0; k < n; k++) {
    ps->h_has[ids ? (size_t)ids[k] : (size_t)k] = 0;
    ps->h_first_row[ids ? (size_t)ids[k] : (size_t)k] = 0;
  }
  return 0;
}

// Checking (tpamd_planner_set_set_checking; nothing of this is enqueued with checking off): a Plan
// call that starts afresh clears the records; every window iteration checks, behind the sweep, the
// windows it solved. P: the largest path of the set, as the solve takes it.
static void clear_window_checks(tpamd_planner_set *ps, hipStream_t st) {
  const int B = ps->S.B;
  hipLaunchKernelGGL(k_pset_check_clear, dim3((unsigned)((B + 127) / 128)), dim3(128), 0, st, B, ps->d_check);
}
static void check_windows(tpamd_planner_set *ps, int P, hipStream_t st) {
  const PlannerSetState &S = ps->S;
  const double safety = ps->cfg.constraint_safety;
  if (ps->cartesian)
    hipLaunchKernelGGL(k_pset_check_cartesian, dim3((unsigned)S.B), dim3(kCheckThreads), 0, st, ps->P, safety, ps->d_tq,
                       ps->d_tJ, ps->table_cap, ps->d_vmax, S.amax, ps->d_vtrans, ps->d_vrot, ps->d_sd2, ps->d_check);
  else
    hipLaunchKernelGGL(k_pset_check_joint, dim3((unsigned)S.B), dim3(kCheckThreads), check_joint_lds(P, S.D), st, ps->P,
                       P, ps->pcap, safety, ps->d_cp, ps->d_vmax, S.amax, ps->d_sd2, ps->d_check);
}

// Plan for every planner of a set. kPlanFresh is tpamd_planner_set_plan; kPlanStreaming is the same
// with the streaming arrays set (a planner whose window is not resident waits); kPlanResume
// re-enters the window loop for the planners that waited (k_pset_resume in place of the prologue,
// nothing goes up). A fresh or streaming Plan drops every suspension left from an earlier call.
enum PlanKind { kPlanFresh, kPlanStreaming, kPlanResume };
static int planner_set_plan_run(tpamd_planner_set *ps, PlanKind kind, const int64_t *start_ns, const int64_t *horizon_ns,
                                tpamd_planner_summary *summary, int32_t *need_first, int32_t *need_count,
                                int32_t *num_waiting) {
  static_assert(sizeof(tpamd_planner_summary) == sizeof(PlannerSummaryDev), "summary layouts must agree");
  tpamd_engine *e = ps->e;
  TPAMD_ON_DEVICE(e);
  PlannerSetState &S = ps->S;
  // the sampling kernel's LDS layout holds the largest path in use; each planner reads its own
  const size_t B = S.B, N = S.N, D = S.D, P = largest_points(ps);
  hipStream_t st = nullptr;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  ps->last_h2d = ps->last_d2h = 0;
  const unsigned gb = (unsigned)((B + 127) / 128);
  ps->streaming = kind != kPlanFresh;
  refresh_plan_params(ps);
  if (kind == kPlanResume) {
    HIPCHK(hipMemsetAsync(S.num_active, 0, 8, st));
    hipLaunchKernelGGL(k_pset_resume, dim3(gb), dim3(128), 0, st, S, ps->P);
  } else {
    if (ps->num_waiting || kind == kPlanStreaming) {
      HIPCHK(hipMemsetAsync(ps->d_suspended, 0, B * 4, st));
      HIPCHK(hipMemsetAsync(ps->d_need, 0, 2 * B * 4, st));
      std::fill(ps->h_wait.begin(), ps->h_wait.end(), 0);
      ps->num_waiting = 0;
    }
    HIPCHK(hipMemcpyAsync(ps->d_start, start_ns, B * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_horizon, horizon_ns, B * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ps->d_loop_start, start_ns, B * 8, hipMemcpyHostToDevice, st));   // :630
    ps->last_h2d += 3 * B * 8;
    if (ps->checking) clear_window_checks(ps, st);
    for (int *z : {ps->P.old_state, ps->P.offset, ps->P.loop, ps->P.append, ps->d_windows})
      HIPCHK(hipMemsetAsync(z, 0, B * 4, st));
    HIPCHK(hipMemsetAsync(S.num_active, 0, 8, st));
    hipLaunchKernelGGL(k_pset_prologue, dim3(gb), dim3(128), 0, st, S);
  }
  hipLaunchKernelGGL(k_pset_check_capacity, dim3(gb), dim3(128), 0, st, S);
  int na[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(na, S.num_active, 8, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  ps->last_d2h += 8;
  tpamd_joint_batch bt{(int)B, (int)D, (int)N, (int)P, 0, 0, ps->cfg.constraint_safety};
  for (int guard = 0; na[0] > 0; guard++) {
    if (guard > 100000) return TPAMD_E_UNSUPPORTED;
    if (na[1]) {          // a looping planner's history is full: double the histories, then go on
      const int rc = grow_rows(ps, /*history=*/true, 2 * ps->cap, st);
      if (rc) return rc;
    }
    tpamd_joint_inputs din{S.knots, ps->d_cp, ps->d_vmax, S.amax, S.path_start, ps->d_delta, S.path_start_velocity,
                           ps->d_sdd0, S.path_time_start, nullptr};
    tpamd_path_outputs dout{ps->w_time, ps->w_s, ps->w_sd, ps->w_sdd, ps->w_q, ps->w_qd, ps->w_qdd, ps->w_lei,
                            ps->w_dtm, ps->w_st, ps->checking ? ps->d_sd2 : nullptr};
    hipLaunchKernelGGL(k_plan_begin, dim3(gb), dim3(128), 0, st, ps->P, e->ws);
    int rc;
    if (ps->cartesian) {
      // the windows are read out of the resident IK tables, each from its planner's row first[b]
      tpamd_cartesian_batch cb{(int)B, (int)D, (int)N, 0, ps->cfg.constraint_safety};
      tpamd_cartesian_inputs cin{ps->d_tq, ps->d_tJ, ps->d_vmax, S.amax, ps->d_vtrans, ps->d_vrot, S.path_start,
                                 ps->d_delta, S.path_start_velocity, ps->d_sdd0, S.path_time_start};
      rc = solve_cartesian(e, &cb, &cin, &dout, st, &ps->P, ps->table_cap);
    } else {
      rc = solve_joint(e, &bt, &din, &dout, st, &ps->P);
    }
    if (rc) return rc;
    if (ps->checking) check_windows(ps, (int)P, st);
    HIPCHK(hipMemsetAsync(S.num_active, 0, 8, st));
    hipLaunchKernelGGL(k_plan_end, dim3(gb), dim3(128), 0, st, ps->P);
    hipLaunchKernelGGL(k_plan_append, dim3((unsigned)((N + 127) / 128), (unsigned)B), dim3(128), 0, st, ps->P);
    hipLaunchKernelGGL(k_pset_check_capacity, dim3(gb), dim3(128), 0, st, S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(na, S.num_active, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ps->last_d2h += 8;
  }
  // ResampleTrajectory(start) :660 and the bookkeeping of :662-684; repeated with larger trajectory
  // buffers if a planner's resampled trajectory does not fit
  for (int attempt = 0; attempt < 8; attempt++) {
    hipLaunchKernelGGL(k_pset_before_resample, dim3(gb), dim3(128), 0, st, S);
    ResampleParams rp;
    rp.B = (int)B; rp.N = ps->cap; rp.D = (int)D; rp.max_out = ps->tcap;
    rp.time = S.h_time; rp.s = S.h_s; rp.sd = S.h_sd; rp.sdd = S.h_sdd; rp.q = S.h_q; rp.qd = S.h_qd; rp.qdd = S.h_qdd;
    rp.amax = S.amax; rp.start_sec = S.start_sec; rp.status = S.resample_skip; rp.ns = S.count;
    rp.ot = S.t_time; rp.os = S.t_s; rp.osd = S.t_sd; rp.osdd = S.t_sdd; rp.oq = S.t_q; rp.oqd = S.t_qd; rp.oqdd = S.t_qdd;
    rp.count = S.resample_count;
    if (S.method == 0) {
      rp.time_step = S.time_step_sec;
      hipLaunchKernelGGL(k_resample, dim3((ps->tcap + 255) / 256, (unsigned)B), dim3(256), 0, st, rp);
    } else {
      rp.time_step = 0.95 * S.time_step_sec;            // GetMinTimeDeltaToKeep :893-900
      hipLaunchKernelGGL(k_resample_skip, dim3((unsigned)B), dim3(64), 0, st, rp);
    }
    HIPCHK(hipMemsetAsync(S.num_active, 0, 8, st));
    hipLaunchKernelGGL(k_pset_epilogue, dim3(gb), dim3(128), 0, st, S);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(na, S.num_active, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    ps->last_d2h += 8;
    if (na[1] <= ps->tcap) break;
    const int rc = grow_rows(ps, /*history=*/false, std::max(2 * ps->tcap, na[1] + 64), st);
    if (rc) return rc;
  }
  hipLaunchKernelGGL(k_pset_summary, dim3(gb), dim3(128), 0, st, S, ps->d_windows, ps->d_summary);
  HIPCHK(hipGetLastError());
  if (summary) {
    HIPCHK(hipMemcpyAsync(summary, ps->d_summary, B * sizeof(PlannerSummaryDev), hipMemcpyDeviceToHost, st));
    ps->last_d2h += B * sizeof(PlannerSummaryDev);
  }
  if (kind != kPlanFresh) {
    HIPCHK(hipMemcpyAsync(ps->h_need.data(), ps->d_need, 2 * B * 4, hipMemcpyDeviceToHost, st));
    ps->last_d2h += 2 * B * 4;
  }
  HIPCHK(hipStreamSynchronize(st));
  if (kind != kPlanFresh) {
    ps->num_waiting = 0;
    for (size_t b = 0; b < B; b++) {
      ps->h_wait[b] = ps->h_need[B + b] > 0;
      ps->num_waiting += ps->h_wait[b];
    }
    if (need_first) std::memcpy(need_first, ps->h_need.data(), B * 4);
    if (need_count) std::memcpy(need_count, ps->h_need.data() + B, B * 4);
    if (num_waiting) *num_waiting = ps->num_waiting;
  }
  return 0;
}

int tpamd_planner_set_plan(tpamd_planner_set *ps, const int64_t *start_ns, const int64_t *horizon_ns,
                           tpamd_planner_summary *summary) {
  if (!ps || !start_ns || !horizon_ns) return TPAMD_E_INVALID_ARGUMENT;
  return planner_set_plan_run(ps, kPlanFresh, start_ns, horizon_ns, summary, nullptr, nullptr, nullptr);
}

int tpamd_planner_set_plan_streaming(tpamd_planner_set *ps, const int64_t *start_ns, const int64_t *horizon_ns,
                                     tpamd_planner_summary *summary, int32_t *need_first, int32_t *need_count,
                                     int32_t *num_waiting) {
  if (!ps || !ps->cartesian || !start_ns || !horizon_ns) return TPAMD_E_INVALID_ARGUMENT;
  return planner_set_plan_run(ps, kPlanStreaming, start_ns, horizon_ns, summary, need_first, need_count, num_waiting);
}

int tpamd_planner_set_plan_resume(tpamd_planner_set *ps, tpamd_planner_summary *summary, int32_t *need_first,
                                  int32_t *need_count, int32_t *num_waiting) {
  if (!ps || !ps->cartesian || ps->num_waiting == 0) return TPAMD_E_INVALID_ARGUMENT;
  return planner_set_plan_run(ps, kPlanResume, nullptr, nullptr, summary, need_first, need_count, num_waiting);
}

int tpamd_planner_set_capacity(const tpamd_planner_set *ps, int32_t *history, int32_t *trajectory) {
  if (!ps) return TPAMD_E_INVALID_ARGUMENT;
  if (history) *history = ps->cap;
  if (trajectory) *trajectory = ps->tcap;
  return 0;
}

int tpamd_planner_set_reserve(tpamd_planner_set *ps, int history_capacity, int trajectory_capacity) {
  if (!ps) return TPAMD_E_INVALID_ARGUMENT;
  if (history_capacity > (1 << 28) || trajectory_capacity > (1 << 28)) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(ps->e);
  if (history_capacity > ps->cap || trajectory_capacity > ps->tcap) {
    // the copies run on the null stream, after the device calls in flight; grow_rows synchronises
    if (order_after_readouts(ps)) return TPAMD_E_HIP;
    if (history_capacity > ps->cap)
      if (int rc = grow_rows(ps, /*history=*/true, history_capacity, nullptr)) return rc;
    if (trajectory_capacity > ps->tcap)
      if (int rc = grow_rows(ps, /*history=*/false, trajectory_capacity, nullptr)) return rc;
  }
  // the engine's workspace for this set's windows: an enqueued-only Plan then allocates nothing
  const int C = ps->cartesian ? 2 * ps->S.D + 2 : 2 * ps->S.D;
  if (carve_workspace(nullptr, ps->S.B, ps->S.N, C, nullptr) > ps->e->ws_buf.bytes) {
    HIPCHK(hipDeviceSynchronize());         // solves in flight use the workspace that is replaced
    if (int rc = ensure_workspace(ps->e, ps->S.B, ps->S.N, C)) return rc;
  }
  return 0;
}

// Plan, enqueued only (include/tpamd.h). The window loop of planner_set_plan_run with the host out
// of it: max_windows iterations, each gated per planner on the device (tpamd_planner_set.h).
int tpamd_planner_set_plan_device(tpamd_planner_set *ps, const int64_t *start_ns, const int64_t *horizon_ns,
                                  int max_windows, tpamd_planner_summary *summary, tpamd_plan_device_info *info,
                                  void *hip_stream) {
  static_assert(sizeof(tpamd_plan_device_info) == 32 && sizeof(PlanDeviceInfoDev) == 32, "info layouts must agree");
  if (!ps || !start_ns || !horizon_ns || max_windows < 1) return TPAMD_E_INVALID_ARGUMENT;
  tpamd_engine *e = ps->e;
  TPAMD_ON_DEVICE(e);
  PlannerSetState &S = ps->S;
  const size_t B = S.B, N = S.N, D = S.D, P = largest_points(ps);
  hipStream_t st = (hipStream_t)hip_stream;
  if (!e->ev_async) HIPCHK(hipEventCreateWithFlags(&e->ev_async, hipEventDisableTiming));
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  ps->last_h2d = ps->last_d2h = 0;
  const unsigned gb = (unsigned)((B + 127) / 128);
  ps->streaming = false;
  refresh_plan_params(ps);
  ps->P.max_iterations = std::min(ps->cfg.max_planning_iterations, max_windows - 1);
  if (ps->num_waiting) {        // suspensions of an earlier streaming Plan are dropped
    HIPCHK(hipMemsetAsync(ps->d_suspended, 0, B * 4, st));
    HIPCHK(hipMemsetAsync(ps->d_need, 0, 2 * B * 4, st));
    std::fill(ps->h_wait.begin(), ps->h_wait.end(), 0);
    ps->num_waiting = 0;
  }
  if (ps->checking) clear_window_checks(ps, st);
  HIPCHK(hipMemsetAsync(S.num_active, 0, 8, st));
  hipLaunchKernelGGL(k_pset_prologue_step, dim3(gb), dim3(128), 0, st, S, ps->P, (const long long *)start_ns,
                     (const long long *)horizon_ns, ps->d_start, ps->d_horizon, ps->d_need_cap);
  tpamd_joint_batch bt{(int)B, (int)D, (int)N, (int)P, 0, 0, ps->cfg.constraint_safety};
  tpamd_joint_inputs din{S.knots, ps->d_cp, ps->d_vmax, S.amax, S.path_start, ps->d_delta, S.path_start_velocity,
                         ps->d_sdd0, S.path_time_start, nullptr};
  tpamd_path_outputs dout{ps->w_time, ps->w_s, ps->w_sd, ps->w_sdd, ps->w_q, ps->w_qd, ps->w_qdd, ps->w_lei,
                          ps->w_dtm, ps->w_st, ps->checking ? ps->d_sd2 : nullptr};
  int rc = 0;
  for (int w = 0; w < max_windows && !rc; w++) {
    if (ps->cartesian) {
      tpamd_cartesian_batch cb{(int)B, (int)D, (int)N, 0, ps->cfg.constraint_safety};
      tpamd_cartesian_inputs cin{ps->d_tq, ps->d_tJ, ps->d_vmax, S.amax, ps->d_vtrans, ps->d_vrot, S.path_start,
                                 ps->d_delta, S.path_start_velocity, ps->d_sdd0, S.path_time_start};
      rc = solve_cartesian(e, &cb, &cin, &dout, st, &ps->P, ps->table_cap);
    } else {
      rc = solve_joint(e, &bt, &din, &dout, st, &ps->P);
    }
    if (rc) break;
    if (ps->checking) check_windows(ps, (int)P, st);
    hipLaunchKernelGGL(k_plan_append_early, dim3((unsigned)((N + 127) / 128), (unsigned)B), dim3(128), 0, st, ps->P);
    if (w + 1 < max_windows) hipLaunchKernelGGL(k_pset_step, dim3(gb), dim3(128), 0, st, S, ps->P, ps->d_need_cap);
    else hipLaunchKernelGGL(k_pset_last_step, dim3(gb), dim3(128), 0, st, S, ps->P);
  }
  if (!rc) {
    ResampleParams rp;
    rp.B = (int)B; rp.N = ps->cap; rp.D = (int)D; rp.max_out = ps->tcap;
    rp.time = S.h_time; rp.s = S.h_s; rp.sd = S.h_sd; rp.sdd = S.h_sdd; rp.q = S.h_q; rp.qd = S.h_qd; rp.qdd = S.h_qdd;
    rp.amax = S.amax; rp.start_sec = S.start_sec; rp.status = S.resample_skip; rp.ns = S.count;
    rp.ot = S.t_time; rp.os = S.t_s; rp.osd = S.t_sd; rp.osdd = S.t_sdd; rp.oq = S.t_q; rp.oqd = S.t_qd; rp.oqdd = S.t_qdd;
    rp.count = S.resample_count;
    if (S.method == 0) {
      rp.time_step = S.time_step_sec;
      hipLaunchKernelGGL(k_resample, dim3((ps->tcap + 255) / 256, (unsigned)B), dim3(256), 0, st, rp);
    } else {
      rp.time_step = 0.95 * S.time_step_sec;            // GetMinTimeDeltaToKeep :893-900
      hipLaunchKernelGGL(k_resample_skip, dim3((unsigned)B), dim3(64), 0, st, rp);
    }
    hipLaunchKernelGGL(k_pset_epilogue_device, dim3(gb), dim3(128), 0, st, S, ps->d_need_cap);
    hipLaunchKernelGGL(k_pset_finish_device, dim3(1), dim3(kFinishThreads), 0, st, S, ps->d_windows, ps->d_need_cap,
                       ps->d_summary, (PlannerSummaryDev *)summary, (PlanDeviceInfoDev *)info);
    if (hipGetLastError() != hipSuccess) rc = TPAMD_E_HIP;
  }
  // whatever was enqueued (an error path included) is ordered in front of the set's and the
  // engine's later work: the event after it, and the null stream behind the event
  if (hipEventRecord(e->ev_async, st) != hipSuccess) return TPAMD_E_HIP;
  e->async_pending = true;
  if (readout_end(ps, st)) return TPAMD_E_HIP;
  HIPCHK(hipStreamWaitEvent(nullptr, ps->ev_read, 0));
  return rc;
}

int tpamd_planner_set_set_checking(tpamd_planner_set *ps, int on) {
  static_assert(sizeof(tpamd_planner_check) == sizeof(PlannerCheckDev), "record layouts must agree");
  if (!ps) return TPAMD_E_INVALID_ARGUMENT;
  if (!on || ps->checking) {
    ps->checking = on != 0;     // (switched off: the buffer stays; switched on again: the records start empty)
    return 0;
  }
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  const size_t B = ps->S.B, N = ps->S.N;
  if (int rc = ps->check_buf.reserve(B * N * 8 + B * sizeof(PlannerCheckDev))) return rc;
  ps->d_sd2 = (double *)ps->check_buf.p;
  ps->d_check = (PlannerCheckDev *)(ps->d_sd2 + B * N);
  clear_window_checks(ps, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(nullptr));
  ps->checking = true;
  return 0;
}

int tpamd_planner_set_checking(const tpamd_planner_set *ps) { return ps && ps->checking; }

int tpamd_planner_set_check_results(tpamd_planner_set *ps, int count, const int32_t *ids, tpamd_planner_check *out) {
  if (!ps || !out || count < 0 || count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (ids) {
    std::vector<char> seen(ps->S.B, 0);
    for (int k = 0; k < count; k++) {
      if (ids[k] < 0 || ids[k] >= ps->S.B || seen[ids[k]]) return TPAMD_E_INVALID_ARGUMENT;
      seen[ids[k]] = 1;
    }
  }
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const int32_t *d_ids = nullptr;
  PlannerCheckDev *d_out = nullptr;
  HostStage in(/*packed=*/true, /*tight=*/true), res;
  in.up(&d_ids, ids, (size_t)count);
  res.down(&d_out, (PlannerCheckDev *)out, (size_t)count);
  if (in.upload(ps->rd_in, st) || res.upload(ps->rd_out, st)) return TPAMD_E_HIP;
  hipLaunchKernelGGL(k_pset_check_results, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, st, ps->S.B, count, d_ids,
                     ps->checking ? ps->d_check : nullptr, d_out);
  HIPCHK(hipGetLastError());
  return res.download(st);
}

int tpamd_planner_set_check_results_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                           tpamd_planner_check *out, void *hip_stream) {
  if (!ps || !out || count < 0 || count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  hipLaunchKernelGGL(k_pset_check_results, dim3((unsigned)((count + 127) / 128)), dim3(128), 0, st, ps->S.B, count, ids,
                     ps->checking ? ps->d_check : nullptr, (PlannerCheckDev *)out);
  HIPCHK(hipGetLastError());
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

int tpamd_planner_set_download_trajectory(tpamd_planner_set *ps, int planner, int first, int count, double *time,
                                          double *s, double *sd, double *sdd, double *q, double *qd, double *qdd) {
  if (!ps || planner < 0 || planner >= ps->S.B || first < 0 || count < 0) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  const PlannerSetState &S = ps->S;
  int fc[2];
  HIPCHK(hipMemcpy(&fc[0], S.t_first + planner, 4, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(&fc[1], S.t_count + planner, 4, hipMemcpyDeviceToHost));
  if (first + count > fc[1]) return TPAMD_E_INVALID_ARGUMENT;
  const size_t o = (size_t)planner * ps->tcap + fc[0] + first, D = S.D, n = count;
  if (time) HIPCHK(hipMemcpy(time, S.t_time + o, n * 8, hipMemcpyDeviceToHost));
  if (s) HIPCHK(hipMemcpy(s, S.t_s + o, n * 8, hipMemcpyDeviceToHost));
  if (sd) HIPCHK(hipMemcpy(sd, S.t_sd + o, n * 8, hipMemcpyDeviceToHost));
  if (sdd) HIPCHK(hipMemcpy(sdd, S.t_sdd + o, n * 8, hipMemcpyDeviceToHost));
  if (q) HIPCHK(hipMemcpy(q, S.t_q + o * D, n * D * 8, hipMemcpyDeviceToHost));
  if (qd) HIPCHK(hipMemcpy(qd, S.t_qd + o * D, n * D * 8, hipMemcpyDeviceToHost));
  if (qdd) HIPCHK(hipMemcpy(qdd, S.t_qdd + o * D, n * D * 8, hipMemcpyDeviceToHost));
  return 0;
}

int tpamd_planner_set_stop_parameters(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                                      double *stop_parameter, double *duration, int32_t *status) {
  if (!ps || count < 0 || !time_ns || !stop_parameter || !status) return TPAMD_E_INVALID_ARGUMENT;
  const PlannerSetState &S = ps->S;
  if (count > S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (ids)
    for (int k = 0; k < count; k++)
      if (ids[k] < 0 || ids[k] >= S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  const size_t n = (size_t)count;
  hipStream_t st = nullptr;
  // one copy up ([time_ns][ids]), one launch, one copy down ([s][duration][status]), unpadded
  FastestStopParams p{};
  HostStage in(/*packed=*/true, /*tight=*/true, /*align=*/1), out(/*packed=*/true, /*tight=*/true, /*align=*/1);
  in.up(&p.query_ns, time_ns, n);
  in.up(&p.ids, ids, n);
  out.down(&p.stop_s, stop_parameter, n);
  out.down_or_scratch(&p.duration, duration, n);
  out.down(&p.status, status, n);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;      // the limits of a device set_waypoints
  if (in.upload(ps->d_stop_in, st) || out.upload(ps->d_stop_out, st)) return TPAMD_E_HIP;
  p.Q = count; p.stride = ps->tcap;
  p.time = S.t_time; p.s = S.t_s; p.qd = S.t_qd; p.qdd = S.t_qdd;
  p.count = S.t_count; p.first = S.t_first; p.initial_plan = S.initial_plan;
  p.amax = S.amax;
  if (!launch_fastest_stop(S.D, p, st)) return TPAMD_E_UNSUPPORTED;
  HIPCHK(hipGetLastError());
  return out.download(st);
}

}  // extern "C"

extern "C" {

int tpamd_planner_set_switch_paths_rounded(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                                           const double *keep_path_until, const int32_t *waypoint_offsets,
                                           const double *waypoints, double rounding, double *stop_parameter,
                                           int32_t *num_points, int32_t *status) {
  if (!ps || count < 0 || !time_ns || !waypoint_offsets || !waypoints || !stop_parameter || !num_points || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;     // SwitchToWaypointPath edits a joint spline
  const PlannerSetState &S = ps->S;
  const size_t B = S.B, D = S.D;
  if ((size_t)count > B) return TPAMD_E_INVALID_ARGUMENT;
  // every id (in range, listed once) and the waypoint offsets are checked before anything changes
  std::vector<char> seen(B, 0);
  std::vector<int32_t> id(count);
  for (int k = 0; k < count; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || seen[b]) return TPAMD_E_INVALID_ARGUMENT;
    seen[b] = 1;
    id[k] = (int32_t)b;
  }
  if (waypoint_offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  for (int k = 0; k < count; k++)
    if (waypoint_offsets[k + 1] < waypoint_offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  // the new P of every listed planner is bounded by its current P and W; P_cap grows first
  int need = 0, wmax = 0;
  for (int k = 0; k < count; k++) {
    const int W = waypoint_offsets[k + 1] - waypoint_offsets[k];
    need = std::max(need, sw_points_bound(ps->h_np[id[k]], W));
    wmax = std::max(wmax, W);
  }
  int rc = ensure_pcap(ps, need, st);
  if (rc) return rc;
  const size_t n = (size_t)count, rows = (size_t)waypoint_offsets[count];
  const int scr_points = need, scr_work = (wmax + 3) * (int)D;
  const size_t per_query = (size_t)scr_points + 3 + (size_t)scr_points * D + scr_work;
  // device buffer: in [time_ns][keep][ids][offsets][waypoints] | out [stop][num_points][status] |
  // stop status | scratch
  SwitchParams p{};
  HostStage s(/*packed=*/true);
  s.up(&p.time_ns, time_ns, n);
  s.up(&p.keep, keep_path_until, n);
  s.up(&p.ids, id.data(), n);
  s.up(&p.offsets, waypoint_offsets, n + 1);
  s.up(&p.wps, waypoints, rows * D);
  s.down(&p.stop_out, stop_parameter, n);
  s.down(&p.np_out, num_points, n);
  s.down(&p.status_out, status, n);
  s.scratch(&p.stop_status, n);
  s.scratch(&p.scr, n * per_query);
  rc = s.upload(ps->sw_buf, st);
  if (rc) return rc;
  p.stop_in = p.stop_out;
  if (!keep_path_until) {       // GetPathStopParameter(time) on the resident trajectories
    FastestStopParams f{};
    f.Q = count; f.stride = ps->tcap;
    f.time = S.t_time; f.s = S.t_s; f.qd = S.t_qd; f.qdd = S.t_qdd;
    f.count = S.t_count; f.first = S.t_first; f.initial_plan = S.initial_plan;
    f.ids = p.ids;
    f.amax = S.amax; f.query_ns = p.time_ns;
    f.stop_s = p.stop_out; f.status = (int *)p.stop_status;
    if (!launch_fastest_stop((int)D, f, st)) return TPAMD_E_UNSUPPORTED;
  }
  p.Q = count; p.D = (int)D; p.K = S.K; p.pcap = ps->pcap; p.tcap = ps->tcap;
  p.scr_points = scr_points; p.scr_work = scr_work; p.radius = rounding;
  p.knots = (double *)S.knots; p.cps = ps->d_cp; p.iv = ps->d_iv; p.np = S.np; p.path_state = S.path_state;
  p.has_path = S.has_path; p.initial_plan = S.initial_plan; p.t_first = S.t_first; p.t_count = S.t_count;
  p.t_time = S.t_time; p.t_qd = S.t_qd;
  hipLaunchKernelGGL(k_pset_switch, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, p);
  HIPCHK(hipGetLastError());
  rc = s.download(st);
  if (rc) return rc;
  for (size_t k = 0; k < n; k++)
    if (status[k] == TPAMD_PLAN_OK) {
      ps->h_np[id[k]] = num_points[k];
      ps->h_stale[id[k]] = 0;
    }
  return 0;
}

int tpamd_planner_set_switch_paths(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                                   const double *keep_path_until, const int32_t *waypoint_offsets,
                                   const double *waypoints, double *stop_parameter, int32_t *num_points,
                                   int32_t *status) {
  return tpamd_planner_set_switch_paths_rounded(ps, count, ids, time_ns, keep_path_until, waypoint_offsets, waypoints,
                                                kSwitchRounding, stop_parameter, num_points, status);
}

}  // extern "C"

// ---------------------------------------------------------------- planner-set waypoint fits
namespace {

// The call-level checks of the two set_waypoints entries (before anything changes): the arrays,
// every id in range and listed once (ids NULL: 0..count-1), offsets from 0 and non-decreasing.
// Fills id[count] and *need, the largest control-point count of a fit.
int waypoint_args(const tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *offsets,
                  const double *waypoints, const double *vmax, const double *amax, const double *delta,
                  const int32_t *status, std::vector<int32_t> *id, int *need) {
  if (!ps || count < 0 || !offsets || !vmax || !amax || !delta || !status) return TPAMD_E_INVALID_ARGUMENT;
  if (ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;     // the fit makes a joint spline
  const size_t B = ps->S.B;
  if ((size_t)count > B || offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<char> seen(B, 0);
  id->resize(count);
  long long most = 0;
  for (int k = 0; k < count; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || seen[b]) return TPAMD_E_INVALID_ARGUMENT;
    seen[b] = 1;
    (*id)[k] = (int32_t)b;
    if (offsets[k + 1] < offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
    const long long W = (long long)offsets[k + 1] - offsets[k];
    if (W > 0) most = std::max(most, W == 1 ? 4 : 3 * W - 2);
  }
  if (offsets[count] > 0 && !waypoints) return TPAMD_E_INVALID_ARGUMENT;
  if (most > (1 << 24)) return TPAMD_E_UNSUPPORTED;
  *need = (int)most;
  return 0;
}

// Grow the set_waypoints device buffer (contents are not kept); a device call in flight may use it.
int ensure_wp_buf(tpamd_planner_set *ps, size_t bytes) {
  if (bytes <= ps->wp_buf.bytes) return 0;
  if (ps->read_pending) HIPCHK(hipEventSynchronize(ps->ev_read));
  return ps->wp_buf.reserve(bytes);
}

// The _device entries that change paths (set_waypoints_device, upload_ik_tables_device): ids[n] and
// offsets[n + 1] go up through pinned staging on `st`, into wp_buf at [0, n) and at the next
// 256-byte boundary. The previous call's copy out of the staging has to be done first; the copy is
// ordered like a device readout (readout_begin), and ev_wp guards the staging against the next
// call. The caller ends with readout_end(ps, st).
// `extra` (may be null): n more ints behind the offsets (an append's destination rows).
int stage_ids_and_offsets(tpamd_planner_set *ps, const std::vector<int32_t> &id, const int32_t *offsets, hipStream_t st,
                          const int **d_ids, const int **d_offsets, const std::vector<int32_t> *extra = nullptr,
                          const int **d_extra = nullptr) {
  const size_t n = id.size(), bytes = align_up(n * 4, 256) + (n + 1) * 4 + (extra ? n * 4 : 0);
  if (ps->wp_pin_busy) {
    HIPCHK(hipEventSynchronize(ps->ev_wp));
    ps->wp_pin_busy = false;
  }
  if (bytes > ps->wp_pin_bytes) {
    if (ps->wp_pin) HIPCHK(hipHostFree(ps->wp_pin));
    ps->wp_pin = nullptr;
    ps->wp_pin_bytes = 0;
    HIPCHK(hipHostMalloc(&ps->wp_pin, bytes, hipHostMallocDefault));
    ps->wp_pin_bytes = bytes;
  }
  char *pin = (char *)ps->wp_pin, *base = (char *)ps->wp_buf.p;
  std::memcpy(pin, id.data(), n * 4);
  std::memcpy(pin + align_up(n * 4, 256), offsets, (n + 1) * 4);
  if (extra) std::memcpy(pin + align_up(n * 4, 256) + (n + 1) * 4, extra->data(), n * 4);
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  HIPCHK(hipMemcpyAsync(base, pin, bytes, hipMemcpyHostToDevice, st));
  HIPCHK(hipEventRecord(ps->ev_wp, st));
  ps->wp_pin_busy = true;
  *d_ids = (const int *)base;
  *d_offsets = (const int *)(base + align_up(n * 4, 256));
  if (extra) *d_extra = (const int *)(base + align_up(n * 4, 256) + (n + 1) * 4);
  return 0;
}

FitParams fit_params(const tpamd_planner_set *ps, int count, double rounding) {
  const PlannerSetState &S = ps->S;
  FitParams p{};
  p.Q = count; p.D = S.D; p.K = S.K; p.pcap = ps->pcap; p.rounding = rounding;
  p.knots = (double *)S.knots; p.cps = ps->d_cp;
  p.s_vmax = ps->d_vmax; p.s_amax = (double *)S.amax; p.s_delta = ps->d_delta; p.s_iv = ps->d_iv;
  p.np = S.np; p.path_state = S.path_state; p.has_path = S.has_path;
  return p;
}

// the host copies of np / has_path after a fit (its outcome follows from W alone)
void fit_bookkeeping(tpamd_planner_set *ps, int count, const std::vector<int32_t> &id, const int32_t *offsets) {
  for (int k = 0; k < count; k++) {
    const int W = offsets[k + 1] - offsets[k];
    if (W < 1) continue;
    ps->h_np[id[k]] = fit_points(W);
    ps->h_stale[id[k]] = 0;
    ps->h_has[id[k]] = 1;
  }
}

}  // namespace

extern "C" {

int tpamd_planner_set_set_waypoints(tpamd_planner_set *ps, int count, const int32_t *ids,
                                    const int32_t *waypoint_offsets, const double *waypoints, double rounding,
                                    const double *max_velocity, const double *max_acceleration, const double *delta,
                                    const double *initial_velocity, int32_t *num_points, int32_t *status) {
  std::vector<int32_t> id;
  int need = 0;
  int rc = waypoint_args(ps, count, ids, waypoint_offsets, waypoints, max_velocity, max_acceleration, delta, status,
                         &id, &need);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = ps->S.D, rows = (size_t)waypoint_offsets[count];
  // device buffer: in [ids][offsets][waypoints][vmax][amax][delta][iv] | out [num_points][status]
  FitParams p{};
  HostStage s(/*packed=*/true);
  s.up(&p.ids, id.data(), n);
  s.up(&p.offsets, waypoint_offsets, n + 1);
  s.up(&p.wps, waypoints, rows * D);
  s.up(&p.vmax, max_velocity, n * D);
  s.up(&p.amax, max_acceleration, n * D);
  s.up(&p.delta, delta, n);
  s.up(&p.iv, initial_velocity, n * D);
  s.down_or_scratch(&p.np_out, num_points, n);
  s.down(&p.status_out, status, n);
  if (ensure_wp_buf(ps, s.bytes())) return TPAMD_E_HIP;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  rc = ensure_pcap(ps, need, st);
  if (rc) return rc;
  p = fit_params(ps, count, rounding);    // the set's arrays after any growth; upload() adds the staged ones
  if (s.upload(ps->wp_buf.p, st)) return TPAMD_E_HIP;
  launch_set_waypoints(p, st);
  HIPCHK(hipGetLastError());
  rc = s.download(st);
  if (rc) return rc;
  fit_bookkeeping(ps, count, id, waypoint_offsets);
  return 0;
}

int tpamd_planner_set_set_waypoints_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                           const int32_t *waypoint_offsets, const double *waypoints, double rounding,
                                           const double *max_velocity, const double *max_acceleration,
                                           const double *delta, const double *initial_velocity, int32_t *num_points,
                                           int32_t *status, void *hip_stream) {
  std::vector<int32_t> id;
  int need = 0;
  int rc = waypoint_args(ps, count, ids, waypoint_offsets, waypoints, max_velocity, max_acceleration, delta, status,
                         &id, &need);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = (size_t)count, bytes = align_up(n * 4, 256) + (n + 1) * 4;
  if (ensure_wp_buf(ps, bytes)) return TPAMD_E_HIP;
  if (need > ps->pcap) {         // the growth runs on the null stream, after the device calls in flight
    if (order_after_readouts(ps)) return TPAMD_E_HIP;
    rc = ensure_pcap(ps, need, nullptr);
    if (rc) return rc;
  }
  FitParams p = fit_params(ps, count, rounding);
  if (stage_ids_and_offsets(ps, id, waypoint_offsets, st, &p.ids, &p.offsets)) return TPAMD_E_HIP;
  p.wps = waypoints; p.vmax = max_velocity; p.amax = max_acceleration; p.delta = delta; p.iv = initial_velocity;
  p.np_out = num_points; p.status_out = status;
  launch_set_waypoints(p, st);
  HIPCHK(hipGetLastError());
  fit_bookkeeping(ps, count, id, waypoint_offsets);
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- path_tools batches and the retarget
namespace {

bool path_tool_offsets_ok(int count, const int32_t *offsets) {
  if (!offsets || offsets[0] != 0) return false;
  for (int k = 0; k < count; k++)
    if (offsets[k + 1] < offsets[k]) return false;
  return true;
}

// The call-level checks of the two retarget entries (before anything changes): those of
// set_waypoints, the times, and TPAMD_E_UNSUPPORTED on a Cartesian set. *need is the largest
// control-point count a fit of [position, stopping point, waypoints...] can have.
int retarget_args(const tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                  const int32_t *offsets, const double *waypoints, const double *vmax, const double *amax,
                  const double *delta, const int32_t *status, std::vector<int32_t> *id, int *need) {
  if (ps && ps->cartesian) return TPAMD_E_UNSUPPORTED;      // the fit makes a joint spline
  if (!time_ns) return TPAMD_E_INVALID_ARGUMENT;
  int fit = 0;
  const int rc = waypoint_args(ps, count, ids, offsets, waypoints, vmax, amax, delta, status, id, &fit);
  if (rc) return rc;
  long long most = 0;
  for (int k = 0; k < count; k++) most = std::max(most, (long long)offsets[k + 1] - offsets[k]);
  if (most + 2 > (1 << 22)) return TPAMD_E_UNSUPPORTED;
  *need = fit_points((int)most + 2);
  return 0;
}

RetargetParams retarget_params(const tpamd_planner_set *ps, int count, double rounding) {
  const PlannerSetState &S = ps->S;
  RetargetParams p{};
  p.Q = count; p.D = S.D; p.K = S.K; p.pcap = ps->pcap; p.tcap = ps->tcap; p.rounding = rounding;
  p.knots = (double *)S.knots; p.cps = ps->d_cp;
  p.s_vmax = ps->d_vmax; p.s_amax = (double *)S.amax; p.s_delta = ps->d_delta; p.s_iv = ps->d_iv;
  p.np = S.np; p.path_state = S.path_state; p.has_path = S.has_path;
  p.initial_plan = S.initial_plan; p.t_first = S.t_first; p.t_count = S.t_count;
  p.t_time = S.t_time; p.t_q = S.t_q; p.t_qd = S.t_qd;
  return p;
}

}  // namespace

extern "C" {

int tpamd_compute_stopping_points_device(tpamd_engine *e, int count, int num_dofs, const double *position,
                                         const double *velocity, const double *acceleration_limit,
                                         const double *corner_rounding, double *point, int32_t *status,
                                         void *hip_stream) {
  if (!e || count < 0 || num_dofs < 1) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!position || !velocity || !acceleration_limit || !corner_rounding || !point || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  StoppingPointParams p{};
  p.count = count; p.D = num_dofs;
  p.position = position; p.velocity = velocity; p.acceleration_limit = acceleration_limit;
  p.corner_rounding = corner_rounding; p.point = point; p.status = status;
  launch_stopping_points(p, (hipStream_t)hip_stream);
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_compute_stopping_points_host(tpamd_engine *e, int count, int num_dofs, const double *position,
                                       const double *velocity, const double *acceleration_limit,
                                       const double *corner_rounding, double *point, int32_t *status) {
  if (!e || count < 0 || num_dofs < 1) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!position || !velocity || !acceleration_limit || !corner_rounding || !point || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = (size_t)num_dofs;
  const double *d_pos, *d_vel, *d_acc, *d_round;
  double *d_point;
  int32_t *d_st;
  HostStage s(/*packed=*/true);
  s.up(&d_pos, position, n * D);
  s.up(&d_vel, velocity, n * D);
  s.up(&d_acc, acceleration_limit, n * D);
  s.up(&d_round, corner_rounding, n);
  s.both(&d_point, point, n * D);       // a row with a bad limit keeps its point
  s.down(&d_st, status, n);
  if (int rc = s.upload(e->stage, st)) return rc;
  const int rc = tpamd_compute_stopping_points_device(e, count, num_dofs, d_pos, d_vel, d_acc, d_round, d_point, d_st, st);
  return rc ? rc : s.download(st);
}

int tpamd_project_points_on_paths_device(tpamd_engine *e, int count, int num_dofs, const int32_t *waypoint_offsets,
                                         const double *waypoints, const double *point, int32_t *waypoint_index,
                                         double *distance_to_path, double *line_parameter, double *projected_point,
                                         int32_t *status, void *hip_stream) {
  if (!e || count < 0 || num_dofs < 1 || !path_tool_offsets_ok(count, waypoint_offsets)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!point || !waypoint_index || !distance_to_path || !line_parameter || !projected_point || !status ||
      (waypoint_offsets[count] > 0 && !waypoints))
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = (hipStream_t)hip_stream;
  const std::vector<int32_t> ints(waypoint_offsets, waypoint_offsets + count + 1);
  const int32_t *d = nullptr;
  if (int rc = stage_pose_ints(e, ints, st, &d)) return rc;
  ProjectParams p{};
  p.count = count; p.D = num_dofs;
  p.offsets = d; p.wps = waypoints; p.point = point;
  p.waypoint_index = waypoint_index; p.distance = distance_to_path; p.line_parameter = line_parameter;
  p.projected = projected_point; p.status = status;
  launch_project_points(p, st);
  return pose_ints_done(e, st);
}

int tpamd_project_points_on_paths_host(tpamd_engine *e, int count, int num_dofs, const int32_t *waypoint_offsets,
                                       const double *waypoints, const double *point, int32_t *waypoint_index,
                                       double *distance_to_path, double *line_parameter, double *projected_point,
                                       int32_t *status) {
  if (!e || count < 0 || num_dofs < 1 || !path_tool_offsets_ok(count, waypoint_offsets)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!point || !waypoint_index || !distance_to_path || !line_parameter || !projected_point || !status ||
      (waypoint_offsets[count] > 0 && !waypoints))
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = (size_t)num_dofs, rows = (size_t)waypoint_offsets[count];
  const double *d_wps, *d_point;
  int32_t *d_index, *d_st;
  double *d_dist, *d_t, *d_proj;
  HostStage s(/*packed=*/true);
  s.up(&d_wps, waypoints, rows * D);
  s.up(&d_point, point, n * D);
  s.both(&d_index, waypoint_index, n);  // an empty list keeps its outputs
  s.both(&d_dist, distance_to_path, n);
  s.both(&d_t, line_parameter, n);
  s.both(&d_proj, projected_point, n * D);
  s.down(&d_st, status, n);
  if (int rc = s.upload(e->stage, st)) return rc;
  const int rc = tpamd_project_points_on_paths_device(e, count, num_dofs, waypoint_offsets, d_wps, d_point, d_index,
                                                      d_dist, d_t, d_proj, d_st, st);
  return rc ? rc : s.download(st);
}

int tpamd_planner_set_retarget(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                               const int32_t *waypoint_offsets, const double *waypoints, double rounding,
                               const double *max_velocity, const double *max_acceleration, const double *delta,
                               const double *stopping_acceleration, int32_t *num_points, int32_t *status,
                               double *position, double *velocity, double *stopping_point) {
  std::vector<int32_t> id;
  int need = 0;
  int rc = retarget_args(ps, count, ids, time_ns, waypoint_offsets, waypoints, max_velocity, max_acceleration, delta,
                         status, &id, &need);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = ps->S.D, rows = (size_t)waypoint_offsets[count];
  // device buffer: in [time_ns][ids][offsets][waypoints][vmax][amax][delta][stop acc] |
  // out [num_points][status][position][velocity][stopping point] | scratch
  RetargetParams p{};
  std::vector<int32_t> np(n);
  HostStage s(/*packed=*/true);
  s.up(&p.time_ns, time_ns, n);
  s.up(&p.ids, id.data(), n);
  s.up(&p.offsets, waypoint_offsets, n + 1);
  s.up(&p.wps, waypoints, rows * D);
  s.up(&p.vmax, max_velocity, n * D);
  s.up(&p.amax, max_acceleration, n * D);
  s.up(&p.delta, delta, n);
  s.up(&p.stop_acc, stopping_acceleration, n * D);
  s.down(&p.np_out, np.data(), n);
  s.down(&p.status_out, status, n);
  s.both(&p.pos_out, position, n * D);        // a planner that fails keeps its rows
  s.both(&p.vel_out, velocity, n * D);
  s.both(&p.stop_out, stopping_point, n * D);
  s.scratch(&p.scr, (rows + 3 * n) * D);
  if (ensure_wp_buf(ps, s.bytes())) return TPAMD_E_HIP;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  rc = ensure_pcap(ps, need, st);
  if (rc) return rc;
  p = retarget_params(ps, count, rounding);    // the set's arrays after any growth; upload() adds the staged ones
  if (s.upload(ps->wp_buf.p, st)) return TPAMD_E_HIP;
  launch_pset_retarget(p, st);
  HIPCHK(hipGetLastError());
  rc = s.download(st);
  if (rc) return rc;
  for (size_t k = 0; k < n; k++) {
    if (num_points) num_points[k] = np[k];
    if (status[k] != TPAMD_PLAN_OK) continue;
    ps->h_np[id[k]] = np[k];
    ps->h_has[id[k]] = 1;
    ps->h_stale[id[k]] = 0;
  }
  return 0;
}

int tpamd_planner_set_retarget_device(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                                      const int32_t *waypoint_offsets, const double *waypoints, double rounding,
                                      const double *max_velocity, const double *max_acceleration, const double *delta,
                                      const double *stopping_acceleration, int32_t *num_points, int32_t *status,
                                      double *position, double *velocity, double *stopping_point, void *hip_stream) {
  std::vector<int32_t> id;
  int need = 0;
  int rc = retarget_args(ps, count, ids, time_ns, waypoint_offsets, waypoints, max_velocity, max_acceleration, delta,
                         status, &id, &need);
  if (rc) return rc;
  if (!num_points) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = (size_t)count, D = ps->S.D, rows = (size_t)waypoint_offsets[count];
  // wp_buf: [ids][offsets] (stage_ids_and_offsets) | scratch
  const size_t ints = align_up(align_up(n * 4, 256) + (n + 1) * 4, 256);
  if (ensure_wp_buf(ps, ints + (rows + 3 * n) * D * 8)) return TPAMD_E_HIP;
  if (need > ps->pcap) {         // the growth runs on the null stream, after the device calls in flight
    if (order_after_readouts(ps)) return TPAMD_E_HIP;
    rc = ensure_pcap(ps, need, nullptr);
    if (rc) return rc;
  }
  RetargetParams p = retarget_params(ps, count, rounding);
  if (stage_ids_and_offsets(ps, id, waypoint_offsets, st, &p.ids, &p.offsets)) return TPAMD_E_HIP;
  p.time_ns = (const long long *)time_ns; p.wps = waypoints; p.vmax = max_velocity; p.amax = max_acceleration;
  p.delta = delta; p.stop_acc = stopping_acceleration;
  p.scr = (double *)((char *)ps->wp_buf.p + ints);
  p.np_out = num_points; p.status_out = status;
  p.pos_out = position; p.vel_out = velocity; p.stop_out = stopping_point;
  launch_pset_retarget(p, st);
  HIPCHK(hipGetLastError());
  // the outcome stays on the device: the host copies hold an upper bound until they are read back
  for (size_t k = 0; k < n; k++) {
    const int W = waypoint_offsets[k + 1] - waypoint_offsets[k];
    ps->h_np[id[k]] = std::max(ps->h_np[id[k]], fit_points(W + 2));
    ps->h_stale[id[k]] = 1;
  }
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- Cartesian planner sets: IK tables
namespace {

// The call-level checks of the two upload_ik_tables entries (before anything changes): a Cartesian
// set, the arrays, every id in range and listed once (ids NULL: 0..count-1), a state of 1 or 2 and
// delta > 0 where those arrays are host arrays (null here: device arrays), offsets from 0 and
// non-decreasing, at least num_samples rows per planner. Fills id[count] and *longest.
int ik_table_args(const tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *offsets, const double *q,
                  const double *J, const double *path_end, const double *vmax, const double *amax,
                  const double *vtrans, const double *vrot, const double *delta, const int32_t *state,
                  const double *host_delta, const int32_t *host_state, std::vector<int32_t> *id, int *longest) {
  if (!ps || !ps->cartesian || count < 0 || !offsets || !q || !J || !path_end || !vmax || !amax || !vtrans || !vrot ||
      !delta || !state)
    return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = ps->S.B;
  if ((size_t)count > B || offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<char> seen(B, 0);
  id->resize(count);
  long long most = 0;
  for (int k = 0; k < count; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || seen[b]) return TPAMD_E_INVALID_ARGUMENT;
    seen[b] = 1;
    (*id)[k] = (int32_t)b;
    const long long rows = (long long)offsets[k + 1] - offsets[k];
    if (rows < ps->S.N) return TPAMD_E_INVALID_ARGUMENT;
    if (host_delta && !(host_delta[k] > 0.0)) return TPAMD_E_INVALID_ARGUMENT;
    if (host_state && host_state[k] != 1 && host_state[k] != 2) return TPAMD_E_INVALID_ARGUMENT;
    most = std::max(most, rows);
  }
  if (most > (1 << 28)) return TPAMD_E_UNSUPPORTED;
  *longest = (int)most;
  return 0;
}

constexpr size_t kIkStagingKept = (size_t)16 << 20;   // upload staging above this size is freed after the call

// The scatter of the packed tables (device pointers in p) into the set's arrays.
void launch_ik_upload(const tpamd_planner_set *ps, IkUploadParams p, int longest, hipStream_t st) {
  const PlannerSetState &S = ps->S;
  const int D = S.D;
  p.D = D; p.table_stride = ps->table_cap;
  p.t_q = ps->d_tq; p.t_J = ps->d_tJ;
  p.s_path_end = ps->d_path_end; p.s_vmax = ps->d_vmax; p.s_amax = (double *)S.amax; p.s_vtrans = ps->d_vtrans;
  p.s_vrot = ps->d_vrot; p.s_delta = ps->d_delta; p.s_iv = ps->d_iv;
  p.s_rows = ps->d_rows; p.s_state = S.path_state; p.s_has = S.has_path; p.s_first_row = ps->d_first_row;
  const unsigned n = (unsigned)p.count;
  hipLaunchKernelGGL(k_pset_ik_rows, dim3((unsigned)(((size_t)longest * D + 255) / 256), n), dim3(256), 0, st, p, D,
                     p.q, p.t_q);
  hipLaunchKernelGGL(k_pset_ik_rows, dim3((unsigned)(((size_t)longest * 6 * D + 255) / 256), n), dim3(256), 0, st, p,
                     6 * D, p.J, p.t_J);
  hipLaunchKernelGGL(k_pset_ik_scalars, dim3((n + 127) / 128), dim3(128), 0, st, p);
}

void ik_bookkeeping(tpamd_planner_set *ps, int count, const std::vector<int32_t> &id, const int32_t *offsets) {
  for (int k = 0; k < count; k++) {
    ps->h_rows[id[k]] = offsets[k + 1] - offsets[k];
    ps->h_first_row[id[k]] = 0;
    ps->h_has[id[k]] = 1;
  }
}

}  // namespace

extern "C" {

int tpamd_planner_set_upload_ik_tables(tpamd_planner_set *ps, int count, const int32_t *ids,
                                       const int32_t *row_offsets, const double *ik_positions,
                                       const double *jacobians, const double *path_end, const double *max_velocity,
                                       const double *max_acceleration, const double *max_translational_velocity,
                                       const double *max_rotational_velocity, const double *delta,
                                       const double *initial_velocity, const int32_t *path_state) {
  std::vector<int32_t> id;
  int longest = 0;
  int rc = ik_table_args(ps, count, ids, row_offsets, ik_positions, jacobians, path_end, max_velocity,
                         max_acceleration, max_translational_velocity, max_rotational_velocity, delta, path_state,
                         delta, path_state, &id, &longest);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = ps->S.D, rows = (size_t)row_offsets[count];
  // device buffer: [ids][offsets][q][J][path_end][vmax][amax][vtrans][vrot][delta][iv][state]
  IkUploadParams p{};
  HostStage s;
  s.up(&p.ids, id.data(), n);
  s.up(&p.offsets, row_offsets, n + 1);
  s.up(&p.q, ik_positions, rows * D);
  s.up(&p.J, jacobians, rows * 6 * D);
  s.up(&p.path_end, path_end, n);
  s.up(&p.vmax, max_velocity, n * D);
  s.up(&p.amax, max_acceleration, n * D);
  s.up(&p.vtrans, max_translational_velocity, n);
  s.up(&p.vrot, max_rotational_velocity, n);
  s.up(&p.delta, delta, n);
  s.up(&p.iv, initial_velocity, n * D);
  s.up(&p.state, path_state, n);
  if (ensure_wp_buf(ps, s.bytes())) return TPAMD_E_HIP;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  rc = ensure_table_cap(ps, longest, st);
  if (rc) return rc;
  if (s.upload(ps->wp_buf.p, st)) return TPAMD_E_HIP;
  p.count = count;
  for (int32_t b : id)
    if (drop_suspension(ps, b, st)) return TPAMD_E_HIP;
  launch_ik_upload(ps, p, longest, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  // the staging of a whole table is as large as the table: it does not stay with the set
  if (ps->wp_buf.bytes > kIkStagingKept) ps->wp_buf.release();
  ik_bookkeeping(ps, count, id, row_offsets);
  return 0;
}

int tpamd_planner_set_upload_ik_tables_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                              const int32_t *row_offsets, const double *ik_positions,
                                              const double *jacobians, const double *path_end,
                                              const double *max_velocity, const double *max_acceleration,
                                              const double *max_translational_velocity,
                                              const double *max_rotational_velocity, const double *delta,
                                              const double *initial_velocity, const int32_t *path_state,
                                              void *hip_stream) {
  std::vector<int32_t> id;
  int longest = 0;
  int rc = ik_table_args(ps, count, ids, row_offsets, ik_positions, jacobians, path_end, max_velocity,
                         max_acceleration, max_translational_velocity, max_rotational_velocity, delta, path_state,
                         nullptr, nullptr, &id, &longest);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = (size_t)count, bytes = align_up(n * 4, 256) + (n + 1) * 4;
  if (ensure_wp_buf(ps, bytes)) return TPAMD_E_HIP;
  if (longest > ps->table_cap) {   // the growth runs on the null stream, after the device calls in flight
    if (order_after_readouts(ps)) return TPAMD_E_HIP;
    rc = ensure_table_cap(ps, longest, nullptr);
    if (rc) return rc;
  }
  IkUploadParams p{};
  p.count = count;
  if (stage_ids_and_offsets(ps, id, row_offsets, st, &p.ids, &p.offsets)) return TPAMD_E_HIP;
  p.q = ik_positions; p.J = jacobians; p.path_end = path_end; p.vmax = max_velocity; p.amax = max_acceleration;
  p.vtrans = max_translational_velocity; p.vrot = max_rotational_velocity; p.delta = delta; p.iv = initial_velocity;
  p.state = path_state;
  for (int32_t b : id)
    if (drop_suspension(ps, b, st)) return TPAMD_E_HIP;
  launch_ik_upload(ps, p, longest, st);
  HIPCHK(hipGetLastError());
  ik_bookkeeping(ps, count, id, row_offsets);
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

}  // extern "C"

namespace {

// The call-level checks of the two append_ik_rows entries (before anything changes): a Cartesian
// set, the arrays, every id in range, listed once and with a table as far as the host knows,
// offsets from 0 and non-decreasing. Fills id[count], dst[count] (each planner's first new row),
// *longest (the largest count) and *need (the slots the longest table takes after the append: its
// live rows, rows - first_row, plus the new ones).
int ik_append_args(const tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *offsets, const double *q,
                   const double *J, std::vector<int32_t> *id, std::vector<int32_t> *dst, int *longest, int *need) {
  if (!ps || !ps->cartesian || count < 0 || !offsets || !q || !J) return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = ps->S.B;
  if ((size_t)count > B || offsets[0] != 0) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_table_counts(ps)) return rc;
  std::vector<char> seen(B, 0);
  id->resize(count);
  dst->resize(count);
  long long most = 0, rows_after = 0;
  for (int k = 0; k < count; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || seen[b]) return TPAMD_E_INVALID_ARGUMENT;
    seen[b] = 1;
    if (!ps->h_has[b] || ps->h_rows[b] < 1) return TPAMD_E_INVALID_ARGUMENT;
    const long long rows = (long long)offsets[k + 1] - offsets[k];
    if (rows < 0) return TPAMD_E_INVALID_ARGUMENT;
    (*id)[k] = (int32_t)b;
    (*dst)[k] = ps->h_rows[b];
    most = std::max(most, rows);
    if ((long long)ps->h_rows[b] + rows > INT32_MAX) return TPAMD_E_UNSUPPORTED;
    rows_after = std::max(rows_after, (long long)ps->h_rows[b] - ps->h_first_row[b] + rows);
  }
  if (rows_after > (1 << 28)) return TPAMD_E_UNSUPPORTED;
  *longest = (int)most;
  *need = (int)rows_after;
  return 0;
}

// The scatter of the packed rows (device pointers in p) behind the planners' last rows.
void launch_ik_append(const tpamd_planner_set *ps, IkUploadParams p, int longest, hipStream_t st) {
  const int D = ps->S.D;
  p.D = D; p.table_stride = ps->table_cap;
  p.t_q = ps->d_tq; p.t_J = ps->d_tJ;
  p.s_rows = ps->d_rows; p.s_has = ps->S.has_path; p.s_first_row = ps->d_first_row;
  const unsigned n = (unsigned)p.count;
  if (longest > 0) {
    hipLaunchKernelGGL(k_pset_ik_rows, dim3((unsigned)(((size_t)longest * D + 255) / 256), n), dim3(256), 0, st, p, D,
                       p.q, p.t_q);
    hipLaunchKernelGGL(k_pset_ik_rows, dim3((unsigned)(((size_t)longest * 6 * D + 255) / 256), n), dim3(256), 0, st, p,
                       6 * D, p.J, p.t_J);
  }
  hipLaunchKernelGGL(k_pset_ik_append_scalars, dim3((n + 127) / 128), dim3(128), 0, st, p);
}

}  // namespace

extern "C" {

int tpamd_planner_set_append_ik_rows(tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *row_offsets,
                                     const double *ik_positions, const double *jacobians) {
  std::vector<int32_t> id, dst;
  int longest = 0, need = 0;
  int rc = ik_append_args(ps, count, ids, row_offsets, ik_positions, jacobians, &id, &dst, &longest, &need);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = (size_t)count, D = ps->S.D, rows = (size_t)row_offsets[count];
  // device buffer: [ids][offsets][dst_first][q][J]
  IkUploadParams p{};
  HostStage s;
  s.up(&p.ids, id.data(), n);
  s.up(&p.offsets, row_offsets, n + 1);
  s.up(&p.dst_first, dst.data(), n);
  s.up(&p.q, ik_positions, rows * D);
  s.up(&p.J, jacobians, rows * 6 * D);
  if (ensure_wp_buf(ps, s.bytes())) return TPAMD_E_HIP;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  rc = ensure_table_cap(ps, need, st);
  if (rc) return rc;
  if (s.upload(ps->wp_buf.p, st)) return TPAMD_E_HIP;
  p.count = count;
  launch_ik_append(ps, p, longest, st);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  if (ps->wp_buf.bytes > kIkStagingKept) ps->wp_buf.release();
  for (int k = 0; k < count; k++) ps->h_rows[id[k]] += row_offsets[k + 1] - row_offsets[k];
  return 0;
}

int tpamd_planner_set_append_ik_rows_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                            const int32_t *row_offsets, const double *ik_positions,
                                            const double *jacobians, void *hip_stream) {
  std::vector<int32_t> id, dst;
  int longest = 0, need = 0;
  int rc = ik_append_args(ps, count, ids, row_offsets, ik_positions, jacobians, &id, &dst, &longest, &need);
  if (rc) return rc;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = (size_t)count, bytes = align_up(n * 4, 256) + (n + 1) * 4 + n * 4;
  if (ensure_wp_buf(ps, bytes)) return TPAMD_E_HIP;
  if (need > ps->table_cap) {      // the growth runs on the null stream, after the device calls in flight
    if (order_after_readouts(ps)) return TPAMD_E_HIP;
    rc = ensure_table_cap(ps, need, nullptr);
    if (rc) return rc;
  }
  IkUploadParams p{};
  p.count = count;
  if (stage_ids_and_offsets(ps, id, row_offsets, st, &p.ids, &p.offsets, &dst, &p.dst_first)) return TPAMD_E_HIP;
  p.q = ik_positions; p.J = jacobians;
  launch_ik_append(ps, p, longest, st);
  HIPCHK(hipGetLastError());
  for (int k = 0; k < count; k++) ps->h_rows[id[k]] += row_offsets[k + 1] - row_offsets[k];
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

int tpamd_planner_set_download_ik_table(tpamd_planner_set *ps, int planner, int32_t *rows, double *ik_positions,
                                        double *jacobians, int capacity) {
  if (!ps || !rows || planner < 0 || planner >= ps->S.B || !ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_table_counts(ps)) return rc;
  const int R = ps->h_has[planner] ? ps->h_rows[planner] : 0;
  *rows = R;
  if (R > 0 && ps->h_first_row[planner] > 0) return TPAMD_E_INVALID_ARGUMENT;   // rows from 0 are gone
  if (R == 0 || (!ik_positions && !jacobians)) return 0;
  if (R > capacity) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;      // a device upload may still be writing
  const size_t D = ps->S.D, o = (size_t)planner * ps->table_cap;
  if (ik_positions) HIPCHK(hipMemcpy(ik_positions, ps->d_tq + o * D, (size_t)R * D * 8, hipMemcpyDeviceToHost));
  if (jacobians) HIPCHK(hipMemcpy(jacobians, ps->d_tJ + o * 6 * D, (size_t)R * 6 * D * 8, hipMemcpyDeviceToHost));
  return 0;
}

int tpamd_planner_set_discard_ik_rows(tpamd_planner_set *ps, int count, const int32_t *ids, const int32_t *keep_from,
                                      int32_t *first_row_out) {
  if (!ps || !ps->cartesian || count < 0) return TPAMD_E_INVALID_ARGUMENT;
  const size_t B = ps->S.B, n = (size_t)count;
  if (n > B) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_table_counts(ps)) return rc;
  std::vector<char> seen(B, 0);
  std::vector<int32_t> id(n), first(n);
  for (size_t k = 0; k < n; k++) {
    const long long b = ids ? (long long)ids[k] : (long long)k;
    if (b < 0 || b >= (long long)B || seen[b]) return TPAMD_E_INVALID_ARGUMENT;
    seen[b] = 1;
    if (!ps->h_has[b] || ps->h_rows[b] < 1) return TPAMD_E_INVALID_ARGUMENT;
    id[k] = (int32_t)b;
  }
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const PlannerSetState &S = ps->S;
  // device buffer: [ids][keep_from][shift][first_out]; only first_out comes back
  IkDiscardParams p{};
  HostStage s;
  s.up(&p.ids, id.data(), n);
  s.up(&p.keep_from, keep_from, n);
  s.scratch(&p.shift, n);
  s.down(&p.first_out, first.data(), n);
  if (ensure_wp_buf(ps, s.bytes())) return TPAMD_E_HIP;
  if (order_after_readouts(ps)) return TPAMD_E_HIP;      // a device append may still be writing
  if (s.upload(ps->wp_buf.p, st)) return TPAMD_E_HIP;
  p.count = count; p.D = S.D; p.table_stride = ps->table_cap; p.cap = ps->cap;
  p.t_q = ps->d_tq; p.t_J = ps->d_tJ;
  p.s_rows = ps->d_rows; p.s_has = S.has_path; p.s_state = S.path_state; p.s_count = S.count;
  p.s_first_row = ps->d_first_row;
  p.h_time = S.h_time; p.h_s = S.h_s; p.delta = ps->d_delta; p.start_time_ns = S.start_time_ns;
  hipLaunchKernelGGL(k_pset_discard_begin, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, st, p);
  hipLaunchKernelGGL(k_pset_ik_compact, dim3(kCompactSplit, (unsigned)n, 2), dim3(kCompactThreads), 0, st, p);
  HIPCHK(hipGetLastError());
  if (s.download(st)) return TPAMD_E_HIP;
  for (size_t k = 0; k < n; k++) ps->h_first_row[id[k]] = first[k];
  if (first_row_out) std::memcpy(first_row_out, first.data(), n * 4);
  return 0;
}

int tpamd_planner_set_ik_table_info(const tpamd_planner_set *ps, int planner, int32_t *first_row, int32_t *rows,
                                    int32_t *capacity) {
  if (!ps || planner < 0 || planner >= ps->S.B || !ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_table_counts(ps)) return rc;
  const bool has = ps->h_has[planner] && ps->h_rows[planner] > 0;
  if (first_row) *first_row = has ? ps->h_first_row[planner] : 0;
  if (rows) *rows = has ? ps->h_rows[planner] : 0;
  if (capacity) *capacity = ps->table_cap;
  return 0;
}

int tpamd_planner_set_ik_table_device_pointers(const tpamd_planner_set *ps, const double **ik_positions,
                                               const double **jacobians) {
  if (!ps || !ps->cartesian) return TPAMD_E_INVALID_ARGUMENT;
  if (ik_positions) *ik_positions = ps->d_tq;
  if (jacobians) *jacobians = ps->d_tJ;
  return 0;
}

int tpamd_planner_set_download_ik_rows(tpamd_planner_set *ps, int planner, int32_t *first_row, int32_t *rows_live,
                                       double *ik_positions, double *jacobians, int capacity) {
  if (!ps || !first_row || !rows_live || planner < 0 || planner >= ps->S.B || !ps->cartesian)
    return TPAMD_E_INVALID_ARGUMENT;
  if (int rc = refresh_table_counts(ps)) return rc;
  const bool has = ps->h_has[planner] && ps->h_rows[planner] > 0;
  const int R = has ? ps->h_rows[planner] - ps->h_first_row[planner] : 0;
  *first_row = has ? ps->h_first_row[planner] : 0;
  *rows_live = R;
  if (R == 0 || (!ik_positions && !jacobians)) return 0;
  if (R > capacity) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;      // a device append may still be writing
  const size_t D = ps->S.D, o = (size_t)planner * ps->table_cap;
  if (ik_positions) HIPCHK(hipMemcpy(ik_positions, ps->d_tq + o * D, (size_t)R * D * 8, hipMemcpyDeviceToHost));
  if (jacobians) HIPCHK(hipMemcpy(jacobians, ps->d_tJ + o * 6 * D, (size_t)R * 6 * D * 8, hipMemcpyDeviceToHost));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- planner-set readouts
extern "C" {

int tpamd_planner_set_sample_at_ticks(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *start_ns,
                                      int64_t step_ns, int num_ticks, double *q, double *qd, double *qdd,
                                      int32_t *status) {
  if (!sample_args_ok(ps, count, ids, /*host_ids=*/true, start_ns, step_ns, num_ticks, status))
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  const size_t n = count, T = num_ticks, D = ps->S.D, ticks = n * T;
  if ((ticks + 255) / 256 > 0x7fffffff) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  // one copy up [start_ns][ids], one launch, one copy down per requested array
  ReadoutParams p = readout_params(ps);
  std::vector<double> values[3];   // q, qd, qdd as they come down
  double *dst[3] = {q, qd, qdd}, **dev[3] = {&p.q, &p.qd, &p.qdd};
  HostStage in(/*packed=*/true, /*tight=*/true), out;
  in.up(&p.start_ns, start_ns, n);
  in.up(&p.ids, ids, n);
  out.down(&p.status, status, ticks);
  for (int a = 0; a < 3; a++) {
    if (dst[a]) values[a].resize(ticks * D);
    out.down(dev[a], dst[a] ? values[a].data() : nullptr, ticks * D);
  }
  if (in.upload(ps->rd_in, st) || out.upload(ps->rd_out, st)) return TPAMD_E_HIP;
  p.count = count; p.num_ticks = num_ticks; p.step_ns = step_ns;
  hipLaunchKernelGGL(k_pset_sample_at_ticks, dim3((unsigned)((ticks + 255) / 256)), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  // the values come down whole; only the OK ticks reach the caller's arrays
  if (int rc = out.download(st)) return rc;
  for (int a = 0; a < 3; a++) {
    if (!dst[a]) continue;
    for (size_t i = 0; i < ticks; i++)
      if (status[i] == TPAMD_PLAN_OK) std::memcpy(dst[a] + i * D, values[a].data() + i * D, D * 8);
  }
  return 0;
}

int tpamd_planner_set_sample_at_ticks_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                             const int64_t *start_ns, int64_t step_ns, int num_ticks, double *q,
                                             double *qd, double *qdd, int32_t *status, void *hip_stream) {
  if (!sample_args_ok(ps, count, ids, /*host_ids=*/false, start_ns, step_ns, num_ticks, status))
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  const size_t ticks = (size_t)count * num_ticks;
  if ((ticks + 255) / 256 > 0x7fffffff) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  ReadoutParams p = readout_params(ps);
  p.count = count; p.num_ticks = num_ticks; p.ids = ids;
  p.start_ns = (const long long *)start_ns; p.step_ns = step_ns;
  p.q = q; p.qd = qd; p.qdd = qdd; p.status = status;
  hipLaunchKernelGGL(k_pset_sample_at_ticks, dim3((unsigned)((ticks + 255) / 256)), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

int tpamd_planner_set_download_trajectories(tpamd_planner_set *ps, int count, const int32_t *ids, int64_t *offsets,
                                            int64_t capacity, double *time, double *s, double *sd, double *sdd,
                                            double *q, double *qd, double *qdd) {
  if (!pack_args_ok(ps, count, ids, /*host_ids=*/true, offsets, capacity)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) {
    offsets[0] = 0;
    return 0;
  }
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = count, D = ps->S.D;
  // [offsets][ids] up (ids only), the scan, offsets down; then the pack and one copy per array
  ReadoutParams p = readout_params(ps);
  HostStage in(/*packed=*/false, /*tight=*/true);
  in.down(&p.offsets, offsets, n + 1);
  in.up(&p.ids, ids, n);
  int rc = in.upload(ps->rd_in, st);
  if (rc) return rc;
  p.count = count;
  hipLaunchKernelGGL(k_pset_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, p);
  HIPCHK(hipGetLastError());
  rc = in.download(st);
  if (rc) return rc;
  const size_t rows = (size_t)offsets[count];
  if ((int64_t)rows > capacity) return TPAMD_E_INVALID_ARGUMENT;
  HostStage out;
  out.down(&p.o_time, time, rows);
  out.down(&p.o_s, s, rows);
  out.down(&p.o_sd, sd, rows);
  out.down(&p.o_sdd, sdd, rows);
  out.down(&p.o_q, q, rows * D);
  out.down(&p.o_qd, qd, rows * D);
  out.down(&p.o_qdd, qdd, rows * D);
  if (rows == 0 || out.bytes() == 0) return 0;
  rc = out.upload(ps->rd_out, st);
  if (rc) return rc;
  p.capacity = (long long)rows;
  hipLaunchKernelGGL(k_pset_pack_trajectories, dim3((unsigned)n), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  return out.download(st);
}

int tpamd_planner_set_download_trajectories_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                                   int64_t *offsets, int64_t capacity, double *time, double *s,
                                                   double *sd, double *sdd, double *q, double *qd, double *qdd,
                                                   void *hip_stream) {
  if (!pack_args_ok(ps, count, ids, /*host_ids=*/false, offsets, capacity)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  ReadoutParams p = readout_params(ps);
  p.count = count; p.ids = ids; p.offsets = (long long *)offsets; p.capacity = capacity;
  p.o_time = time; p.o_s = s; p.o_sd = sd; p.o_sdd = sdd; p.o_q = q; p.o_qd = qd; p.o_qdd = qdd;
  hipLaunchKernelGGL(k_pset_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, p);      // offsets[0] = 0 for none
  if (count > 0) hipLaunchKernelGGL(k_pset_pack_trajectories, dim3((unsigned)count), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

// Stopping trajectories: the find pass (status, keep, segment rows and shift per listed planner),
// the scan of the segment lengths into offsets, the write pass (rows at offsets[k], if they fit).
int tpamd_planner_set_stop_trajectories(tpamd_planner_set *ps, int count, const int32_t *ids, const int64_t *time_ns,
                                        const double *max_acceleration, double time_step, int32_t *status,
                                        int32_t *keep, int64_t *offsets, int64_t capacity, double *time, double *q,
                                        double *qd, double *qdd) {
  if (!stop_args_ok(ps, count, ids, /*host_ids=*/true, time_ns, max_acceleration, status, keep, offsets, capacity))
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) {
    offsets[0] = 0;
    return 0;
  }
  if (ps->S.D > 16) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = nullptr;
  const size_t n = count, D = ps->S.D;
  // up: [time_ns][max_acceleration][ids]; scratch: [first][last][status][keep][shift][length][offsets]
  StopTrajParams p = stop_params(ps);
  long long *d_offsets = nullptr;
  HostStage in(/*packed=*/true, /*tight=*/true), sb;
  in.up(&p.stop_ns, time_ns, n);
  in.up(&p.amax, max_acceleration, n * D);
  in.up(&p.ids, ids, n);
  sb.scratch(&p.seg_first, n);
  sb.scratch(&p.seg_last, n);
  sb.down(&p.status, status, n);
  sb.down(&p.keep, keep, n);
  sb.scratch(&p.seg_offset, n);
  sb.scratch(&p.seg_len, n);
  sb.down(&d_offsets, offsets, n + 1);
  if (ensure_stop_buf(ps, sb.bytes()) || ps->rd_in.reserve(in.bytes())) return TPAMD_E_HIP;
  // a device stop in flight on another stream may still use the scratch
  if (ps->read_pending) HIPCHK(hipStreamWaitEvent(st, ps->ev_read, 0));
  if (in.upload(ps->rd_in.p, st) || sb.upload(ps->stop_buf.p, st)) return TPAMD_E_HIP;
  p.Q = count; p.mode = kRsSetFind; p.time_step = time_step;
  if (!launch_stop_trajectories((int)D, p, st)) return TPAMD_E_UNSUPPORTED;
  hipLaunchKernelGGL(k_stop_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, count, p.seg_len, d_offsets);
  HIPCHK(hipGetLastError());
  int rc = sb.download(st);
  if (rc) return rc;
  const size_t rows = (size_t)offsets[count];
  if ((int64_t)rows > capacity) return TPAMD_E_INVALID_ARGUMENT;
  HostStage out;
  out.down(&p.o_time, time, rows);
  out.down(&p.o_q, q, rows * D);
  out.down(&p.o_qd, qd, rows * D);
  out.down(&p.o_qdd, qdd, rows * D);
  if (rows == 0 || out.bytes() == 0) return 0;
  rc = out.upload(ps->rd_out, st);
  if (rc) return rc;
  p.mode = kRsSetWrite;
  p.offsets = d_offsets; p.capacity = (long long)rows;
  launch_stop_trajectories((int)D, p, st);
  HIPCHK(hipGetLastError());
  return out.download(st);
}

int tpamd_planner_set_stop_trajectories_device(tpamd_planner_set *ps, int count, const int32_t *ids,
                                               const int64_t *time_ns, const double *max_acceleration,
                                               double time_step, int32_t *status, int32_t *keep, int64_t *offsets,
                                               int64_t capacity, double *time, double *q, double *qd, double *qdd,
                                               void *hip_stream) {
  if (!stop_args_ok(ps, count, ids, /*host_ids=*/false, time_ns, max_acceleration, status, keep, offsets, capacity))
    return TPAMD_E_INVALID_ARGUMENT;
  if (ps->S.D > 16) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  const size_t n = count;
  StopTrajParams p = stop_params(ps);
  HostStage sb;
  sb.scratch(&p.seg_first, n);
  sb.scratch(&p.seg_last, n);
  sb.scratch(&p.seg_offset, n);
  sb.scratch(&p.seg_len, n);
  if (sb.bytes() > 0 && ensure_stop_buf(ps, sb.bytes())) return TPAMD_E_HIP;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  if (sb.upload(ps->stop_buf.p, st)) return TPAMD_E_HIP;   // no copies: the scratch's addresses only
  p.Q = count; p.mode = kRsSetFind;
  p.ids = ids; p.stop_ns = (const long long *)time_ns; p.amax = max_acceleration; p.time_step = time_step;
  p.status = status; p.keep = keep;
  launch_stop_trajectories(ps->S.D, p, st);
  hipLaunchKernelGGL(k_stop_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, count, p.seg_len,
                     (long long *)offsets);                                               // offsets[0] = 0 for none
  p.mode = kRsSetWrite;
  p.offsets = (const long long *)offsets; p.capacity = capacity;
  p.o_time = time; p.o_q = q; p.o_qd = qd; p.o_qdd = qdd;
  launch_stop_trajectories(ps->S.D, p, st);
  HIPCHK(hipGetLastError());
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

}  // extern "C"

// ---------------------------------------------------------------- planner sets: state records
// tpamd_planner_set_state_info / export_state_* / import_state_* / copy_planners (csrc/tpamd_state.h:
// the record; csrc/tpamd_state.hip: the kernels).
namespace {

uint64_t double_bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}

SetShape state_shape(const tpamd_planner_set *ps) {
  SetShape s{};
  s.kind = ps->cartesian ? kStateCartesian : kStateJoint;
  s.num_dofs = ps->S.D; s.num_samples = ps->S.N; s.sampling_method = ps->S.method;
  s.time_step_ns = ps->cfg.time_step_ns;
  s.constraint_safety_bits = double_bits(ps->cfg.constraint_safety);
  s.max_initial_velocity_error_bits = double_bits(ps->cfg.max_initial_velocity_error);
  return s;
}

StateSetView state_view(const tpamd_planner_set *ps) {
  const PlannerSetState &S = ps->S;
  StateSetView v{};
  v.B = S.B; v.D = S.D; v.N = S.N; v.K = S.K; v.pcap = ps->pcap; v.cap = ps->cap; v.tcap = ps->tcap;
  v.table_cap = ps->cartesian ? ps->table_cap : 0;
  v.shape = state_shape(ps);
  v.knots = (double *)S.knots; v.cp = ps->d_cp; v.vmax = ps->d_vmax; v.amax = (double *)S.amax; v.iv = ps->d_iv;
  v.delta = ps->d_delta; v.path_end = ps->d_path_end; v.vtrans = ps->d_vtrans; v.vrot = ps->d_vrot;
  v.np = S.np; v.path_state = S.path_state; v.has_path = S.has_path; v.count = S.count;
  v.initial_plan = S.initial_plan; v.planned_to_end = S.planned_to_end; v.target_reached = S.target_reached;
  v.path_horizon = S.path_horizon; v.path_start = S.path_start; v.path_start_velocity = S.path_start_velocity;
  v.path_time_start = S.path_time_start;
  v.start_time_ns = S.start_time_ns; v.end_time_ns = S.end_time_ns; v.final_decel_start_ns = S.final_decel_start_ns;
  v.w_time = ps->w_time; v.w_lei = ps->w_lei; v.t_first = S.t_first; v.t_count = S.t_count;
  double *h[7] = {S.h_time, S.h_s, S.h_sd, S.h_sdd, S.h_q, S.h_qd, S.h_qdd};
  double *t[7] = {S.t_time, S.t_s, S.t_sd, S.t_sdd, S.t_q, S.t_qd, S.t_qdd};
  for (int i = 0; i < 7; i++) { v.h[i] = h[i]; v.t[i] = t[i]; }
  v.tq = ps->d_tq; v.tJ = ps->d_tJ; v.rows = ps->d_rows; v.first_row = ps->d_first_row;
  v.suspended = ps->cartesian ? ps->d_suspended : nullptr;
  static_assert(sizeof(StateCheckDev) == sizeof(PlannerCheckDev), "check record layouts must agree");
  v.check = ps->checking ? (StateCheckDev *)ps->d_check : nullptr;
  return v;
}

// the largest record the set's capacities allow
uint64_t state_bytes_bound(const tpamd_planner_set *ps) {
  StateRecordHeader h{};
  h.shape = state_shape(ps);
  h.num_points = ps->cartesian ? 0 : ps->pcap;
  h.history_count = ps->cap; h.trajectory_count = ps->tcap;
  h.table_rows = ps->cartesian ? ps->table_cap : 0;
  h.has_path = 1; h.initial_plan = 1;
  return state_record_layout(h).bytes;
}

// workgroups per planner of the copy kernel (each moves 16 KiB per trip): one per 64 KiB a record
// can have, 16 at the most
int state_copy_blocks(const tpamd_planner_set *ps) {
  return (int)std::min<uint64_t>(std::max<uint64_t>(state_bytes_bound(ps) >> 16, 1), 16);
}

// The layout kernel's per-planner scratch: room for every planner of the set from the first state
// call on, so that the enqueued-only entries allocate nothing after it (no call lists more).
int ensure_state_items(tpamd_planner_set *ps) {
  const size_t need = (size_t)ps->S.B * sizeof(StateItem);
  if (need <= ps->state_items.bytes) return 0;
  if (ps->read_pending) HIPCHK(hipEventSynchronize(ps->ev_read));
  return ps->state_items.reserve(need);
}

// ids of a host entry: in range, and each listed once where the call changes planners
bool state_ids_ok(const tpamd_planner_set *ps, int count, const int32_t *ids, bool distinct) {
  if (!ps || count < 0) return false;
  const int B = ps->S.B;
  if (count > B) return false;
  if (!ids) return true;
  std::vector<char> seen(distinct ? B : 0, 0);
  for (int k = 0; k < count; k++) {
    if (ids[k] < 0 || ids[k] >= B) return false;
    if (distinct) {
      if (seen[ids[k]]) return false;
      seen[ids[k]] = 1;
    }
  }
  return true;
}

// offsets[count + 1]: from a multiple of 16 on, non-decreasing, every one a multiple of 16
bool state_offsets_ok(int count, const int64_t *offsets) {
  if (!offsets || offsets[0] < 0) return false;
  for (int k = 0; k <= count; k++)
    if ((offsets[k] & 15) || (k && offsets[k] < offsets[k - 1])) return false;
  return true;
}

// The host copies of a planner's path counts after an import that the host has seen.
void state_bookkeeping(tpamd_planner_set *ps, int b, int num_points, int has_path, int table_rows, int first_row) {
  if (num_points) ps->h_np[b] = num_points;
  ps->h_has[b] = (char)has_path;
  ps->h_stale[b] = 0;
  ps->h_rows[b] = table_rows;
  ps->h_first_row[b] = first_row;
}

// Capacity for records with these counts, before an import of the host kind.
int state_grow_for(tpamd_planner_set *ps, int num_points, int history, int trajectory, int live_rows, hipStream_t st) {
  if (num_points > ps->pcap)
    if (int rc = ensure_pcap(ps, num_points, st)) return rc;
  if (history > ps->cap)
    if (int rc = grow_rows(ps, /*history=*/true, history, st)) return rc;
  if (trajectory > ps->tcap)
    if (int rc = grow_rows(ps, /*history=*/false, trajectory, st)) return rc;
  if (ps->cartesian && live_rows > ps->table_cap)
    if (int rc = ensure_table_cap(ps, live_rows, st)) return rc;
  return 0;
}

// The sizes and counts of the listed planners (host ids, null: 0 .. count-1), on the null stream;
// synchronises. count > 0.
int state_info_run(tpamd_planner_set *ps, int count, const int32_t *ids, StateInfoDev *out) {
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  if (ensure_state_items(ps)) return TPAMD_E_HIP;
  StateCall c{};
  c.count = count;
  c.items = (StateItem *)ps->state_items.p;
  HostStage s;
  s.up(&c.ids, ids, count);
  s.down(&c.info, out, count);
  if (int rc = s.upload(ps->state_buf, nullptr)) return rc;
  launch_state_export(state_view(ps), c, 1, nullptr);
  HIPCHK(hipGetLastError());
  return s.download(nullptr);
}

}  // namespace

extern "C" {

int tpamd_planner_set_state_info(tpamd_planner_set *ps, int count, const int32_t *ids, tpamd_planner_state_info *info) {
  static_assert(sizeof(tpamd_planner_state_info) == sizeof(StateInfoDev), "info layouts must agree");
  static_assert(sizeof(tpamd_planner_summary) == sizeof(StateSummaryDev), "summary layouts must agree");
  if (!state_ids_ok(ps, count, ids, false)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!info) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  return state_info_run(ps, count, ids, (StateInfoDev *)info);
}

size_t tpamd_planner_set_state_bytes_bound(const tpamd_planner_set *ps) {
  return ps ? (size_t)state_bytes_bound(ps) : 0;
}

int tpamd_planner_set_export_state_device(tpamd_planner_set *ps, int count, const int32_t *ids, void *blob,
                                          const int64_t *offsets, int32_t *status, void *hip_stream) {
  if (!ps || count < 0 || count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!blob || !offsets || !status || ((uintptr_t)blob & 15)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (ensure_state_items(ps)) return TPAMD_E_HIP;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  StateCall c{};
  c.count = count; c.ids = ids; c.blob = (unsigned char *)blob; c.offsets = (const long long *)offsets;
  c.status = status; c.items = (StateItem *)ps->state_items.p;
  launch_state_export(state_view(ps), c, state_copy_blocks(ps), st);
  HIPCHK(hipGetLastError());
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

int tpamd_planner_set_export_state_host(tpamd_planner_set *ps, int count, const int32_t *ids, void *blob,
                                        const int64_t *offsets, int32_t *status) {
  if (!state_ids_ok(ps, count, ids, false)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!blob || !status || !state_offsets_ok(count, offsets)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  if (ensure_state_items(ps)) return TPAMD_E_HIP;
  const size_t total = (size_t)offsets[count];
  StateCall c{};
  c.count = count;
  c.items = (StateItem *)ps->state_items.p;
  HostStage s;
  s.up(&c.ids, ids, count);
  s.up(&c.offsets, offsets, count + 1);
  s.down(&c.status, status, count);
  // the caller's bytes go up first: what no record covers comes back as it was, as the _device entry leaves it
  if (total > 0) s.both(&c.blob, blob, total);
  else s.scratch(&c.blob, 16);      // every slot is empty: the statuses alone
  if (int rc = s.upload(ps->state_buf, nullptr)) return rc;
  launch_state_export(state_view(ps), c, state_copy_blocks(ps), nullptr);
  HIPCHK(hipGetLastError());
  return s.download(nullptr);
}

int tpamd_planner_set_import_state_device(tpamd_planner_set *ps, int count, const int32_t *ids, const void *blob,
                                          const int64_t *offsets, tpamd_planner_summary *summary, int32_t *status,
                                          void *hip_stream) {
  if (!ps || count < 0 || count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!blob || !offsets || !status || ((uintptr_t)blob & 15)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(ps->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (ensure_state_items(ps)) return TPAMD_E_HIP;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  StateCall c{};
  c.count = count; c.ids = ids; c.blob = (unsigned char *)blob; c.offsets = (const long long *)offsets;
  c.status = status; c.summary = (StateSummaryDev *)summary; c.items = (StateItem *)ps->state_items.p;
  launch_state_import(state_view(ps), c, state_copy_blocks(ps), st);
  HIPCHK(hipGetLastError());
  // the outcome stays on the device: the host copies of the planners the call may have changed hold
  // an upper bound (np) until they are read back (refresh_path_counts, refresh_table_counts)
  const int B = ps->S.B;
  for (int b = 0; b < (ids ? B : count); b++) {
    ps->h_np[b] = std::max(ps->h_np[b], ps->pcap);
    ps->h_stale[b] = 1;
  }
  if (ps->cartesian) ps->table_stale = true;
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

int tpamd_planner_set_import_state_host(tpamd_planner_set *ps, int count, const int32_t *ids, const void *blob,
                                        const int64_t *offsets, tpamd_planner_summary *summary, int32_t *status) {
  if (!state_ids_ok(ps, count, ids, true)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!blob || !status || !state_offsets_ok(count, offsets)) return TPAMD_E_INVALID_ARGUMENT;
  // every record before anything changes
  const SetShape shape = state_shape(ps);
  const unsigned char *bytes = (const unsigned char *)blob;
  std::vector<StateRecordHeader> head(count);
  int np = 0, hc = 0, tc = 0, live = 0;
  for (int k = 0; k < count; k++) {
    const unsigned char *rec = bytes + offsets[k];
    if (state_record_validate(rec, (size_t)(offsets[k + 1] - offsets[k]), shape) != kStateOk)
      return TPAMD_E_INVALID_ARGUMENT;
    head[k] = state_record_header(rec);
    np = std::max(np, head[k].num_points); hc = std::max(hc, head[k].history_count);
    tc = std::max(tc, head[k].trajectory_count); live = std::max(live, head[k].table_rows - head[k].first_row);
  }
  TPAMD_ON_DEVICE(ps->e);
  if (order_after_readouts(ps)) return TPAMD_E_HIP;
  if (int rc = refresh_table_counts(ps)) return rc;
  if (int rc = state_grow_for(ps, np, hc, tc, live, nullptr)) return rc;
  if (ensure_state_items(ps)) return TPAMD_E_HIP;
  const size_t total = (size_t)offsets[count];
  std::vector<StateSummaryDev> sum(count);
  StateCall c{};
  c.count = count;
  c.items = (StateItem *)ps->state_items.p;
  HostStage s;
  s.up(&c.ids, ids, count);
  s.up(&c.offsets, offsets, count + 1);
  s.down(&c.status, status, count);
  s.down(&c.summary, sum.data(), count);
  s.up(&c.blob, blob, total);
  if (int rc = s.upload(ps->state_buf, nullptr)) return rc;
  launch_state_import(state_view(ps), c, state_copy_blocks(ps), nullptr);
  HIPCHK(hipGetLastError());
  if (int rc = s.download(nullptr)) return rc;
  if (summary) std::memcpy(summary, sum.data(), (size_t)count * sizeof(StateSummaryDev));
  for (int k = 0; k < count; k++)
    if (status[k] == TPAMD_PLAN_OK)
      state_bookkeeping(ps, ids ? ids[k] : k, head[k].num_points, head[k].has_path, head[k].table_rows,
                        head[k].first_row);
  return 0;
}

int tpamd_planner_set_copy_planners(tpamd_planner_set *dst, const int32_t *dst_ids, tpamd_planner_set *src,
                                    const int32_t *src_ids, int count, tpamd_planner_summary *summary,
                                    int32_t *status) {
  if (!dst || !src || !state_ids_ok(dst, count, dst_ids, true) || !state_ids_ok(src, count, src_ids, false))
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  if (!status || !state_shape_equal(state_shape(dst), state_shape(src))) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<StateInfoDev> info(count);
  std::vector<int64_t> offsets(count + 1, 0);
  {
    TPAMD_ON_DEVICE(src->e);
    if (int rc = state_info_run(src, count, src_ids, info.data())) return rc;
  }
  int np = 0, hc = 0, tc = 0, live = 0;
  for (int k = 0; k < count; k++) {
    // a planner that refused (it waits for IK rows) gets a header's room: the import reports it
    offsets[k + 1] = offsets[k] + (info[k].status == TPAMD_PLAN_OK ? info[k].bytes : (int64_t)sizeof(StateRecordHeader));
    np = std::max(np, info[k].num_points); hc = std::max(hc, info[k].history_count);
    tc = std::max(tc, info[k].trajectory_count); live = std::max(live, info[k].table_rows - info[k].first_row);
  }
  const size_t total = (size_t)offsets[count];
  std::vector<int32_t> exported(count, 0);
  if (dst->e->device != src->e->device) {
    // the host pair: down from the source's device, up to the destination's
    std::vector<unsigned char> blob(total);
    if (int rc = tpamd_planner_set_export_state_host(src, count, src_ids, blob.data(), offsets.data(), exported.data()))
      return rc;
    for (int k = 0; k < count; k++)
      if (exported[k] != TPAMD_PLAN_OK) {      // nothing changes unless every planner can move
        std::memcpy(status, exported.data(), (size_t)count * 4);
        return 0;
      }
    return tpamd_planner_set_import_state_host(dst, count, dst_ids, blob.data(), offsets.data(), summary, status);
  }
  TPAMD_ON_DEVICE(dst->e);
  for (int k = 0; k < count; k++)
    if (info[k].status != TPAMD_PLAN_OK) {       // nothing changes unless every planner can move
      for (int j = 0; j < count; j++) status[j] = info[j].status;
      return 0;
    }
  // through a scratch blob on the device, so that with dst == src any permutation of the ids works
  if (order_after_readouts(dst) || order_after_readouts(src)) return TPAMD_E_HIP;
  if (int rc = refresh_table_counts(dst)) return rc;
  if (int rc = state_grow_for(dst, np, hc, tc, live, nullptr)) return rc;
  if (ensure_state_items(src) || ensure_state_items(dst)) return TPAMD_E_HIP;
  std::vector<StateSummaryDev> sum(count);
  StateCall ex{}, im{};
  ex.count = im.count = count;
  ex.items = (StateItem *)src->state_items.p;
  im.items = (StateItem *)dst->state_items.p;
  int32_t *d_exported = nullptr;
  HostStage s;
  s.up(&ex.ids, src_ids, count);
  s.up(&im.ids, dst_ids, count);
  s.up(&ex.offsets, offsets.data(), count + 1);
  s.down(&d_exported, exported.data(), count);
  s.down(&im.status, status, count);
  s.down(&im.summary, sum.data(), count);
  s.scratch(&ex.blob, total);
  if (int rc = s.upload(dst->state_buf, nullptr)) return rc;
  ex.status = d_exported;
  im.offsets = ex.offsets;
  im.blob = ex.blob;
  launch_state_export(state_view(src), ex, state_copy_blocks(src), nullptr);
  launch_state_import(state_view(dst), im, state_copy_blocks(dst), nullptr);
  HIPCHK(hipGetLastError());
  if (int rc = s.download(nullptr)) return rc;
  if (summary) std::memcpy(summary, sum.data(), (size_t)count * sizeof(StateSummaryDev));
  for (int k = 0; k < count; k++)
    if (status[k] == TPAMD_PLAN_OK)
      state_bookkeeping(dst, dst_ids ? dst_ids[k] : k, info[k].num_points, info[k].has_path, info[k].table_rows,
                        info[k].first_row);
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------- buffer sets
struct tpamd_buffer_set {
  tpamd_engine *e = nullptr;
  void *fixed = nullptr, *rows = nullptr;   // first | count | sequence; time | q | qd | qdd (grows)
  size_t fixed_bytes = 0, rows_bytes = 0;
  BufferSetState S{};
  DeviceBuffer in, out;                     // staging of the host-pointer entries; they grow
};

namespace {

size_t carve_buffer_rows(char *base, size_t B, size_t cap, size_t D, BufferSetState *S) {
  Stage st(base);
  double *t = st.take<double>(B * cap), *q = st.take<double>(B * cap * D), *qd = st.take<double>(B * cap * D),
         *qdd = st.take<double>(B * cap * D);
  if (S) { S->time = t; S->q = q; S->qd = qd; S->qdd = qdd; S->cap = (int)cap; }
  return st.off;
}

// Rows of a larger per-buffer capacity; every buffer's samples move to row 0. Synchronises.
int bset_grow(tpamd_buffer_set *bs, int new_cap, hipStream_t st) {
  const BufferSetState old = bs->S;
  void *old_rows = bs->rows, *fresh = nullptr;
  const size_t need = carve_buffer_rows(nullptr, old.B, new_cap, old.D, nullptr);
  HIPCHK(hipMalloc(&fresh, need));
  carve_buffer_rows((char *)fresh, old.B, new_cap, old.D, &bs->S);
  bs->rows = fresh; bs->rows_bytes = need;
  hipLaunchKernelGGL(k_bset_regrow, dim3((unsigned)old.B), dim3(kBsThreads), 0, st, old, bs->S);
  hipLaunchKernelGGL(k_bset_zero_first, dim3((unsigned)((old.B + 255) / 256)), dim3(256), 0, st, old.B, old.first);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipFree(old_rows));
  return 0;
}

// Host-pointer inserts: the listed buffers' sample counts come down, and the capacity doubles
// until count + extra[k] rows fit every listed buffer -- before anything changes.
int bset_make_room(tpamd_buffer_set *bs, int count, const int32_t *ids, const std::vector<long long> &extra,
                   hipStream_t st) {
  std::vector<int> have(bs->S.B);
  HIPCHK(hipMemcpyAsync(have.data(), bs->S.count, have.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  long long need = 0;
  for (int k = 0; k < count; k++) need = std::max(need, (long long)have[ids ? ids[k] : k] + extra[k]);
  if (need <= bs->S.cap) return 0;
  long long cap = std::max(bs->S.cap, 1);
  while (cap < need) cap *= 2;
  if (cap > 0x3fffffff) return TPAMD_E_UNSUPPORTED;
  return bset_grow(bs, (int)cap, st);
}

// count and ids of a call: ids null lists buffers 0 .. count-1; host ids are range-checked, and in
// a call that changes buffers each may be listed once.
bool bset_list_ok(const tpamd_buffer_set *bs, int count, const int32_t *ids, bool host_ids, bool mutating) {
  if (!bs || count < 0) return false;
  if (!ids && count > bs->S.B) return false;
  if (ids && host_ids) {
    std::vector<char> seen(mutating ? bs->S.B : 0, 0);
    for (int k = 0; k < count; k++) {
      if (ids[k] < 0 || ids[k] >= bs->S.B) return false;
      if (mutating && seen[ids[k]]++) return false;
    }
  }
  return true;
}

BufferOpParams bset_params(const tpamd_buffer_set *bs, int count) {
  BufferOpParams p{};
  p.S = bs->S;
  p.count = count;
  return p;
}

// ReadoutParams view of a buffer set: its layout is that of a planner set's resident trajectories
ReadoutParams bset_readout_params(const tpamd_buffer_set *bs) {
  const BufferSetState &S = bs->S;
  ReadoutParams p{};
  p.B = S.B; p.D = S.D; p.tcap = S.cap;
  p.t_first = S.first; p.t_count = S.count;
  p.t_time = S.time; p.t_q = S.q; p.t_qd = S.qd; p.t_qdd = S.qdd;
  return p;
}

enum BsetOp { kOpInsert, kOpDiscard, kOpStop, kOpAddOffset, kOpClear, kOpInfo };

// one launch on st
int bset_launch(BsetOp op, const BufferOpParams &p, hipStream_t st) {
  if (p.count <= 0) return 0;
  const dim3 per_lane((unsigned)((p.count + 63) / 64)), per_group((unsigned)p.count);
  switch (op) {
    case kOpInsert: hipLaunchKernelGGL(k_bset_insert, per_group, dim3(kBsThreads), 0, st, p); break;
    case kOpDiscard: hipLaunchKernelGGL(k_bset_discard, per_lane, dim3(64), 0, st, p); break;
    case kOpStop: if (!launch_bset_stop(p, st)) return TPAMD_E_UNSUPPORTED; break;
    case kOpAddOffset: hipLaunchKernelGGL(k_bset_add_offset, per_group, dim3(kBsThreads), 0, st, p); break;
    case kOpClear: hipLaunchKernelGGL(k_bset_clear, per_lane, dim3(64), 0, st, p); break;
    case kOpInfo: hipLaunchKernelGGL(k_bset_info, per_lane, dim3(64), 0, st, p); break;
  }
  HIPCHK(hipGetLastError());
  return 0;
}

// the staged form of a host-pointer call: inputs up in one copy, the launch, outputs down
int bset_run_host(tpamd_buffer_set *bs, BsetOp op, const BufferOpParams &p, HostStage &in, HostStage &out,
                  hipStream_t st) {
  if (int rc = bset_launch(op, p, st)) return rc;
  (void)bs; (void)in;
  return out.download(st);
}

bool one_time(const void *a, const void *b) { return (a != nullptr) != (b != nullptr); }

}  // namespace

extern "C" {

int tpamd_buffer_set_create(tpamd_engine *e, int num_buffers, int num_dofs, int capacity, double timestep_tolerance,
                            tpamd_buffer_set **out) {
  if (!e || !out || num_buffers < 1 || num_dofs < 1 || capacity < 0 || !(timestep_tolerance > 0))
    return TPAMD_E_INVALID_ARGUMENT;
  if (num_dofs > kRsMaxDofs) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(e);
  tpamd_buffer_set *bs = new (std::nothrow) tpamd_buffer_set;
  if (!bs) return TPAMD_E_HIP;
  bs->e = e;
  BufferSetState &S = bs->S;
  S.B = num_buffers; S.D = num_dofs; S.tol = timestep_tolerance;
  const int cap = capacity > 0 ? capacity : 256;
  Stage fx(nullptr);
  fx.take<int>(S.B); fx.take<int>(S.B); fx.take<int>(S.B);
  bs->fixed_bytes = fx.off;
  bs->rows_bytes = carve_buffer_rows(nullptr, S.B, cap, S.D, nullptr);
  if (hipMalloc(&bs->fixed, bs->fixed_bytes) != hipSuccess || hipMalloc(&bs->rows, bs->rows_bytes) != hipSuccess ||
      hipMemset(bs->fixed, 0, bs->fixed_bytes) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
    tpamd_buffer_set_destroy(bs);
    return TPAMD_E_HIP;
  }
  Stage f2(bs->fixed);
  S.first = f2.take<int>(S.B); S.count = f2.take<int>(S.B); S.sequence = f2.take<int>(S.B);
  carve_buffer_rows((char *)bs->rows, S.B, cap, S.D, &S);
  *out = bs;
  return 0;
}

void tpamd_buffer_set_destroy(tpamd_buffer_set *bs) {
  if (!bs) return;
  DeviceScope scope(bs->e->device);
  (void)hipDeviceSynchronize();          // calls enqueued on the caller's streams may still use the rows
  if (bs->fixed) (void)hipFree(bs->fixed);
  if (bs->rows) (void)hipFree(bs->rows);
  bs->in.release();
  bs->out.release();
  delete bs;
}

int tpamd_buffer_set_reserve(tpamd_buffer_set *bs, int capacity) {
  if (!bs || capacity < 0) return TPAMD_E_INVALID_ARGUMENT;
  if (capacity <= bs->S.cap) return 0;
  TPAMD_ON_DEVICE(bs->e);
  HIPCHK(hipDeviceSynchronize());        // earlier _device calls on other streams
  return bset_grow(bs, capacity, nullptr);
}

int tpamd_buffer_set_capacity(const tpamd_buffer_set *bs) { return bs ? bs->S.cap : 0; }

size_t tpamd_buffer_set_device_bytes(const tpamd_buffer_set *bs) {
  return bs ? bs->fixed_bytes + bs->rows_bytes + bs->in.bytes + bs->out.bytes : 0;
}

// ---- insert
int tpamd_buffer_set_insert(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *offsets,
                            const double *time, const double *q, const double *qd, const double *qdd,
                            int32_t *status) {
  if (!bset_list_ok(bs, count, ids, true, true) || !offsets || !status) return TPAMD_E_INVALID_ARGUMENT;
  if (offsets[0] < 0) return TPAMD_E_INVALID_ARGUMENT;
  std::vector<long long> extra(count);
  for (int k = 0; k < count; k++) {
    if (offsets[k + 1] < offsets[k]) return TPAMD_E_INVALID_ARGUMENT;
    extra[k] = offsets[k + 1] - offsets[k];
  }
  const size_t rows = (size_t)offsets[count], n = count, D = bs->S.D;
  if (rows > 0 && (!time || !q || !qd || !qdd)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  if (int rc = bset_make_room(bs, count, ids, extra, st)) return rc;
  BufferOpParams p = bset_params(bs, count);
  HostStage in(/*packed=*/true), out;
  in.up(&p.offsets, offsets, n + 1);
  in.up(&p.i_time, time, rows);
  in.up(&p.i_q, q, rows * D);
  in.up(&p.i_qd, qd, rows * D);
  in.up(&p.i_qdd, qdd, rows * D);
  in.up(&p.ids, ids, n);
  out.down(&p.status, status, n);
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  p.source = kBsFromRows; p.capacity = (long long)rows;
  return bset_run_host(bs, kOpInsert, p, in, out, st);
}

int tpamd_buffer_set_insert_device(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *offsets,
                                   int64_t capacity, const double *time, const double *q, const double *qd,
                                   const double *qdd, int32_t *status, void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, true) || !offsets || !status || capacity < 0)
    return TPAMD_E_INVALID_ARGUMENT;
  if (capacity > 0 && (!time || !q || !qd || !qdd)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.status = status; p.source = kBsFromRows;
  p.offsets = (const long long *)offsets; p.capacity = capacity;
  p.i_time = time; p.i_q = q; p.i_qd = qd; p.i_qdd = qdd;
  return bset_launch(kOpInsert, p, (hipStream_t)hip_stream);
}

static int bset_from_planner_args(const tpamd_buffer_set *bs, const tpamd_planner_set *ps) {
  if (!bs || !ps || bs->e != ps->e || bs->S.D != ps->S.D) return TPAMD_E_INVALID_ARGUMENT;
  return 0;
}
static void bset_planner_source(BufferOpParams &p, const tpamd_planner_set *ps) {
  p.source = kBsFromPlanners;
  p.pB = ps->S.B; p.ptcap = ps->tcap;
  p.t_first = ps->S.t_first; p.t_count = ps->S.t_count;
  p.i_time = ps->S.t_time; p.i_q = ps->S.t_q; p.i_qd = ps->S.t_qd; p.i_qdd = ps->S.t_qdd;
}

int tpamd_buffer_set_insert_from_planner_set(tpamd_buffer_set *bs, tpamd_planner_set *ps, int count,
                                             const int32_t *ids, const int32_t *planner_ids, int32_t *status) {
  if (bset_from_planner_args(bs, ps) || !bset_list_ok(bs, count, ids, true, true) || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (!planner_ids && count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (planner_ids)
    for (int k = 0; k < count; k++)
      if (planner_ids[k] < 0 || planner_ids[k] >= ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  // a device readout of the planner set: behind its last change and its readouts in flight
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  std::vector<int> samples(ps->S.B);
  HIPCHK(hipMemcpyAsync(samples.data(), ps->S.t_count, samples.size() * 4, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  std::vector<long long> extra(count);
  for (int k = 0; k < count; k++) extra[k] = samples[planner_ids ? planner_ids[k] : k];
  if (int rc = bset_make_room(bs, count, ids, extra, st)) return rc;
  BufferOpParams p = bset_params(bs, count);
  const size_t n = count;
  HostStage in(/*packed=*/true), out;
  in.up(&p.ids, ids, n);
  in.up(&p.planner_ids, planner_ids, n);
  out.down(&p.status, status, n);
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  bset_planner_source(p, ps);
  return bset_run_host(bs, kOpInsert, p, in, out, st);
}

int tpamd_buffer_set_insert_from_planner_set_device(tpamd_buffer_set *bs, tpamd_planner_set *ps, int count,
                                                    const int32_t *ids, const int32_t *planner_ids,
                                                    int32_t *status, void *hip_stream) {
  if (bset_from_planner_args(bs, ps) || !bset_list_ok(bs, count, ids, false, true) || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (!planner_ids && count > ps->S.B) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = (hipStream_t)hip_stream;
  if (readout_begin(ps, st)) return TPAMD_E_HIP;
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.planner_ids = planner_ids; p.status = status;
  bset_planner_source(p, ps);
  if (int rc = bset_launch(kOpInsert, p, st)) return rc;
  return readout_end(ps, st) ? TPAMD_E_HIP : 0;
}

// ---- append
int tpamd_buffer_set_append_sample(tpamd_buffer_set *bs, int count, const int32_t *ids, const double *time,
                                   const double *q, const double *qd, const double *qdd, int32_t *status) {
  if (!bset_list_ok(bs, count, ids, true, true) || !time || !q || !qd || !qdd || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  if (int rc = bset_make_room(bs, count, ids, std::vector<long long>(count, 1), st)) return rc;
  BufferOpParams p = bset_params(bs, count);
  const size_t n = count, D = bs->S.D;
  HostStage in(/*packed=*/true), out;
  in.up(&p.i_time, time, n);
  in.up(&p.i_q, q, n * D);
  in.up(&p.i_qd, qd, n * D);
  in.up(&p.i_qdd, qdd, n * D);
  in.up(&p.ids, ids, n);
  out.down(&p.status, status, n);
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  p.source = kBsAppend;
  return bset_run_host(bs, kOpInsert, p, in, out, st);
}

int tpamd_buffer_set_append_sample_device(tpamd_buffer_set *bs, int count, const int32_t *ids, const double *time,
                                          const double *q, const double *qd, const double *qdd, int32_t *status,
                                          void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, true) || !time || !q || !qd || !qdd || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.status = status; p.source = kBsAppend;
  p.i_time = time; p.i_q = q; p.i_qd = qd; p.i_qdd = qdd;
  return bset_launch(kOpInsert, p, (hipStream_t)hip_stream);
}

// ---- discard, add_offset, clear: a time (or none) per listed buffer, nothing comes back
static int bset_simple_host(tpamd_buffer_set *bs, BsetOp op, int count, const int32_t *ids, const int64_t *time_ns,
                            const double *time_sec) {
  if (!bset_list_ok(bs, count, ids, true, true)) return TPAMD_E_INVALID_ARGUMENT;
  if (op != kOpClear && !one_time(time_ns, time_sec)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  BufferOpParams p = bset_params(bs, count);
  const size_t n = count;
  HostStage in(/*packed=*/true), out;
  in.up(&p.time_ns, time_ns, n);
  in.up(&p.time_sec, time_sec, n);
  in.up(&p.ids, ids, n);
  if (in.upload(bs->in, st)) return TPAMD_E_HIP;
  return bset_run_host(bs, op, p, in, out, st);
}
static int bset_simple_device(tpamd_buffer_set *bs, BsetOp op, int count, const int32_t *ids, const int64_t *time_ns,
                              const double *time_sec, int32_t *status, void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, true)) return TPAMD_E_INVALID_ARGUMENT;
  if (op != kOpClear && !one_time(time_ns, time_sec)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.status = status;
  p.time_ns = (const long long *)time_ns; p.time_sec = time_sec;
  return bset_launch(op, p, (hipStream_t)hip_stream);
}

int tpamd_buffer_set_discard_before(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *time_ns,
                                    const double *time_sec) {
  return bset_simple_host(bs, kOpDiscard, count, ids, time_ns, time_sec);
}
int tpamd_buffer_set_discard_before_device(tpamd_buffer_set *bs, int count, const int32_t *ids,
                                           const int64_t *time_ns, const double *time_sec, int32_t *status,
                                           void *hip_stream) {
  return bset_simple_device(bs, kOpDiscard, count, ids, time_ns, time_sec, status, hip_stream);
}
int tpamd_buffer_set_add_offset(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *offset_ns,
                                const double *offset_sec) {
  return bset_simple_host(bs, kOpAddOffset, count, ids, offset_ns, offset_sec);
}
int tpamd_buffer_set_add_offset_device(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *offset_ns,
                                       const double *offset_sec, int32_t *status, void *hip_stream) {
  return bset_simple_device(bs, kOpAddOffset, count, ids, offset_ns, offset_sec, status, hip_stream);
}
int tpamd_buffer_set_clear(tpamd_buffer_set *bs, int count, const int32_t *ids) {
  return bset_simple_host(bs, kOpClear, count, ids, nullptr, nullptr);
}
int tpamd_buffer_set_clear_device(tpamd_buffer_set *bs, int count, const int32_t *ids, int32_t *status,
                                  void *hip_stream) {
  return bset_simple_device(bs, kOpClear, count, ids, nullptr, nullptr, status, hip_stream);
}

// ---- stop
int tpamd_buffer_set_stop_before_time(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *time_ns,
                                      const double *time_sec, const double *max_acceleration, double time_step,
                                      int32_t *status) {
  if (!bset_list_ok(bs, count, ids, true, true) || !one_time(time_ns, time_sec) || !max_acceleration || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  BufferOpParams p = bset_params(bs, count);
  const size_t n = count, D = bs->S.D;
  HostStage in(/*packed=*/true), out;
  in.up(&p.time_ns, time_ns, n);
  in.up(&p.time_sec, time_sec, n);
  in.up(&p.amax, max_acceleration, n * D);
  in.up(&p.ids, ids, n);
  out.down(&p.status, status, n);
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  p.time_step = time_step;
  return bset_run_host(bs, kOpStop, p, in, out, st);
}

int tpamd_buffer_set_stop_before_time_device(tpamd_buffer_set *bs, int count, const int32_t *ids,
                                             const int64_t *time_ns, const double *time_sec,
                                             const double *max_acceleration, double time_step, int32_t *status,
                                             void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, true) || !one_time(time_ns, time_sec) || !max_acceleration || !status)
    return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.status = status;
  p.time_ns = (const long long *)time_ns; p.time_sec = time_sec;
  p.amax = max_acceleration; p.time_step = time_step;
  return bset_launch(kOpStop, p, (hipStream_t)hip_stream);
}

// ---- info
int tpamd_buffer_set_info(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *time_ns,
                          int32_t *num_samples, int32_t *sequence, int64_t *start_ns, int64_t *end_ns,
                          int32_t *positions_up_to) {
  if (!bset_list_ok(bs, count, ids, true, false) || (positions_up_to && !time_ns)) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  BufferOpParams p = bset_params(bs, count);
  const size_t n = count;
  HostStage in(/*packed=*/true), out(/*packed=*/true);
  in.up(&p.time_ns, time_ns, n);
  in.up(&p.ids, ids, n);
  out.down(&p.o_start_ns, start_ns, n);
  out.down(&p.o_end_ns, end_ns, n);
  out.down(&p.o_count, num_samples, n);
  out.down(&p.o_sequence, sequence, n);
  out.down(&p.o_up_to, positions_up_to, n);
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  return bset_run_host(bs, kOpInfo, p, in, out, st);
}

int tpamd_buffer_set_info_device(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *time_ns,
                                 int32_t *num_samples, int32_t *sequence, int64_t *start_ns, int64_t *end_ns,
                                 int32_t *positions_up_to, void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, false) || (positions_up_to && !time_ns)) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  BufferOpParams p = bset_params(bs, count);
  p.ids = ids; p.time_ns = (const long long *)time_ns;
  p.o_count = num_samples; p.o_sequence = sequence; p.o_up_to = positions_up_to;
  p.o_start_ns = (long long *)start_ns; p.o_end_ns = (long long *)end_ns;
  return bset_launch(kOpInfo, p, (hipStream_t)hip_stream);
}

// ---- sample_at_ticks and the packed download: the readout kernels on the buffer set's rows
int tpamd_buffer_set_sample_at_ticks(tpamd_buffer_set *bs, int count, const int32_t *ids, const int64_t *start_ns,
                                     int64_t step_ns, int num_ticks, double *q, double *qd, double *qdd,
                                     int32_t *status) {
  if (!bset_list_ok(bs, count, ids, true, false) || !start_ns || !status || step_ns <= 0 || num_ticks < 1)
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  const size_t n = count, T = num_ticks, D = bs->S.D, ticks = n * T;
  if ((ticks + 255) / 256 > 0x7fffffff) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  ReadoutParams p = bset_readout_params(bs);
  std::vector<double> values[3];   // q, qd, qdd as they come down
  double *dst[3] = {q, qd, qdd}, **dev[3] = {&p.q, &p.qd, &p.qdd};
  HostStage in(/*packed=*/true, /*tight=*/true), out;
  in.up(&p.start_ns, start_ns, n);
  in.up(&p.ids, ids, n);
  out.down(&p.status, status, ticks);
  for (int a = 0; a < 3; a++) {
    if (dst[a]) values[a].resize(ticks * D);
    out.down(dev[a], dst[a] ? values[a].data() : nullptr, ticks * D);
  }
  if (in.upload(bs->in, st) || out.upload(bs->out, st)) return TPAMD_E_HIP;
  p.count = count; p.num_ticks = num_ticks; p.step_ns = step_ns;
  hipLaunchKernelGGL(k_pset_sample_at_ticks, dim3((unsigned)((ticks + 255) / 256)), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  if (int rc = out.download(st)) return rc;
  for (int a = 0; a < 3; a++) {    // only the OK ticks reach the caller's arrays
    if (!dst[a]) continue;
    for (size_t i = 0; i < ticks; i++)
      if (status[i] == TPAMD_PLAN_OK) std::memcpy(dst[a] + i * D, values[a].data() + i * D, D * 8);
  }
  return 0;
}

int tpamd_buffer_set_sample_at_ticks_device(tpamd_buffer_set *bs, int count, const int32_t *ids,
                                            const int64_t *start_ns, int64_t step_ns, int num_ticks, double *q,
                                            double *qd, double *qdd, int32_t *status, void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, false) || !start_ns || !status || step_ns <= 0 || num_ticks < 1)
    return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) return 0;
  const size_t ticks = (size_t)count * num_ticks;
  if ((ticks + 255) / 256 > 0x7fffffff) return TPAMD_E_UNSUPPORTED;
  TPAMD_ON_DEVICE(bs->e);
  ReadoutParams p = bset_readout_params(bs);
  p.count = count; p.num_ticks = num_ticks; p.ids = ids;
  p.start_ns = (const long long *)start_ns; p.step_ns = step_ns;
  p.q = q; p.qd = qd; p.qdd = qdd; p.status = status;
  hipLaunchKernelGGL(k_pset_sample_at_ticks, dim3((unsigned)((ticks + 255) / 256)), dim3(256), 0,
                     (hipStream_t)hip_stream, p);
  HIPCHK(hipGetLastError());
  return 0;
}

int tpamd_buffer_set_download(tpamd_buffer_set *bs, int count, const int32_t *ids, int64_t *offsets,
                              int64_t capacity, double *time, double *q, double *qd, double *qdd) {
  if (!bset_list_ok(bs, count, ids, true, false) || !offsets || capacity < 0) return TPAMD_E_INVALID_ARGUMENT;
  if (count == 0) {
    offsets[0] = 0;
    return 0;
  }
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = nullptr;
  const size_t n = count, D = bs->S.D;
  ReadoutParams p = bset_readout_params(bs);
  HostStage in(/*packed=*/false, /*tight=*/true);
  in.down(&p.offsets, offsets, n + 1);
  in.up(&p.ids, ids, n);
  int rc = in.upload(bs->in, st);
  if (rc) return rc;
  p.count = count;
  hipLaunchKernelGGL(k_pset_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, p);
  HIPCHK(hipGetLastError());
  rc = in.download(st);
  if (rc) return rc;
  const size_t rows = (size_t)offsets[count];
  if ((int64_t)rows > capacity) return TPAMD_E_INVALID_ARGUMENT;
  HostStage out;
  out.down(&p.o_time, time, rows);
  out.down(&p.o_q, q, rows * D);
  out.down(&p.o_qd, qd, rows * D);
  out.down(&p.o_qdd, qdd, rows * D);
  if (rows == 0 || out.bytes() == 0) return 0;
  rc = out.upload(bs->out, st);
  if (rc) return rc;
  p.capacity = (long long)rows;
  hipLaunchKernelGGL(k_pset_pack_trajectories, dim3((unsigned)n), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  return out.download(st);
}

int tpamd_buffer_set_download_device(tpamd_buffer_set *bs, int count, const int32_t *ids, int64_t *offsets,
                                     int64_t capacity, double *time, double *q, double *qd, double *qdd,
                                     void *hip_stream) {
  if (!bset_list_ok(bs, count, ids, false, false) || !offsets || capacity < 0) return TPAMD_E_INVALID_ARGUMENT;
  TPAMD_ON_DEVICE(bs->e);
  hipStream_t st = (hipStream_t)hip_stream;
  ReadoutParams p = bset_readout_params(bs);
  p.count = count; p.ids = ids; p.offsets = (long long *)offsets; p.capacity = capacity;
  p.o_time = time; p.o_q = q; p.o_qd = qd; p.o_qdd = qdd;
  hipLaunchKernelGGL(k_pset_scan_offsets, dim3(1), dim3(kScanThreads), 0, st, p);      // offsets[0] = 0 for none
  if (count > 0) hipLaunchKernelGGL(k_pset_pack_trajectories, dim3((unsigned)count), dim3(256), 0, st, p);
  HIPCHK(hipGetLastError());
  return 0;
}

}  // extern "C"

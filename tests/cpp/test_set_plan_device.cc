// GPU test of the enqueued-only Plan of planner sets (run by tests/test_gpu_set_plan_device.py):
// tpamd_planner_set_plan_device / _reserve / _capacity and the mirror's PlanDevice /
// FinishPlanDevice. Every set that goes through plan_device on a non-blocking stream has a twin
// driven through tpamd_planner_set_plan whose max_planning_iterations is max_windows - 1; all
// comparisons are bit for bit (summaries, packed trajectories, stop parameters).
// Shapes: N = 100, delta 0.005, horizon 0.4 s, B = 70 (and one case with B = 130).
//   1. twin equality at D = 3 and 7, both sampling methods, max_windows 1, 2 and 4: a first Plan
//      and three receding-horizon replans of a set that mixes planners without a path, starts
//      outside the trajectory, fresh paths that need 1 and >= 3 windows, erase-only planners,
//      planners at their target and planners after switch_paths;
//   2. a Cartesian set with resident tables (D = 7 and the generic route at D = 4), one table too
//      short (TPAMD_PLAN_INTERNAL in both sets);
//   3. capacity: history_capacity 2 N and trajectory_capacity 16 give RESOURCE_EXHAUSTED for the
//      planners that lack room and leave the others bit-equal to the twin; reserve + reset + new
//      path recovers; reserve in mid-motion changes nothing;
//   4. ordering without synchronisation by the caller, and the four-call control cycle on one stream;
//   5. the call does not wait for the stream; 6. call-level errors.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/path_timing_trajectory_set.h"
#include "test_support.h"

static const int kN = 100;

template <typename T>
struct Dev {       // a device array with a host image
  T *p = nullptr;
  size_t n = 0;
  explicit Dev(size_t count) : n(count) { HIP_OK(hipMalloc((void **)&p, std::max<size_t>(count, 1) * sizeof(T))); }
  ~Dev() { (void)hipFree(p); }
  Dev(const Dev &) = delete;
  void Up(const std::vector<T> &h) { HIP_OK(hipMemcpy(p, h.data(), std::min(n, h.size()) * sizeof(T), hipMemcpyHostToDevice)); }
  std::vector<T> Down() const {
    std::vector<T> h(n);
    HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
};

// Everything the C-ABI shows of a set after a Plan, for bit-for-bit comparison.
struct Snapshot {
  std::vector<tpamd_planner_summary> summary;
  std::vector<int64_t> offsets;
  std::vector<double> rows;          // time, s, sd, sdd, q, qd, qdd packed one after the other
  std::vector<double> stop, duration;
  std::vector<int32_t> stop_status;
};

static Snapshot Take(tpamd_planner_set *ps, int B, int D, const std::vector<tpamd_planner_summary> &summary) {
  Snapshot s;
  s.summary = summary;
  s.offsets.assign(B + 1, 0);
  size_t total = 0;
  for (int b = 0; b < B; b++) total += (size_t)std::max(summary[b].num_samples, 0);
  s.rows.assign(std::max<size_t>(total, 1) * (4 + 3 * D), 0.0);
  double *t = s.rows.data(), *q = t + 4 * total;
  CHECK(tpamd_planner_set_download_trajectories(ps, B, nullptr, s.offsets.data(), (int64_t)total, t, t + total,
                                                t + 2 * total, t + 3 * total, q, q + total * D, q + 2 * total * D) == 0);
  CHECK((size_t)s.offsets[B] == total);
  // the fastest stop 30 ms after each planner's start (one without a plan reports its own status)
  std::vector<int64_t> when(B);
  for (int b = 0; b < B; b++) when[b] = summary[b].start_time_ns + 30 * kMs;
  s.stop.assign(B, -1.0); s.duration.assign(B, -1.0); s.stop_status.assign(B, -1);
  CHECK(tpamd_planner_set_stop_parameters(ps, B, nullptr, when.data(), s.stop.data(), s.duration.data(),
                                          s.stop_status.data()) == 0);
  return s;
}

// planners of `a` that differ from `b` in anything; `only` (may be null) selects the planners looked at
static int Differences(const Snapshot &a, const Snapshot &b, int B, int D, const std::vector<char> *only = nullptr) {
  int bad = 0;
  const size_t ta = (size_t)a.offsets[B], tb = (size_t)b.offsets[B];
  for (int k = 0; k < B; k++) {
    if (only && !(*only)[k]) continue;
    bool same = std::memcmp(&a.summary[k], &b.summary[k], sizeof(tpamd_planner_summary)) == 0;
    const size_t na = (size_t)(a.offsets[k + 1] - a.offsets[k]), nb = (size_t)(b.offsets[k + 1] - b.offsets[k]);
    same = same && na == nb;
    if (same && na > 0) {
      for (int f = 0; f < 4; f++)
        same = same && std::memcmp(&a.rows[f * ta + a.offsets[k]], &b.rows[f * tb + b.offsets[k]], na * 8) == 0;
      for (int f = 0; f < 3; f++)
        same = same && std::memcmp(&a.rows[4 * ta + (f * ta + a.offsets[k]) * D],
                                   &b.rows[4 * tb + (f * tb + b.offsets[k]) * D], na * D * 8) == 0;
    }
    same = same && a.stop_status[k] == b.stop_status[k] && std::memcmp(&a.stop[k], &b.stop[k], 8) == 0 &&
           std::memcmp(&a.duration[k], &b.duration[k], 8) == 0;
    bad += !same;
  }
  return bad;
}

static tpamd_planner_set_config Config(int B, int D, int method, int max_iterations) {
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 4;
  cfg.sampling_method = method; cfg.max_planning_iterations = max_iterations; cfg.constraint_safety = 0.8;
  cfg.max_initial_velocity_error = 1e-2; cfg.time_step_ns = method ? 4 * kMs : kMs;
  return cfg;
}

// Waypoint paths for planners 0 .. count-1: W[k] waypoints each, `span` apart at the most.
struct Paths {
  std::vector<int32_t> offsets{0};
  std::vector<double> wps, vmax, amax, delta;
  void Add(int D, int W, double span) {
    std::vector<double> at(D);
    for (int d = 0; d < D; d++) at[d] = -1.5 + 3.0 * Rnd();
    for (int w = 0; w < W; w++) {
      for (int d = 0; d < D; d++) {
        if (w) at[d] += span * (2.0 * Rnd() - 1.0);
        wps.push_back(at[d]);
      }
    }
    offsets.push_back(offsets.back() + W);
    for (int d = 0; d < D; d++) { vmax.push_back(1.0 + Rnd()); amax.push_back(2.0 + 3.0 * Rnd()); }
    delta.push_back(0.005);
  }
  int Load(tpamd_planner_set *ps, const std::vector<int32_t> *ids = nullptr) const {
    const int n = (int)delta.size();
    std::vector<int32_t> np(n), st(n);
    const int rc = tpamd_planner_set_set_waypoints(ps, n, ids ? ids->data() : nullptr, offsets.data(), wps.data(), 0.2,
                                                   vmax.data(), amax.data(), delta.data(), nullptr, np.data(), st.data());
    for (int k = 0; k < n; k++) CHECK(st[k] == TPAMD_PLAN_OK);
    return rc;
  }
};

// One plan_device call on `stream`, synchronised, with the summaries and the info brought down.
struct AsyncPlan {
  int B;
  Dev<int64_t> start, horizon;
  Dev<tpamd_planner_summary> summary;
  Dev<tpamd_plan_device_info> info;
  explicit AsyncPlan(int B_) : B(B_), start(B_), horizon(B_), summary(B_), info(1) {}
  int Enqueue(tpamd_planner_set *ps, const std::vector<int64_t> &s, const std::vector<int64_t> &h, int max_windows,
              hipStream_t stream) {
    start.Up(s);
    horizon.Up(h);
    return tpamd_planner_set_plan_device(ps, start.p, horizon.p, max_windows, summary.p, info.p, stream);
  }
  int Run(tpamd_planner_set *ps, const std::vector<int64_t> &s, const std::vector<int64_t> &h, int max_windows,
          hipStream_t stream, std::vector<tpamd_planner_summary> *sm, tpamd_plan_device_info *inf) {
    const int rc = Enqueue(ps, s, h, max_windows, stream);
    HIP_OK(hipStreamSynchronize(stream));
    *sm = summary.Down();
    *inf = info.Down()[0];
    return rc;
  }
};

static void CheckInfo(const tpamd_plan_device_info &info, const std::vector<tpamd_planner_summary> &sm) {
  int ok = 0, exhausted = 0, windows = 0;
  for (const auto &r : sm) {
    ok += r.status == TPAMD_PLAN_OK;
    exhausted += r.status == TPAMD_PLAN_RESOURCE_EXHAUSTED;
    windows = std::max(windows, (int)r.windows);
  }
  CHECK(info.num_ok == ok && info.num_failed == (int)sm.size() - ok && info.num_exhausted == exhausted);
  CHECK(info.max_windows_solved == windows);
  if (!exhausted) CHECK(info.needed_history == 0 && info.needed_trajectory == 0);
}

// ---- 1. twin equality
static void TestTwins(tpamd_engine *e, hipStream_t stream, int B, int D, int method, int max_windows) {
  g_seed = 4200 + 17 * D + method;          // the same planners for every max_windows
  const int kNoPath = B - 1, kOutOfRange = 5, kBeforeStart = 6;
  tpamd_planner_set_config cfg = Config(B, D, method, 200), twin_cfg = Config(B, D, method, max_windows - 1);
  tpamd_planner_set *dev = nullptr, *twin = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &dev) == 0 && tpamd_planner_set_create(e, &twin_cfg, &twin) == 0);
  if (!dev || !twin) return;
  // planner kinds: b % 7 == 3 long paths planned far ahead (>= 3 windows); 50 .. 54 short paths
  // (planned to the end in one window: at the target afterwards); b % 3 == 1 replan with a short
  // horizon (planned enough: erase only); 10 .. 14 switch paths before the second replan
  Paths paths;
  for (int b = 0; b < B - 1; b++) {
    if (b % 7 == 3) paths.Add(D, 8, 1.5);
    else if (b >= 50 && b < 55) paths.Add(D, 2, 0.1 / std::sqrt((double)D));
    else paths.Add(D, 2 + (int)(Rnd() * 3.0) % 3, 1.5);
  }
  CHECK(paths.Load(dev) == 0 && paths.Load(twin) == 0);
  CHECK(tpamd_planner_set_reserve(dev, 0, 0) == 0);
  AsyncPlan call(B);
  std::vector<tpamd_planner_summary> sd(B), st(B);
  tpamd_plan_device_info info{};
  int calls = 0, equal = 0, deadline = 0, three = 0, one = 0, erase_only = 0, at_target = 0, switched_ok = 0,
      out_of_range = 0, invalid = 0, no_path = 0;
  for (int round = 0; round < 4; round++) {
    std::vector<int64_t> start(B), horizon(B);
    for (int b = 0; b < B; b++) {
      start[b] = (1000 + 100 * round) * kMs;
      horizon[b] = b % 7 == 3 ? 2000 * kMs : (b % 3 == 0 ? 100 * kMs : 400 * kMs);
      if (round > 0 && b % 3 == 1 && b % 7 != 3) horizon[b] = 10 * kMs;
      if (b == kOutOfRange || b == kBeforeStart) horizon[b] = 100 * kMs;    // one window: they hold a plan
      if (round == 2 && b == kOutOfRange) start[b] = sd[b].end_time_ns + 10000 * kMs;
      if (round == 2 && b == kBeforeStart) start[b] = sd[b].start_time_ns - 50 * kMs;
    }
    if (round == 2) {
      // the online switch at the next start, in both sets (a synchronous host entry)
      std::vector<int32_t> ids = {10, 11, 12, 13, 14}, off = {0}, np(5), ss(5), ss2(5);
      std::vector<int64_t> when(5, start[10]);
      std::vector<double> w, stop(5);
      for (int k = 0; k < 5; k++) {
        const int W = 2 + k % 2;
        for (int j = 0; j < W * D; j++) w.push_back(-1.5 + 3.0 * Rnd());
        off.push_back(off.back() + W);
      }
      CHECK(tpamd_planner_set_switch_paths(dev, 5, ids.data(), when.data(), nullptr, off.data(), w.data(), stop.data(),
                                           np.data(), ss.data()) == 0);
      CHECK(tpamd_planner_set_switch_paths(twin, 5, ids.data(), when.data(), nullptr, off.data(), w.data(), stop.data(),
                                           np.data(), ss2.data()) == 0);
      CHECK(ss == ss2);
      for (int k = 0; k < 5; k++) switched_ok += ss[k] == TPAMD_PLAN_OK;
    }
    CHECK(call.Run(dev, start, horizon, max_windows, stream, &sd, &info) == 0);
    CHECK(tpamd_planner_set_plan(twin, start.data(), horizon.data(), st.data()) == 0);
    size_t up = 1, down = 1;
    tpamd_planner_set_last_plan_bytes(dev, &up, &down);
    CHECK(up == 0 && down == 0);
    CheckInfo(info, sd);
    const Snapshot a = Take(dev, B, D, sd), b = Take(twin, B, D, st);
    const int bad = Differences(a, b, B, D);
    CHECK(bad == 0);
    if (bad) std::printf("  B %d D %d method %d max_windows %d round %d: %d planners differ\n", B, D, method, max_windows,
                         round, bad);
    calls++;
    equal += B - bad;
    for (int k = 0; k < B; k++) {
      const auto &r = sd[k];
      deadline += r.status == TPAMD_PLAN_DEADLINE_EXCEEDED;
      if (r.status == TPAMD_PLAN_DEADLINE_EXCEEDED) CHECK(st[k].status == TPAMD_PLAN_DEADLINE_EXCEEDED && r.windows == max_windows);
      three += r.windows >= 3;
      one += round == 0 && r.status == TPAMD_PLAN_OK && r.windows == 1;
      erase_only += round > 0 && r.status == TPAMD_PLAN_OK && r.windows == 0 && r.num_samples > 0 && !r.target_reached;
      at_target += r.status == TPAMD_PLAN_OK && r.target_reached && r.path_state == 3;
      out_of_range += r.status == TPAMD_PLAN_OUT_OF_RANGE;
      invalid += k == kBeforeStart && r.status == TPAMD_PLAN_INVALID_ARGUMENT;
      no_path += k == kNoPath && r.status == TPAMD_PLAN_FAILED_PRECONDITION;
      CHECK(r.windows <= max_windows);
    }
  }
  CHECK(no_path == 4);
  // k_plan_end checks the loop limit before completion (:655-658): with max_windows 1 every planner
  // that solves a window is cut, whatever the window reached
  if (max_windows == 1) CHECK(deadline >= 3 * (B - 1));
  if (max_windows >= 2)
    CHECK(out_of_range >= 1 && invalid >= 1 && one >= 10 && at_target >= 5 && switched_ok >= 3 && erase_only >= 10 &&
          deadline >= B / 7 - 1);                            // the long paths planned 2 s ahead are cut
  if (max_windows == 4) CHECK(three >= 3);
  tpamd_planner_set_destroy(dev);
  tpamd_planner_set_destroy(twin);
  std::printf("plan_device twins (B %d, D %d, method %d, max_windows %d): %d calls, %d planner states bit-equal, "
              "%d cut with DEADLINE_EXCEEDED, %d with >= 3 windows, %d one-window first plans, %d erase-only, %d at the "
              "target, %d switched, %d out of range, %d before the start, %d without a path\n",
              B, D, method, max_windows, calls, equal, deadline, three, one, erase_only, at_target, switched_ok,
              out_of_range, invalid, no_path);
}

// ---- 2. Cartesian sets with resident tables
static void TestCartesian(tpamd_engine *e, hipStream_t stream, int D) {
  const int B = 24, kShort = 7, max_windows = 4;
  g_seed = 880 + D;
  // the tables are samples of waypoint splines: fitted by a joint set, read back, sampled by the engine
  tpamd_planner_set_config jcfg = Config(B, D, 0, 200);
  tpamd_planner_set *fit = nullptr;
  CHECK(tpamd_planner_set_create(e, &jcfg, &fit) == 0);
  if (!fit) return;
  Paths paths;
  for (int b = 0; b < B; b++) paths.Add(D, 3 + b % 3, 0.8);
  CHECK(paths.Load(fit) == 0);
  std::vector<int32_t> off = {0};
  std::vector<double> tq, tJ, pe(B), vm, am, vt(B), vr(B), dl(B);
  int longest = 0;
  for (int b = 0; b < B; b++) {
    int32_t P = 0;
    CHECK(tpamd_planner_set_download_path(fit, b, &P, nullptr, nullptr, 0) == 0 && P >= 3);
    std::vector<double> knots(P + 3), cps((size_t)P * D);
    CHECK(tpamd_planner_set_download_path(fit, b, &P, knots.data(), cps.data(), P) == 0);
    pe[b] = knots[P + 2];
    dl[b] = (b % 2 ? 0.3 : 0.45) * pe[b] / (kN - 1);
    int rows = (int)std::lround(pe[b] / dl[b]) + kN + 1;
    std::vector<double> q((size_t)rows * D), q1(q.size()), q2(q.size());
    const double zero = 0.0;
    CHECK(tpamd_sample_joint_paths_host(e, 1, D, rows, P, knots.data(), cps.data(), &zero, &dl[b], q.data(), q1.data(),
                                        q2.data()) == 0);
    if (b == kShort) rows = kN + 2;            // its second window is not resident
    longest = std::max(longest, rows);
    for (int r = 0; r < rows; r++) {
      for (int d = 0; d < D; d++) tq.push_back(q[(size_t)r * D + d]);
      for (int c = 0; c < 6; c++)
        for (int d = 0; d < D; d++)
          tJ.push_back(0.2 * std::sin(q[(size_t)r * D + d] * (c + 1.0) + 0.31 * d) + (c == d ? 1.0 : 0.0));
    }
    off.push_back(off.back() + rows);
    for (int d = 0; d < D; d++) { vm.push_back(0.5 + 0.6 * Rnd()); am.push_back(1.2 + 1.8 * Rnd()); }
    vt[b] = 0.3 + 0.3 * Rnd();
    vr[b] = 0.8 + 0.4 * Rnd();
  }
  tpamd_planner_set_destroy(fit);
  std::vector<int32_t> state(B, 1);
  tpamd_planner_set_config cfg = Config(B, D, 0, 200), twin_cfg = Config(B, D, 0, max_windows - 1);
  cfg.time_step_ns = twin_cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *dev = nullptr, *twin = nullptr;
  CHECK(tpamd_planner_set_create_cartesian(e, &cfg, longest, &dev) == 0);
  CHECK(tpamd_planner_set_create_cartesian(e, &twin_cfg, longest, &twin) == 0);
  if (!dev || !twin) return;
  for (tpamd_planner_set *ps : {dev, twin})
    CHECK(tpamd_planner_set_upload_ik_tables(ps, B, nullptr, off.data(), tq.data(), tJ.data(), pe.data(), vm.data(),
                                             am.data(), vt.data(), vr.data(), dl.data(), nullptr, state.data()) == 0);
  CHECK(tpamd_planner_set_reserve(dev, 0, 0) == 0);
  AsyncPlan call(B);
  std::vector<tpamd_planner_summary> sd(B), st(B);
  tpamd_plan_device_info info{};
  int equal = 0, ok = 0, internal = 0, several = 0;
  for (int round = 0; round < 3; round++) {
    // 750 ms ahead; every third planner far enough ahead for several windows, the short table's among them
    std::vector<int64_t> start(B, (int64_t)(200 * round) * kMs), horizon(B, 750 * kMs);
    for (int b = 1; b < B; b += 3) horizon[b] = 6000 * kMs;
    CHECK(call.Run(dev, start, horizon, max_windows, stream, &sd, &info) == 0);
    CHECK(tpamd_planner_set_plan(twin, start.data(), horizon.data(), st.data()) == 0);
    CheckInfo(info, sd);
    const int bad = Differences(Take(dev, B, D, sd), Take(twin, B, D, st), B, D);
    CHECK(bad == 0);
    equal += B - bad;
    for (int b = 0; b < B; b++) {
      ok += sd[b].status == TPAMD_PLAN_OK;
      several += sd[b].windows >= 2;
    }
    internal += sd[kShort].status == TPAMD_PLAN_INTERNAL && st[kShort].status == TPAMD_PLAN_INTERNAL;
  }
  CHECK(internal >= 1 && ok >= B && several >= 3);
  tpamd_planner_set_destroy(dev);
  tpamd_planner_set_destroy(twin);
  std::printf("plan_device Cartesian (D %d): 3 calls, %d planner states bit-equal, %d OK plans, %d of several windows, the "
              "short table INTERNAL in both sets %d times\n", D, equal, ok, several, internal);
}

// ---- 3. capacity
static void TestCapacity(tpamd_engine *e, hipStream_t stream, bool history) {
  const int B = 70, D = 7, method = history ? 0 : 1, max_windows = 6;
  g_seed = history ? 311 : 312;
  tpamd_planner_set_config cfg = Config(B, D, method, 200), twin_cfg = Config(B, D, method, max_windows - 1);
  if (history) cfg.history_capacity = 2 * kN; else cfg.trajectory_capacity = 16;
  tpamd_planner_set *dev = nullptr, *twin = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &dev) == 0 && tpamd_planner_set_create(e, &twin_cfg, &twin) == 0);
  if (!dev || !twin) return;
  int32_t cap = 0, tcap = 0;
  CHECK(tpamd_planner_set_capacity(dev, &cap, &tcap) == 0);
  CHECK(history ? cap == 2 * kN : tcap == 16);
  // history: every fifth planner runs a long path planned 1.2 s ahead, the others need one window.
  // trajectory: every fifth planner's path is so short that its trajectory has at most 16 samples.
  Paths paths;
  std::vector<int64_t> start(B, 500 * kMs), horizon(B);
  for (int b = 0; b < B; b++) {
    const bool special = b % 5 == 0;
    if (history) paths.Add(D, special ? 8 : 3, 1.5);
    else paths.Add(D, 2, special ? 2e-4 : 1.0);
    horizon[b] = history ? (special ? 1200 * kMs : 100 * kMs) : 400 * kMs;
  }
  CHECK(paths.Load(dev) == 0 && paths.Load(twin) == 0);
  AsyncPlan call(B);
  std::vector<tpamd_planner_summary> sd(B), st(B);
  tpamd_plan_device_info info{};
  CHECK(call.Run(dev, start, horizon, max_windows, stream, &sd, &info) == 0);
  CHECK(tpamd_planner_set_plan(twin, start.data(), horizon.data(), st.data()) == 0);
  CheckInfo(info, sd);
  std::vector<char> exhausted(B, 0), others(B, 0);
  int n_ex = 0, needed = 0;
  for (int b = 0; b < B; b++) {
    exhausted[b] = sd[b].status == TPAMD_PLAN_RESOURCE_EXHAUSTED;
    others[b] = !exhausted[b];
    n_ex += exhausted[b];
    if (!exhausted[b]) continue;
    CHECK(history ? b % 5 == 0 : b % 5 != 0);
    if (history) {
      CHECK(sd[b].history_count <= cap && sd[b].history_count + kN > cap);
      needed = std::max(needed, sd[b].history_count + kN);
    } else {
      CHECK(sd[b].num_samples == 0 && st[b].status == TPAMD_PLAN_OK && st[b].num_samples > tcap);
      needed = std::max(needed, (int)st[b].num_samples);
    }
  }
  CHECK(n_ex >= 5 && n_ex < B && info.num_exhausted == n_ex);
  if (history) CHECK(info.needed_history == needed && needed > cap && info.needed_trajectory == 0);
  else CHECK(info.needed_trajectory == needed && info.needed_history == 0);
  CHECK(Differences(Take(dev, B, D, sd), Take(twin, B, D, st), B, D, &others) == 0);
  // the recovery: reserve what info asks for, reset the planners, the path again, plan again -- until
  // nobody lacks room (a history grows by one window's worth per round, a trajectory fits at once)
  std::vector<char> affected = exhausted;
  int rounds = 0;
  for (; rounds < 12 && info.num_exhausted > 0; rounds++) {
    CHECK(tpamd_planner_set_reserve(dev, info.needed_history, info.needed_trajectory) == 0);
    int32_t c2 = 0, t2 = 0;
    CHECK(tpamd_planner_set_capacity(dev, &c2, &t2) == 0);
    CHECK(c2 >= info.needed_history && t2 >= info.needed_trajectory && c2 >= cap && t2 >= tcap);
    std::vector<int32_t> ids;
    Paths again;
    for (int b = 0; b < B; b++) {
      if (!affected[b]) continue;           // all of them again: each ends with one Plan on a new path
      ids.push_back(b);
      again.offsets.push_back(again.offsets.back() + paths.offsets[b + 1] - paths.offsets[b]);
      again.wps.insert(again.wps.end(), paths.wps.begin() + (size_t)paths.offsets[b] * D,
                       paths.wps.begin() + (size_t)paths.offsets[b + 1] * D);
      again.vmax.insert(again.vmax.end(), paths.vmax.begin() + (size_t)b * D, paths.vmax.begin() + (size_t)(b + 1) * D);
      again.amax.insert(again.amax.end(), paths.amax.begin() + (size_t)b * D, paths.amax.begin() + (size_t)(b + 1) * D);
      again.delta.push_back(paths.delta[b]);
    }
    CHECK(tpamd_planner_set_reset(dev, (int)ids.size(), ids.data()) == 0);
    CHECK(again.Load(dev, &ids) == 0);
    CHECK(call.Run(dev, start, horizon, max_windows, stream, &sd, &info) == 0);
  }
  CHECK(info.num_exhausted == 0 && rounds >= 1);
  // a fresh twin: the affected planners alone, the same path and the same one Plan
  tpamd_planner_set *fresh = nullptr;
  CHECK(tpamd_planner_set_create(e, &twin_cfg, &fresh) == 0);
  if (fresh) {
    CHECK(paths.Load(fresh) == 0);
    CHECK(tpamd_planner_set_plan(fresh, start.data(), horizon.data(), st.data()) == 0);
    CHECK(Differences(Take(dev, B, D, sd), Take(fresh, B, D, st), B, D, &affected) == 0);
    int ok = 0;
    for (int b = 0; b < B; b++) ok += affected[b] && sd[b].status == TPAMD_PLAN_OK;
    if (!history) CHECK(ok == n_ex);        // (a long path may still meet the loop limit of max_windows)
    // reserve in mid-motion: the next synchronous Plan of the reserved set is the unreserved twin's
    tpamd_planner_set *mid = nullptr;
    CHECK(tpamd_planner_set_create(e, &twin_cfg, &mid) == 0);
    if (mid) {
      std::vector<tpamd_planner_summary> sm(B);
      CHECK(paths.Load(mid) == 0);
      CHECK(tpamd_planner_set_plan(mid, start.data(), horizon.data(), sm.data()) == 0);
      int32_t c0 = 0, t0 = 0, c1 = 0, t1 = 0;
      CHECK(tpamd_planner_set_capacity(mid, &c0, &t0) == 0);
      CHECK(tpamd_planner_set_reserve(mid, 3 * c0 + 7, 2 * t0 + 3) == 0);
      CHECK(tpamd_planner_set_reserve(mid, c0, 1) == 0);          // never shrinks
      CHECK(tpamd_planner_set_capacity(mid, &c1, &t1) == 0);
      CHECK(c1 == 3 * c0 + 7 && t1 == 2 * t0 + 3);
      std::vector<int64_t> next(B, 600 * kMs);
      CHECK(tpamd_planner_set_plan(mid, next.data(), horizon.data(), sm.data()) == 0);
      CHECK(tpamd_planner_set_plan(fresh, next.data(), horizon.data(), st.data()) == 0);
      CHECK(Differences(Take(mid, B, D, sm), Take(fresh, B, D, st), B, D) == 0);
      tpamd_planner_set_destroy(mid);
    }
    tpamd_planner_set_destroy(fresh);
  }
  tpamd_planner_set_destroy(dev);
  tpamd_planner_set_destroy(twin);
  std::printf("plan_device capacity (%s): %d planners RESOURCE_EXHAUSTED, needed %d (capacity %d), the others bit-equal "
              "to the twin; recovered in %d rounds of reserve / reset / path / plan, equal to a fresh twin; reserve in "
              "mid-motion changes nothing\n", history ? "history" : "trajectory", n_ex, needed, history ? cap : tcap, rounds);
}

// ---- 4. ordering, 5. no waiting, 6. call-level errors
struct HostGate {
  std::atomic<int> open{0}, released{0}, timed_out{0};
};
static void WaitForGate(void *p) {
  HostGate *g = (HostGate *)p;
  const auto t0 = std::chrono::steady_clock::now();
  while (!g->open.load()) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(1)) { g->timed_out = 1; return; }
    std::this_thread::yield();
  }
  g->released = 1;
}

// setpoints of the ticks that are OK (the values of the others are left as they were)
static bool SameSetpoints(const std::vector<int32_t> &sa, const std::vector<int32_t> &sb, const std::vector<double> &a,
                          const std::vector<double> &b, int D) {
  if (sa != sb || a.size() != b.size()) return false;
  for (size_t k = 0; k < sa.size(); k++)
    if (sa[k] == TPAMD_PLAN_OK && std::memcmp(&a[k * D], &b[k * D], D * 8) != 0) return false;
  return true;
}

static void TestOrdering(tpamd_engine *e, hipStream_t stream) {
  const int B = 70, D = 7, max_windows = 6, T = 8;
  const int cycle_windows = 16;     // a path that starts in mid-motion, through its stopping point, takes many short windows
  g_seed = 505;
  hipStream_t second = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&second, hipStreamNonBlocking));
  tpamd_planner_set_config cfg = Config(B, D, 0, 200), twin_cfg = Config(B, D, 0, max_windows - 1);
  const tpamd_planner_set_config cycle_cfg = Config(B, D, 0, cycle_windows - 1);
  tpamd_planner_set *A = nullptr, *At = nullptr, *Bs = nullptr, *Bt = nullptr, *Cd = nullptr, *Cs = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &A) == 0 && tpamd_planner_set_create(e, &twin_cfg, &At) == 0);
  CHECK(tpamd_planner_set_create(e, &cfg, &Bs) == 0 && tpamd_planner_set_create(e, &cfg, &Bt) == 0);
  CHECK(tpamd_planner_set_create(e, &cfg, &Cd) == 0 && tpamd_planner_set_create(e, &cycle_cfg, &Cs) == 0);
  tpamd_buffer_set *bd = nullptr, *bs = nullptr;
  CHECK(tpamd_buffer_set_create(e, B, D, 2048, 1e-6, &bd) == 0 && tpamd_buffer_set_create(e, B, D, 2048, 1e-6, &bs) == 0);
  if (!A || !At || !Bs || !Bt || !Cd || !Cs || !bd || !bs) return;
  Paths pa, pb;
  for (int b = 0; b < B; b++) { pa.Add(D, 3, 1.5); pb.Add(D, 4, 1.5); }
  std::vector<int64_t> s0(B, 1000 * kMs), s1(B, 1100 * kMs), hz(B, 300 * kMs);
  std::vector<tpamd_planner_summary> sm(B), sa(B), sat(B), sb(B), sbt(B);
  AsyncPlan call(B);
  tpamd_plan_device_info info{};
  for (tpamd_planner_set *ps : {A, At, Cd, Cs}) {
    CHECK(pa.Load(ps) == 0);
    if (ps == A || ps == Cd) CHECK(call.Run(ps, s0, hz, ps == A ? max_windows : cycle_windows, stream, &sm, &info) == 0);
    else CHECK(tpamd_planner_set_plan(ps, s0.data(), hz.data(), sm.data()) == 0);
  }
  for (tpamd_planner_set *ps : {Bs, Bt}) {
    CHECK(pb.Load(ps) == 0);
    CHECK(tpamd_planner_set_plan(ps, s0.data(), hz.data(), sm.data()) == 0);
  }
  // (a) plan_device on A (stream), at once the synchronous Plan of B on the same engine, then a
  // device readout of A on a second stream; nothing is synchronised in between
  Dev<int64_t> ticks(B);
  Dev<double> q((size_t)B * T * D), qd((size_t)B * T * D), qdd((size_t)B * T * D);
  Dev<int32_t> status((size_t)B * T);
  std::vector<int64_t> t0(B, 1120 * kMs);
  ticks.Up(t0);
  HIP_OK(hipMemset(q.p, 0xff, q.n * 8)); HIP_OK(hipMemset(qd.p, 0xff, qd.n * 8)); HIP_OK(hipMemset(qdd.p, 0xff, qdd.n * 8));
  HIP_OK(hipMemset(status.p, 0xff, status.n * 4));
  HIP_OK(hipDeviceSynchronize());
  CHECK(call.Enqueue(A, s1, hz, max_windows, stream) == 0);
  CHECK(tpamd_planner_set_plan(Bs, s1.data(), hz.data(), sb.data()) == 0);
  CHECK(tpamd_planner_set_sample_at_ticks_device(A, B, nullptr, ticks.p, 4 * kMs, T, q.p, qd.p, qdd.p, status.p, second) == 0);
  HIP_OK(hipStreamSynchronize(second));
  HIP_OK(hipStreamSynchronize(stream));
  sa = call.summary.Down();
  CHECK(tpamd_planner_set_plan(At, s1.data(), hz.data(), sat.data()) == 0);
  CHECK(tpamd_planner_set_plan(Bt, s1.data(), hz.data(), sbt.data()) == 0);
  std::vector<double> hq(q.n), hqd(q.n), hqdd(q.n);
  std::vector<int32_t> hst(status.n);
  CHECK(tpamd_planner_set_sample_at_ticks(At, B, nullptr, t0.data(), 4 * kMs, T, hq.data(), hqd.data(), hqdd.data(),
                                          hst.data()) == 0);
  const int bad_a = Differences(Take(A, B, D, sa), Take(At, B, D, sat), B, D);
  const int bad_b = Differences(Take(Bs, B, D, sb), Take(Bt, B, D, sbt), B, D);
  CHECK(bad_a == 0 && bad_b == 0);
  int ticks_ok = 0;
  for (int32_t v : hst) ticks_ok += v == TPAMD_PLAN_OK;
  CHECK(ticks_ok > B * T / 2);
  const bool readout = SameSetpoints(status.Down(), hst, q.Down(), hq, D) && SameSetpoints(status.Down(), hst, qd.Down(), hqd, D) &&
                       SameSetpoints(status.Down(), hst, qdd.Down(), hqdd, D);
  CHECK(readout);
  std::printf("plan_device ordering: plan_device on A, Plan of B and a device readout of A on a second stream, "
              "unsynchronised: %d + %d planners differ from their twins, readout %s (%d ticks OK)\n", bad_a, bad_b,
              readout ? "equal" : "DIFFERENT", ticks_ok);
  // (b) one control cycle on one stream, one synchronisation at its end
  std::vector<int32_t> ids(B), roff = {0};
  std::vector<int64_t> when(B, 1100 * kMs);
  std::vector<double> rw, rv, ra, rd(B, 0.005);
  for (int b = 0; b < B; b++) {
    ids[b] = b;
    for (int j = 0; j < 2 * D; j++) rw.push_back(-1.5 + 3.0 * Rnd());
    roff.push_back(roff.back() + 2);
    for (int j = 0; j < D; j++) { rv.push_back(1.0 + Rnd()); ra.push_back(2.0 + 3.0 * Rnd()); }
  }
  Dev<int64_t> d_when(B);
  Dev<double> d_w(rw.size()), d_v(rv.size()), d_a(ra.size()), d_dl(B);
  Dev<int32_t> d_np(B), d_rs(B), d_is(B);
  d_when.Up(when); d_w.Up(rw); d_v.Up(rv); d_a.Up(ra); d_dl.Up(rd);
  HIP_OK(hipMemset(q.p, 0xff, q.n * 8)); HIP_OK(hipMemset(qd.p, 0xff, qd.n * 8)); HIP_OK(hipMemset(qdd.p, 0xff, qdd.n * 8));
  HIP_OK(hipMemset(status.p, 0xff, status.n * 4));
  call.start.Up(s1);
  call.horizon.Up(hz);
  HIP_OK(hipDeviceSynchronize());
  CHECK(tpamd_planner_set_retarget_device(Cd, B, ids.data(), d_when.p, roff.data(), d_w.p, 0.2, d_v.p, d_a.p, d_dl.p,
                                          d_a.p, d_np.p, d_rs.p, nullptr, nullptr, nullptr, stream) == 0);
  CHECK(tpamd_planner_set_plan_device(Cd, call.start.p, call.horizon.p, cycle_windows, call.summary.p, call.info.p,
                                      stream) == 0);
  CHECK(tpamd_buffer_set_insert_from_planner_set_device(bd, Cd, B, nullptr, nullptr, d_is.p, stream) == 0);
  CHECK(tpamd_buffer_set_sample_at_ticks_device(bd, B, nullptr, ticks.p, 4 * kMs, T, q.p, qd.p, qdd.p, status.p,
                                                stream) == 0);
  HIP_OK(hipStreamSynchronize(stream));
  std::vector<int32_t> np_h(B), rs_h(B), is_h(B);
  CHECK(tpamd_planner_set_retarget(Cs, B, ids.data(), when.data(), roff.data(), rw.data(), 0.2, rv.data(), ra.data(),
                                   rd.data(), ra.data(), np_h.data(), rs_h.data(), nullptr, nullptr, nullptr) == 0);
  CHECK(tpamd_planner_set_plan(Cs, s1.data(), hz.data(), sat.data()) == 0);
  CHECK(tpamd_buffer_set_insert_from_planner_set(bs, Cs, B, nullptr, nullptr, is_h.data()) == 0);
  CHECK(tpamd_buffer_set_sample_at_ticks(bs, B, nullptr, t0.data(), 4 * kMs, T, hq.data(), hqd.data(), hqdd.data(),
                                         hst.data()) == 0);
  int retargeted = 0, planned = 0;
  const std::vector<tpamd_planner_summary> sc = call.summary.Down();
  for (int b = 0; b < B; b++) { retargeted += rs_h[b] == TPAMD_PLAN_OK; planned += sc[b].status == TPAMD_PLAN_OK; }
  ticks_ok = 0;
  for (int32_t v : hst) ticks_ok += v == TPAMD_PLAN_OK;
  const bool cycle = d_rs.Down() == rs_h && d_np.Down() == np_h && d_is.Down() == is_h && SameSetpoints(status.Down(), hst, q.Down(), hq, D) &&
                     SameSetpoints(status.Down(), hst, qd.Down(), hqd, D) && SameSetpoints(status.Down(), hst, qdd.Down(), hqdd, D) &&
                     std::memcmp(sc.data(), sat.data(), B * sizeof(tpamd_planner_summary)) == 0;
  CHECK(cycle);
  if (!cycle) {
    const std::vector<int32_t> a1 = d_rs.Down(), a2 = d_np.Down(), a3 = d_is.Down(), a4 = status.Down();
    std::printf("  cycle: retarget status %d, points %d, insert status %d, tick status %d, q %d, summaries %d equal; "
                "planner 0: status %d / %d, windows %d / %d, samples %d / %d, insert %d / %d, tick %d / %d\n", a1 == rs_h,
                a2 == np_h, a3 == is_h, a4 == hst, (int)SameSetpoints(a4, hst, q.Down(), hq, D),
                std::memcmp(sc.data(), sat.data(), B * sizeof(tpamd_planner_summary)) == 0, sc[0].status, sat[0].status,
                sc[0].windows, sat[0].windows, sc[0].num_samples, sat[0].num_samples, a3[0], is_h[0], a4[0], hst[0]);
  }
  CHECK(retargeted >= B / 2 && planned >= B / 2 && ticks_ok > B * T / 2);
  std::printf("plan_device cycle: retarget_device -> plan_device -> insert_from_planner_set_device -> sample_at_ticks_device "
              "on one stream, one synchronisation: setpoints %s the synchronous cycle's (%d retargeted, %d planned, %d "
              "ticks OK)\n", cycle ? "bit-equal to" : "DIFFER from", retargeted, planned, ticks_ok);
  // 5. the call does not wait: a host function holds the stream until the test opens the gate
  HostGate gate;
  std::vector<int64_t> s2(B, 1200 * kMs);
  call.start.Up(s2);
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipLaunchHostFunc(stream, WaitForGate, &gate));
  const int rc = tpamd_planner_set_plan_device(A, call.start.p, call.horizon.p, max_windows, call.summary.p, call.info.p,
                                               stream);
  const bool returned_early = !gate.released.load() && !gate.timed_out.load();
  size_t up = 1, down = 1;
  tpamd_planner_set_last_plan_bytes(A, &up, &down);
  gate.open = 1;
  HIP_OK(hipStreamSynchronize(stream));
  CHECK(rc == 0 && returned_early && gate.released.load() == 1 && gate.timed_out.load() == 0 && up == 0 && down == 0);
  sa = call.summary.Down();
  CHECK(tpamd_planner_set_plan(At, s2.data(), hz.data(), sat.data()) == 0);
  const int bad_w = Differences(Take(A, B, D, sa), Take(At, B, D, sat), B, D);
  CHECK(bad_w == 0);
  std::printf("plan_device does not wait: returned with the stream held by a host function (released %d, timed out %d), "
              "0 / 0 bytes over PCIe, %d planners differ from the twin afterwards\n", gate.released.load(),
              gate.timed_out.load(), bad_w);
  // 6. call-level errors change nothing
  CHECK(tpamd_planner_set_plan_device(nullptr, call.start.p, call.horizon.p, 2, nullptr, nullptr, stream) ==
        TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_plan_device(A, nullptr, call.horizon.p, 2, nullptr, nullptr, stream) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_plan_device(A, call.start.p, nullptr, 2, nullptr, nullptr, stream) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_plan_device(A, call.start.p, call.horizon.p, 0, nullptr, nullptr, stream) ==
        TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_plan_device(A, call.start.p, call.horizon.p, -3, call.summary.p, call.info.p, stream) ==
        TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_reserve(nullptr, 1, 1) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_capacity(nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  HIP_OK(hipStreamSynchronize(stream));
  const int bad_e = Differences(Take(A, B, D, sa), Take(At, B, D, sat), B, D);
  // ... and the next Plan, with NULL summary and info, is the twin's
  std::vector<int64_t> s3(B, 1300 * kMs);
  call.start.Up(s3);
  CHECK(tpamd_planner_set_plan_device(A, call.start.p, call.horizon.p, max_windows, nullptr, nullptr, stream) == 0);
  HIP_OK(hipStreamSynchronize(stream));
  CHECK(tpamd_planner_set_plan(At, s3.data(), hz.data(), sat.data()) == 0);
  // the summaries of A are not known to the host (NULL): the twin's sample counts size the download
  const int bad_n = Differences(Take(A, B, D, sat), Take(At, B, D, sat), B, D);
  CHECK(bad_e == 0 && bad_n == 0);
  std::printf("plan_device call-level errors: 7 refused, %d planners changed, %d differ after the next Plan\n", bad_e, bad_n);
  tpamd_buffer_set_destroy(bd);
  tpamd_buffer_set_destroy(bs);
  for (tpamd_planner_set *ps : {A, At, Bs, Bt, Cd, Cs}) tpamd_planner_set_destroy(ps);
  HIP_OK(hipStreamDestroy(second));
}

// ---- the mirror: PlanDevice / FinishPlanDevice against Plan on a twin
static void TestMirror(hipStream_t stream) {
  using namespace trajectory_planning;
  using tpamd::compat::FromUnixNanos;
  using tpamd::compat::Milliseconds;
  using tpamd::compat::Nanoseconds;
  using tpamd::compat::StatusCode;
  using tpamd::compat::ToUnixNanos;
  const int B = 70, D = 7, max_windows = 2;
  g_seed = 99;
  PathTimingTrajectoryOptions opt, twin_opt;
  opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(1));
  twin_opt.SetNumDofs(D).SetNumPathSamples(kN).SetTimeStep(Milliseconds(1)).SetMaxPlanningLoops(max_windows - 1);
  PathTimingTrajectorySet dev(opt, B, 10), twin(twin_opt, B, 10);
  CHECK(dev.status().ok() && twin.status().ok());
  if (!dev.status().ok() || !twin.status().ok()) return;
  std::vector<size_t> all;
  std::vector<std::vector<VectorXd>> wps(B);
  std::vector<VectorXd> vmax(B, VectorXd(D)), amax(B, VectorXd(D));
  for (int b = 0; b < B; b++) {
    all.push_back(b);
    for (int w = 0; w < 3; w++) {
      VectorXd p(D);
      for (int d = 0; d < D; d++) p[d] = -1.5 + 3.0 * Rnd();
      wps[b].push_back(p);
    }
    for (int d = 0; d < D; d++) { vmax[b][d] = 1.0 + Rnd(); amax[b][d] = 2.0 + 3.0 * Rnd(); }
  }
  for (PathTimingTrajectorySet *s : {&dev, &twin})
    for (const auto &st : s->SetWaypointPaths(all, wps, vmax, amax, {}, 0.2, 0.005)) CHECK(st.ok());
  int h0 = 0, t0 = 0, h1 = 0, t1 = 0;
  CHECK(dev.GetCapacity(&h0, &t0).ok() && dev.Reserve(h0 + 50, 0).ok() && dev.GetCapacity(&h1, &t1).ok());
  CHECK(h1 == h0 + 50 && t1 == t0);
  Dev<int64_t> d_start(B), d_horizon(B);
  int equal = 0, stale = 0;
  for (int round = 0; round < 3; round++) {
    std::vector<int64_t> s(B, (1000 + 100 * round) * kMs), h(B, 400 * kMs);
    d_start.Up(s);
    d_horizon.Up(h);
    CHECK(dev.PlanDevice(d_start.p, d_horizon.p, max_windows, stream).ok());
    CHECK(dev.PlanDevicePending());
    PlannedTrajectory none;
    stale += dev.GetTrajectory(0, &none).code() == StatusCode::kFailedPrecondition;
    CHECK(dev.PlanDevice(d_start.p, d_horizon.p, max_windows, stream).code() == StatusCode::kFailedPrecondition);
    const auto got = dev.FinishPlanDevice();
    const auto want = twin.Plan(std::vector<Time>(B, FromUnixNanos(s[0])), std::vector<Duration>(B, Nanoseconds(h[0])));
    CHECK(!dev.PlanDevicePending() && dev.LastPlanDeviceInfo().num_ok + dev.LastPlanDeviceInfo().num_failed == B);
    for (int b = 0; b < B; b++) {
      PlannedTrajectory a, c;
      bool same = got[b].code() == want[b].code() && dev.GetNumTimeSamples(b) == twin.GetNumTimeSamples(b) &&
                  ToUnixNanos(dev.GetEndTime(b)) == ToUnixNanos(twin.GetEndTime(b)) &&
                  ToUnixNanos(dev.GetFinalDecelStart(b)) == ToUnixNanos(twin.GetFinalDecelStart(b)) &&
                  dev.IsTrajectoryAtEnd(b) == twin.IsTrajectoryAtEnd(b) &&
                  dev.WindowsOfLastPlan(b) == twin.WindowsOfLastPlan(b);
      same = same && dev.GetTrajectory(b, &a).ok() && twin.GetTrajectory(b, &c).ok() && a.time.size() == c.time.size();
      same = same && (a.time.empty() || (std::memcmp(a.time.data(), c.time.data(), a.time.size() * 8) == 0 &&
                                         std::memcmp(a.positions.data(), c.positions.data(), a.positions.size() * 8) == 0 &&
                                         std::memcmp(a.velocities.data(), c.velocities.data(), a.velocities.size() * 8) == 0));
      equal += same;
    }
  }
  CHECK(equal == 3 * B && stale == 3);
  CHECK(dev.FinishPlanDevice()[0].code() == StatusCode::kFailedPrecondition);
  std::printf("plan_device mirror: PlanDevice + FinishPlanDevice = Plan on a twin for %d planner states, getters refused "
              "%d times while a call was in flight\n", equal, stale);
}

int main() {
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) { std::printf("no engine\n"); return 1; }
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  for (int D : {3, 7})
    for (int method : {0, 1})
      for (int max_windows : {1, 2, 4}) TestTwins(e, stream, 70, D, method, max_windows);
  TestTwins(e, stream, 130, 7, 0, 2);
  TestCartesian(e, stream, 7);
  TestCartesian(e, stream, 4);
  TestCapacity(e, stream, /*history=*/true);
  TestCapacity(e, stream, /*history=*/false);
  TestOrdering(e, stream);
  TestMirror(stream);
  HIP_OK(hipStreamDestroy(stream));
  tpamd_engine_destroy(e);
  if (g_fail) {
    std::printf("%d FAILURES\n", g_fail);
    return 1;
  }
  std::printf("ALL OK\n");
  return 0;
}

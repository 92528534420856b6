// GPU test of streaming IK tables through the C-ABI (run by tests/test_gpu_cartesian_stream.py):
// tpamd_planner_set_plan_streaming / _plan_resume / _append_ik_rows[_device] on Cartesian sets that
// start from the first N rows of every table, against one oracle IK-table planner per planner on the
// FULL table (oracle/tp_oracle_plan.c) and against a whole-table set, bit for bit.
//
// The synthetic family is that of tests/cpp/test_cartesian_set_gpu.cc at a small shape: B = 32
// planners, N = 64, W in 3..6 waypoints, delta = f kend / (N - 1) with f in {0.4, 0.25} mixed inside
// a set; 4 ms step, 750 ms horizon, a replan every 200 ms until every planner is at its end.
//   exact     1. every suspension is answered with exactly need_count rows cut out of the full table;
//             after every completed Plan the streaming set equals its oracles and the whole-table
//             set; 4. the final tables are the rows appended, never more than BuildIkTable's count
//             and fewer for some; 7. the set starts with table_capacity = N, so the appends double
//             the capacity and the rows before survive; the PCIe bytes of every call
//   ahead     2. need_count + 7 rows per append: equal to `exact`, fewer suspensions
//   short     3. one planner gets need_count - 1 rows: it keeps waiting for one row while the second
//             resume leaves its neighbours' trajectories untouched
//   plan      5. tpamd_planner_set_plan on a short table still gives TPAMD_PLAN_INTERNAL
//   refusals  6. the new entries on a joint set, resume with nobody waiting, a repeated id, a planner
//             without a table; a suspension dropped by reset and by a fresh upload
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "test_support.h"

static const int kN = 64, kB = 32;
static const double kSafety = 0.8, kMaxIvError = 1e-3;
static const int kMaxIter = 10000;

struct Rng {
  unsigned long long s;
  explicit Rng(unsigned long long seed) : s(seed * 2862933555777941757ULL + 3037000493ULL) { next(); next(); }
  double next() {
    s = s * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(s >> 11) / 9007199254740992.0;
  }
  double uniform(double lo, double hi) { return lo + (hi - lo) * next(); }
};

static bool Same(const double *a, const double *b, size_t n) { return n == 0 || std::memcmp(a, b, n * 8) == 0; }

struct Table {
  int D = 0, rows = 0;
  double delta = 0, path_end = 0, vt = 0, vr = 0;
  std::vector<double> q, J, vmax, amax;
};

static void FakeJacobian(const double *q, int rows, int D, std::vector<double> *J) {
  J->assign((size_t)rows * 6 * D, 0.0);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < 6; c++)
      for (int d = 0; d < D; d++)
        (*J)[((size_t)r * 6 + c) * D + d] = 0.2 * std::sin(q[(size_t)r * D + d] * (c + 1.0) + 0.31 * d) + (c == d ? 1.0 : 0.0);
}

static Table MakeTable(unsigned long long seed, int D, double frac) {
  Rng rng(seed);
  Table t;
  t.D = D;
  const int W = 3 + (int)(rng.next() * 4.0);       // 3..6
  std::vector<double> wps((size_t)W * D);
  for (auto &v : wps) v = rng.uniform(-1.0, 1.0);
  const int P = 3 * W - 2;
  std::vector<double> cps((size_t)P * D), knots(P + 3);
  const int np = tpo_joint_fit_spline(wps.data(), W, D, 0.2, cps.data(), knots.data());
  CHECK(np == P);
  t.path_end = knots[P + 2];
  t.delta = frac * t.path_end / (kN - 1);
  t.rows = (int)std::lround(t.path_end / t.delta) + kN + 1;
  t.q.resize((size_t)t.rows * D);
  std::vector<double> q1(t.q.size()), q2(t.q.size());
  CHECK(tpo_joint_sample_path(knots.data(), P + 3, cps.data(), P, D, 0.0, t.delta, t.rows, t.q.data(), q1.data(),
                              q2.data()) == 0);
  FakeJacobian(t.q.data(), t.rows, D, &t.J);
  t.vmax.resize(D); t.amax.resize(D);
  for (int d = 0; d < D; d++) t.vmax[d] = rng.uniform(0.5, 1.1);
  for (int d = 0; d < D; d++) t.amax[d] = rng.uniform(1.2, 3.0);
  t.vt = rng.uniform(0.3, 0.6);
  t.vr = rng.uniform(0.8, 1.2);
  return t;
}

static std::vector<Table> MakeFamily(int B, int D, unsigned long long seed0) {
  std::vector<Table> f(B);
  for (int b = 0; b < B; b++) f[b] = MakeTable(seed0 + b, D, (b % 2) ? 0.25 : 0.4);
  return f;
}

static tpo_planner *MakeOracle(const Table &t, int method) {
  tpo_planner *p = tpo_planner_create(t.D, kN, t.delta, kSafety, 4 * kMs, method, kMaxIter, kMaxIvError);
  tpo_planner_set_limits(p, t.vmax.data(), t.amax.data());
  tpo_planner_set_ik_table(p, t.q.data(), t.J.data(), t.rows, t.path_end, t.vt, t.vr, 1);
  return p;
}

// the first rows[k] rows (0: the whole table) of the listed planners' tables, host entry
static int Upload(tpamd_planner_set *set, const std::vector<int32_t> &ids, const std::vector<const Table *> &t,
                  const std::vector<int> &rows) {
  const int n = (int)t.size(), D = t[0]->D;
  std::vector<int32_t> off(n + 1, 0), st(n, 1);
  for (int k = 0; k < n; k++) off[k + 1] = off[k] + (rows[k] ? rows[k] : t[k]->rows);
  std::vector<double> q((size_t)off[n] * D), J((size_t)off[n] * 6 * D), pe(n), vm((size_t)n * D), am((size_t)n * D), vt(n),
      vr(n), dl(n);
  for (int k = 0; k < n; k++) {
    const size_t r = (size_t)(off[k + 1] - off[k]);
    std::memcpy(&q[(size_t)off[k] * D], t[k]->q.data(), r * D * 8);
    std::memcpy(&J[(size_t)off[k] * 6 * D], t[k]->J.data(), r * 6 * D * 8);
    std::memcpy(&vm[(size_t)k * D], t[k]->vmax.data(), D * 8);
    std::memcpy(&am[(size_t)k * D], t[k]->amax.data(), D * 8);
    pe[k] = t[k]->path_end; vt[k] = t[k]->vt; vr[k] = t[k]->vr; dl[k] = t[k]->delta;
  }
  return tpamd_planner_set_upload_ik_tables(set, n, ids.data(), off.data(), q.data(), J.data(), pe.data(), vm.data(),
                                            am.data(), vt.data(), vr.data(), dl.data(), nullptr, st.data());
}

static int UploadAll(tpamd_planner_set *set, const std::vector<Table> &fam, int rows) {
  std::vector<int32_t> ids(fam.size());
  std::vector<const Table *> ptr(fam.size());
  for (size_t b = 0; b < fam.size(); b++) { ids[b] = (int32_t)b; ptr[b] = &fam[b]; }
  return Upload(set, ids, ptr, std::vector<int>(fam.size(), rows));
}

static tpamd_planner_set *MakeSet(tpamd_engine *e, int B, int D, int method, int table_capacity) {
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 0;
  cfg.history_capacity = 0; cfg.trajectory_capacity = 8192;
  cfg.sampling_method = method; cfg.max_planning_iterations = kMaxIter;
  cfg.constraint_safety = kSafety; cfg.max_initial_velocity_error = kMaxIvError;
  cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *set = nullptr;
  CHECK(tpamd_planner_set_create_cartesian(e, &cfg, table_capacity, &set) == 0);
  return set;
}

struct Trajectories {
  std::vector<int64_t> off;
  std::vector<double> time, s, sd, sdd, q, qd, qdd;
};
static bool Download(tpamd_planner_set *set, int B, int D, Trajectories *t) {
  t->off.assign(B + 1, 0);
  int rc = tpamd_planner_set_download_trajectories(set, B, nullptr, t->off.data(), 0, nullptr, nullptr, nullptr, nullptr,
                                                   nullptr, nullptr, nullptr);
  const size_t rows = (size_t)t->off[B];
  if (rc != 0 && rows == 0) return false;
  t->time.resize(rows); t->s.resize(rows); t->sd.resize(rows); t->sdd.resize(rows);
  t->q.resize(rows * D); t->qd.resize(rows * D); t->qdd.resize(rows * D);
  if (rows == 0) return true;
  rc = tpamd_planner_set_download_trajectories(set, B, nullptr, t->off.data(), (int64_t)rows, t->time.data(), t->s.data(),
                                               t->sd.data(), t->sdd.data(), t->q.data(), t->qd.data(), t->qdd.data());
  return rc == 0;
}

// planner b of two sets: the trajectory bits
static bool SamePlanner(const Trajectories &x, const Trajectories &y, int b, int D) {
  const int64_t n = x.off[b + 1] - x.off[b];
  if (n != y.off[b + 1] - y.off[b]) return false;
  const size_t i = (size_t)x.off[b], j = (size_t)y.off[b];
  return Same(&x.time[i], &y.time[j], n) && Same(&x.s[i], &y.s[j], n) && Same(&x.sd[i], &y.sd[j], n) &&
         Same(&x.sdd[i], &y.sdd[j], n) && Same(&x.q[i * D], &y.q[j * D], n * D) && Same(&x.qd[i * D], &y.qd[j * D], n * D) &&
         Same(&x.qdd[i * D], &y.qdd[j * D], n * D);
}
static bool SameSets(const std::vector<tpamd_planner_summary> &sx, const Trajectories &x,
                     const std::vector<tpamd_planner_summary> &sy, const Trajectories &y, int B, int D) {
  if (std::memcmp(sx.data(), sy.data(), B * sizeof(tpamd_planner_summary)) != 0 || x.off != y.off) return false;
  for (int b = 0; b < B; b++)
    if (!SamePlanner(x, y, b, D)) return false;
  return true;
}

// planner b of the set against its oracle: 0 if every integer and every double agrees
static int Compare(const tpamd_planner_summary &sm, const Trajectories &t, int b, int D, const tpo_planner *o, int orc) {
  int bad = 0;
  bad |= (sm.status != orc) << 0;
  const int M = tpo_planner_num_samples(o);
  bad |= (sm.num_samples != M || t.off[b + 1] - t.off[b] != M) << 1;
  if (bad) return bad;
  bad |= (sm.end_time_ns != tpo_planner_end_time(o)) << 2;
  bad |= (sm.final_decel_start_ns != tpo_planner_final_decel_start(o)) << 3;
  bad |= (sm.target_reached != tpo_planner_target_reached(o)) << 4;
  bad |= (sm.windows != tpo_planner_windows(o)) << 5;
  bad |= (sm.path_state != tpo_planner_path_state(o)) << 6;
  const size_t r = (size_t)t.off[b];
  bad |= !Same(&t.time[r], tpo_planner_time(o), M) << 7;
  bad |= !Same(&t.s[r], tpo_planner_path_parameter(o), M) << 8;
  bad |= !Same(&t.sd[r], tpo_planner_path_velocity(o), M) << 9;
  bad |= !Same(&t.sdd[r], tpo_planner_path_acceleration(o), M) << 10;
  bad |= !Same(&t.q[r * D], tpo_planner_positions(o), (size_t)M * D) << 11;
  bad |= !Same(&t.qd[r * D], tpo_planner_velocities(o), (size_t)M * D) << 12;
  bad |= !Same(&t.qdd[r * D], tpo_planner_accelerations(o), (size_t)M * D) << 13;
  return bad;
}

static unsigned long long Hash(unsigned long long h, const void *p, size_t bytes) {
  const unsigned char *c = (const unsigned char *)p;
  for (size_t i = 0; i < bytes; i++) h = (h ^ c[i]) * 1099511628211ULL;
  return h;
}
static unsigned long long HashPlan(const std::vector<tpamd_planner_summary> &sm, const Trajectories &t) {
  unsigned long long h = 1469598103934665603ULL;
  h = Hash(h, sm.data(), sm.size() * sizeof(tpamd_planner_summary));
  h = Hash(h, t.off.data(), t.off.size() * 8);
  for (const auto *v : {&t.time, &t.s, &t.sd, &t.sdd, &t.q, &t.qd, &t.qdd}) h = Hash(h, v->data(), v->size() * 8);
  return h;
}

// rows first .. first + count[k] - 1 of the listed planners' full tables, appended through the host
// entry or, from device memory on a non-blocking stream, through the _device entry
static int Append(tpamd_planner_set *set, const std::vector<Table> &fam, const std::vector<int32_t> &ids,
                  const std::vector<int> &first, const std::vector<int> &count, bool device) {
  const int n = (int)ids.size(), D = fam[0].D;
  std::vector<int32_t> off(n + 1, 0);
  for (int k = 0; k < n; k++) off[k + 1] = off[k] + count[k];
  std::vector<double> q((size_t)off[n] * D + 1), J((size_t)off[n] * 6 * D + 1);
  for (int k = 0; k < n; k++) {
    const Table &t = fam[ids[k]];
    CHECK(first[k] + count[k] <= t.rows);
    std::memcpy(&q[(size_t)off[k] * D], &t.q[(size_t)first[k] * D], (size_t)count[k] * D * 8);
    std::memcpy(&J[(size_t)off[k] * 6 * D], &t.J[(size_t)first[k] * 6 * D], (size_t)count[k] * 6 * D * 8);
  }
  if (!device) return tpamd_planner_set_append_ik_rows(set, n, ids.data(), off.data(), q.data(), J.data());
  hipStream_t stream = nullptr;
  double *dq = nullptr, *dJ = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  HIP_OK(hipMalloc((void **)&dq, q.size() * 8));
  HIP_OK(hipMalloc((void **)&dJ, J.size() * 8));
  HIP_OK(hipMemcpyAsync(dq, q.data(), q.size() * 8, hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemcpyAsync(dJ, J.data(), J.size() * 8, hipMemcpyHostToDevice, stream));
  const int rc = tpamd_planner_set_append_ik_rows_device(set, n, ids.data(), off.data(), dq, dJ, stream);
  HIP_OK(hipStreamSynchronize(stream));
  HIP_OK(hipFree(dq)); HIP_OK(hipFree(dJ));
  HIP_OK(hipStreamDestroy(stream));
  return rc;
}

struct WalkOptions {
  int D = 7, method = 0;
  unsigned long long seed0 = 1;
  int extra = 0;                   // rows per append beyond need_count (test 2)
  bool short_append = false;       // test 3
  bool device_append = false;      // the _device entry on a non-blocking stream
  const char *name = "";
};
struct WalkResult {
  std::vector<unsigned long long> hashes;      // one per completed Plan
  int suspensions = 0, mixed_calls = 0, mixed_resumes = 0, plans = 0, short_cases = 0;
};

// One receding-horizon walk: streaming set against its oracles and a whole-table set.
static WalkResult Walk(tpamd_engine *e, const WalkOptions &o) {
  const int B = kB, D = o.D;
  WalkResult res;
  std::vector<Table> fam = MakeFamily(B, D, o.seed0);
  std::vector<tpo_planner *> orc(B);
  for (int b = 0; b < B; b++) orc[b] = MakeOracle(fam[b], o.method);
  int longest = 0;
  for (const Table &t : fam) longest = std::max(longest, t.rows);
  tpamd_planner_set *whole = MakeSet(e, B, D, o.method, longest), *stream = MakeSet(e, B, D, o.method, kN);
  if (!whole || !stream) return res;
  CHECK(UploadAll(whole, fam, 0) == 0);
  CHECK(UploadAll(stream, fam, kN) == 0);                 // rows 0 .. N-1 only
  const size_t bytes0 = tpamd_planner_set_device_bytes(stream);
  std::vector<int> rows(B, kN);                           // what the streaming set holds
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<int> rc(B, 0), reached(B, 0);
  std::vector<tpamd_planner_summary> sw(B), ss(B);
  std::vector<int32_t> nf(B), nc(B);
  Trajectories tw, ts, before, after;
  int reported = 0;
  for (int step = 0; step < 300; step++) {
    for (int b = 0; b < B; b++) rc[b] = tpo_planner_plan(orc[b], start[b], horizon[b]);
    for (int b = 0; b < B; b++) CHECK(rc[b] == TPO_PLAN_OK);
    CHECK(tpamd_planner_set_plan(whole, start.data(), horizon.data(), sw.data()) == 0);
    size_t up0 = 0, down0 = 0;
    tpamd_planner_set_last_plan_bytes(whole, &up0, &down0);
    int32_t waiting = -1;
    CHECK(tpamd_planner_set_plan_streaming(stream, start.data(), horizon.data(), ss.data(), nf.data(), nc.data(),
                                           &waiting) == 0);
    {
      // the streaming call moves what Plan moves for the windows it ran, plus 8 bytes per planner down
      size_t up = 0, down = 0;
      int max_windows = 0;
      for (int b = 0; b < B; b++) max_windows = std::max(max_windows, ss[b].windows);
      tpamd_planner_set_last_plan_bytes(stream, &up, &down);
      CHECK(up == (size_t)24 * B && up == up0);
      CHECK(down <= (size_t)56 * B + 8 * ((size_t)max_windows + 2) + 8 + (size_t)8 * B);
      if (waiting == 0) CHECK(down == down0 + (size_t)8 * B);
    }
    bool shorted = false;
    for (int round = 0; waiting > 0; round++) {
      CHECK(round < 64);
      if (round >= 64) break;
      int counted = 0, finished_here = 0;
      for (int b = 0; b < B; b++) {
        if (nc[b] > 0) {
          counted++;
          CHECK(ss[b].status == TPAMD_PLAN_NEEDS_ROWS && nf[b] == rows[b] && nc[b] >= 1);
        } else {
          CHECK(nf[b] == 0 && ss[b].status == TPAMD_PLAN_OK);
          finished_here++;
        }
      }
      CHECK(counted == waiting);
      res.suspensions += waiting;
      if (round == 0 && finished_here > 0) res.mixed_calls++;
      std::vector<int32_t> ids;
      std::vector<int> first, count;
      int victim = -1;
      for (int b = 0; b < B; b++) {
        if (nc[b] == 0) continue;
        int c = std::min(nc[b] + o.extra, fam[b].rows - nf[b]);
        if (o.short_append && !shorted && victim < 0 && nc[b] >= 2 && waiting >= 2) { victim = b; c = nc[b] - 1; }
        ids.push_back(b); first.push_back(nf[b]); count.push_back(c);
      }
      CHECK(Append(stream, fam, ids, first, count, o.device_append) == 0);
      for (size_t k = 0; k < ids.size(); k++) rows[ids[k]] += count[k];
      const int victim_need = victim >= 0 ? nf[victim] + nc[victim] - 1 : 0;
      CHECK(tpamd_planner_set_plan_resume(stream, ss.data(), nf.data(), nc.data(), &waiting) == 0);
      if (waiting > 0)         // a resume after which some planners wait again while others of it finished
        for (int32_t b : ids)
          if (nc[b] == 0 && ss[b].status == TPAMD_PLAN_OK && ss[b].windows > 0) { res.mixed_resumes++; break; }
      {
        size_t up = 0, down = 0;
        tpamd_planner_set_last_plan_bytes(stream, &up, &down);
        CHECK(up == 0);                                     // a resume moves nothing upwards
      }
      if (victim >= 0) {
        // test 3: one row short. The planner waits for that row; the second resume finishes it and
        // leaves every planner that was not waiting exactly as it was
        shorted = true;
        CHECK(nc[victim] == 1 && nf[victim] == victim_need && ss[victim].status == TPAMD_PLAN_NEEDS_ROWS);
        std::vector<char> was_waiting(B);
        for (int b = 0; b < B; b++) was_waiting[b] = nc[b] > 0;
        CHECK(Download(stream, B, D, &before));
        std::vector<tpamd_planner_summary> sb = ss;
        std::vector<int32_t> ids2;
        std::vector<int> first2, count2;
        for (int b = 0; b < B; b++)
          if (nc[b] > 0) { ids2.push_back(b); first2.push_back(nf[b]); count2.push_back(b == victim ? 1 : nc[b]); }
        CHECK(Append(stream, fam, ids2, first2, count2, false) == 0);
        for (size_t k = 0; k < ids2.size(); k++) rows[ids2[k]] += count2[k];
        res.suspensions += waiting;
        CHECK(tpamd_planner_set_plan_resume(stream, ss.data(), nf.data(), nc.data(), &waiting) == 0);
        CHECK(Download(stream, B, D, &after));
        CHECK(ss[victim].status == TPAMD_PLAN_OK || nc[victim] > 0);      // it went on (it may wait at a later window)
        int untouched = 0, others = 0;
        for (int b = 0; b < B; b++) {
          if (was_waiting[b]) continue;
          others++;
          untouched += SamePlanner(before, after, b, D) &&
                       std::memcmp(&sb[b], &ss[b], sizeof(tpamd_planner_summary)) == 0;
        }
        CHECK(others > 0 && untouched == others);
        res.short_cases++;
      }
    }
    // the completed Plan
    CHECK(Download(whole, B, D, &tw) && Download(stream, B, D, &ts));
    CHECK(SameSets(sw, tw, ss, ts, B, D));
    for (int b = 0; b < B; b++) {
      const int bad = Compare(ss[b], ts, b, D, orc[b], rc[b]);
      CHECK(bad == 0);
      if (bad && ++reported <= 10)
        std::printf("  %s step %d planner %d: differences 0x%x (status %d / oracle %d, samples %d / %d, windows %d / %d)\n",
                    o.name, step, b, bad, ss[b].status, rc[b], ss[b].num_samples, tpo_planner_num_samples(orc[b]),
                    ss[b].windows, tpo_planner_windows(orc[b]));
    }
    res.hashes.push_back(HashPlan(ss, ts));
    res.plans++;
    int all_done = 1;
    for (int b = 0; b < B; b++) {
      reached[b] = tpo_planner_target_reached(orc[b]);
      if (!reached[b]) {
        start[b] = std::min<int64_t>(tpo_planner_end_time(orc[b]), start[b] + 200 * kMs);
        all_done = 0;
      }
    }
    if (all_done) break;
  }
  int at_end = 0;
  for (int b = 0; b < B; b++) at_end += reached[b];
  CHECK(at_end == B);
  CHECK(res.suspensions > 0);
  // 4 / 7: the final tables are the rows appended; the capacity grew from N and the first rows survived
  int same = 0, fewer = 0;
  for (int b = 0; b < B; b++) {
    int32_t r = -1;
    CHECK(tpamd_planner_set_download_ik_table(stream, b, &r, nullptr, nullptr, 0) == 0 && r == rows[b]);
    const int full = tpamd_ik_table_rows(fam[b].path_end, fam[b].delta, kN);
    CHECK(full == fam[b].rows && r <= full);
    fewer += r < full;
    std::vector<double> q((size_t)r * D), J((size_t)r * 6 * D);
    CHECK(tpamd_planner_set_download_ik_table(stream, b, &r, q.data(), J.data(), r) == 0);
    same += Same(q.data(), fam[b].q.data(), q.size()) && Same(J.data(), fam[b].J.data(), J.size());
  }
  CHECK(same == B);
  if (fewer == 0) std::printf("  %s: NO planner ends with fewer rows than the whole table\n", o.name);
  CHECK(fewer > 0);
  CHECK(tpamd_planner_set_device_bytes(stream) > bytes0);
  std::printf("%s: D %d %s: %d Plan calls, %d suspensions, %d streaming calls and %d resumes with waiting and finishing "
              "planners, %d of %d final tables shorter than the whole table, %d at the end%s\n",
              o.name, D, o.method ? "skip" : "uniform", res.plans, res.suspensions, res.mixed_calls, res.mixed_resumes,
              fewer, B, at_end, g_fail ? " (FAILURES)" : "");
  for (auto *p : orc) tpo_planner_destroy(p);
  tpamd_planner_set_destroy(whole);
  tpamd_planner_set_destroy(stream);
  return res;
}

// test 5: tpamd_planner_set_plan on a table that ends inside the path
static void TestPlanStillFails(tpamd_engine *e) {
  const int B = 8, D = 6, p = 3;
  std::vector<Table> fam = MakeFamily(B, D, 61000);
  int longest = 0;
  for (const Table &t : fam) longest = std::max(longest, t.rows);
  tpamd_planner_set *whole = MakeSet(e, B, D, 0, longest), *cut = MakeSet(e, B, D, 0, longest);
  if (!whole || !cut) return;
  CHECK(UploadAll(whole, fam, 0) == 0);
  std::vector<int32_t> ids(B);
  std::vector<const Table *> ptr(B);
  std::vector<int> rows(B, 0);
  for (int b = 0; b < B; b++) { ids[b] = b; ptr[b] = &fam[b]; }
  rows[p] = (kN + fam[p].rows) / 2;
  CHECK(Upload(cut, ids, ptr, rows) == 0);
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<tpamd_planner_summary> s1(B), s2(B);
  Trajectories t1, t2;
  int failed_at = -1, equal_before = 0;
  for (int step = 0; step < 300 && failed_at < 0; step++) {
    CHECK(tpamd_planner_set_plan(whole, start.data(), horizon.data(), s1.data()) == 0);
    CHECK(tpamd_planner_set_plan(cut, start.data(), horizon.data(), s2.data()) == 0);
    CHECK(Download(whole, B, D, &t1) && Download(cut, B, D, &t2));
    for (int b = 0; b < B; b++) {
      if (b == p && s2[b].status != TPAMD_PLAN_OK) { failed_at = step; continue; }
      CHECK(std::memcmp(&s1[b], &s2[b], sizeof(tpamd_planner_summary)) == 0 && SamePlanner(t1, t2, b, D));
      equal_before += b == p;
    }
    bool done = true;
    for (int b = 0; b < B; b++)
      if (!s1[b].target_reached) { start[b] = std::min<int64_t>(s1[b].end_time_ns, start[b] + 200 * kMs); done = false; }
    if (done) break;
  }
  CHECK(failed_at >= 0 && s2[p].status == TPAMD_PLAN_INTERNAL && equal_before == failed_at);
  // the streaming entries were never used: nobody waits
  CHECK(tpamd_planner_set_plan_resume(cut, s2.data(), nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  std::printf("plan on a short table: TPAMD_PLAN_INTERNAL at Plan %d, %d Plans equal before it, neighbours equal\n",
              failed_at, equal_before);
  tpamd_planner_set_destroy(whole);
  tpamd_planner_set_destroy(cut);
}

// test 6: refused calls change nothing; a suspension is dropped by reset and by a fresh upload
static void TestRefusals(tpamd_engine *e) {
  const int D = 7;
  {
    // a joint set
    const int B = 4;
    tpamd_planner_set_config cfg{};
    cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 16;
    cfg.sampling_method = 0; cfg.max_planning_iterations = 200; cfg.constraint_safety = kSafety;
    cfg.max_initial_velocity_error = kMaxIvError; cfg.time_step_ns = 4 * kMs;
    tpamd_planner_set *a = nullptr, *b = nullptr;
    CHECK(tpamd_planner_set_create(e, &cfg, &a) == 0 && tpamd_planner_set_create(e, &cfg, &b) == 0);
    if (!a || !b) return;
    Rng rng(98);
    std::vector<int32_t> off(B + 1), np(B), st(B);
    std::vector<double> wps, vm((size_t)B * D), am((size_t)B * D), dl(B, 0.02);
    for (int k = 0; k <= B; k++) {
      off[k] = (int32_t)(wps.size() / D);
      if (k < B) for (int i = 0; i < 4 * D; i++) wps.push_back(rng.uniform(-1.0, 1.0));
    }
    for (auto &v : vm) v = rng.uniform(0.5, 1.1);
    for (auto &v : am) v = rng.uniform(1.2, 3.0);
    for (tpamd_planner_set *s : {a, b})
      CHECK(tpamd_planner_set_set_waypoints(s, B, nullptr, off.data(), wps.data(), 0.2, vm.data(), am.data(), dl.data(),
                                            nullptr, np.data(), st.data()) == 0);
    std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
    std::vector<tpamd_planner_summary> s1(B), s2(B);
    std::vector<int32_t> nf(B, 5), nc(B, 5);
    int32_t waiting = 5;
    CHECK(tpamd_planner_set_plan(a, start.data(), horizon.data(), s1.data()) == 0);
    CHECK(tpamd_planner_set_plan(b, start.data(), horizon.data(), s2.data()) == 0);
    Table t = MakeTable(7, D, 0.4);
    std::vector<int32_t> o2{0, 3};
    CHECK(tpamd_planner_set_append_ik_rows(a, 1, nullptr, o2.data(), t.q.data(), t.J.data()) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows_device(a, 1, nullptr, o2.data(), t.q.data(), t.J.data(), nullptr) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_plan_streaming(a, start.data(), horizon.data(), s1.data(), nf.data(), nc.data(), &waiting) ==
          TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_plan_resume(a, s1.data(), nf.data(), nc.data(), &waiting) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(waiting == 5 && nf[0] == 5 && nc[0] == 5);
    for (int k = 0; k < B; k++) start[k] = 200 * kMs;
    CHECK(tpamd_planner_set_plan(a, start.data(), horizon.data(), s1.data()) == 0);
    CHECK(tpamd_planner_set_plan(b, start.data(), horizon.data(), s2.data()) == 0);
    Trajectories t1, t2;
    CHECK(Download(a, B, D, &t1) && Download(b, B, D, &t2));
    const bool eq = SameSets(s1, t1, s2, t2, B, D) && t1.time.size() > 0;
    CHECK(eq);
    std::printf("streaming entries on a joint set: refused, plans %s\n", eq ? "unchanged" : "CHANGED");
    tpamd_planner_set_destroy(a);
    tpamd_planner_set_destroy(b);
  }
  // Cartesian sets: x takes the refused calls and the drops, y is its twin / the fresh set
  const int B = 6;
  std::vector<Table> fam = MakeFamily(B, D, 62000), other = MakeFamily(2, D, 63000);
  int longest = 0;
  for (const Table &t : fam) longest = std::max(longest, t.rows);
  for (const Table &t : other) longest = std::max(longest, t.rows);
  tpamd_planner_set *x = MakeSet(e, B, D, 0, longest), *y = MakeSet(e, B, D, 0, longest);
  if (!x || !y) return;
  std::vector<int32_t> five{0, 1, 2, 3, 4};
  std::vector<const Table *> ptr5{&fam[0], &fam[1], &fam[2], &fam[3], &fam[4]};
  CHECK(Upload(x, five, ptr5, std::vector<int>(5, kN)) == 0);          // planner 5 has no table
  // a horizon no first window reaches: the first Plan chains windows to the end of the path, past row N - 1
  std::vector<int64_t> start(B, 0), horizon(B, 60000 * kMs);
  std::vector<tpamd_planner_summary> sx(B), sy(B);
  std::vector<int32_t> nf(B), nc(B);
  int32_t waiting = -1;
  CHECK(tpamd_planner_set_plan_resume(x, sx.data(), nf.data(), nc.data(), &waiting) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_plan_streaming(x, start.data(), horizon.data(), sx.data(), nf.data(), nc.data(), &waiting) == 0);
  CHECK(waiting == 5 && sx[5].status == TPAMD_PLAN_FAILED_PRECONDITION && nc[5] == 0);
  for (int b = 0; b < 5; b++) CHECK(sx[b].status == TPAMD_PLAN_NEEDS_ROWS && nf[b] == kN && nc[b] >= 1);
  {
    // refused appends: a repeated id, an id out of range, a planner without a table, bad offsets
    const Table &t = fam[0];
    const double *q = &t.q[(size_t)kN * D], *J = &t.J[(size_t)kN * 6 * D];
    const int32_t rep[2] = {0, 0}, bad[2] = {0, B}, none[2] = {0, 5}, ok[2] = {0, 1};
    const int32_t o3[3] = {0, 1, 2}, o_bad[3] = {1, 2, 3}, o_dec[3] = {0, 2, 1};
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, rep, o3, q, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, bad, o3, q, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, none, o3, q, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows_device(x, 2, none, o3, q, J, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, ok, o_bad, q, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, ok, o_dec, q, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, 2, ok, o3, nullptr, J) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_append_ik_rows(x, -1, ok, o3, q, J) == TPAMD_E_INVALID_ARGUMENT);
    const int32_t o0[1] = {0};
    CHECK(tpamd_planner_set_append_ik_rows(x, 0, nullptr, o0, q, J) == 0);                 // nothing listed
    for (int b = 0; b < 5; b++) {
      int32_t r = -1;
      CHECK(tpamd_planner_set_download_ik_table(x, b, &r, nullptr, nullptr, 0) == 0 && r == kN);
    }
  }
  // planner 0 is reset and gets another path; planner 1 gets another path by a fresh upload; both
  // stop waiting. Planners 2..4 get their rows and resume.
  const int32_t id0 = 0;
  CHECK(tpamd_planner_set_reset(x, 1, &id0) == 0);
  CHECK(Upload(x, {0, 1}, {&other[0], &other[1]}, {0, 0}) == 0);
  {
    std::vector<int32_t> ids{2, 3, 4};
    std::vector<int> first{nf[2], nf[3], nf[4]}, count{nc[2], nc[3], nc[4]};
    CHECK(Append(x, fam, ids, first, count, false) == 0);
    int guard = 0;
    CHECK(tpamd_planner_set_plan_resume(x, sx.data(), nf.data(), nc.data(), &waiting) == 0);
    CHECK(nc[0] == 0 && nc[1] == 0 && waiting <= 3);
    while (waiting > 0 && guard++ < 64) {
      ids.clear(); first.clear(); count.clear();
      for (int b = 2; b < 5; b++)
        if (nc[b] > 0) { ids.push_back(b); first.push_back(nf[b]); count.push_back(nc[b]); }
      CHECK(Append(x, fam, ids, first, count, false) == 0);
      CHECK(tpamd_planner_set_plan_resume(x, sx.data(), nf.data(), nc.data(), &waiting) == 0);
      CHECK(nc[0] == 0 && nc[1] == 0);
    }
    CHECK(waiting == 0);
    for (int b = 2; b < 5; b++) CHECK(sx[b].status == TPAMD_PLAN_OK && sx[b].num_samples > 0);
    CHECK(tpamd_planner_set_plan_resume(x, sx.data(), nf.data(), nc.data(), &waiting) == TPAMD_E_INVALID_ARGUMENT);
  }
  // the fresh set: the new paths of planners 0 and 1, nothing before
  CHECK(Upload(y, {0, 1}, {&other[0], &other[1]}, {0, 0}) == 0);
  Trajectories tx, ty;
  int equal = 0, plans = 0;
  for (int step = 0; step < 3; step++) {
    CHECK(tpamd_planner_set_plan(x, start.data(), horizon.data(), sx.data()) == 0);
    CHECK(tpamd_planner_set_plan(y, start.data(), horizon.data(), sy.data()) == 0);
    CHECK(Download(x, B, D, &tx) && Download(y, B, D, &ty));
    bool eq = true;
    for (int b = 0; b < 2; b++) {
      CHECK(sx[b].status == TPAMD_PLAN_OK && sx[b].num_samples > 0);
      eq = eq && std::memcmp(&sx[b], &sy[b], sizeof(tpamd_planner_summary)) == 0 && SamePlanner(tx, ty, b, D);
    }
    CHECK(eq);
    equal += eq;
    plans++;
    for (int b = 0; b < B; b++)
      if (sx[b].status == TPAMD_PLAN_OK && !sx[b].target_reached)
        start[b] = std::min<int64_t>(sx[b].end_time_ns, start[b] + 200 * kMs);
  }
  std::printf("suspension dropped by reset and by upload: %d of %d Plans equal to a fresh set\n", equal, plans);
  tpamd_planner_set_destroy(x);
  tpamd_planner_set_destroy(y);
}

// No argument: everything. "walk D method": the three walks of one family. "plan", "refusals".
int main(int argc, char **argv) {
  const bool all = argc < 2;
  const bool walks = all || std::strcmp(argv[1], "walk") == 0;
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) { std::printf("no engine\n"); return 1; }
  for (int D : {5, 6, 7})
    for (int method : {0, 1}) {
      if (!walks || (argc >= 4 && (std::atoi(argv[2]) != D || std::atoi(argv[3]) != method))) continue;
      WalkOptions o;
      o.D = D; o.method = method; o.seed0 = 70000 + 1000 * D + 100000 * method;
      o.name = "exact";
      const WalkResult exact = Walk(e, o);
      o.extra = 7; o.name = "ahead"; o.device_append = true;
      const WalkResult ahead = Walk(e, o);
      CHECK(exact.plans > 0 && exact.hashes == ahead.hashes);            // 2: independent of the chunking
      CHECK(ahead.suspensions < exact.suspensions);
      // some call suspended planners while others finished in that same call
      CHECK(exact.mixed_calls > 0 && exact.mixed_calls + exact.mixed_resumes + ahead.mixed_resumes > 0);
      o.extra = 0; o.name = "short"; o.short_append = true; o.device_append = false;
      const WalkResult sh = Walk(e, o);
      CHECK(sh.short_cases > 0 && sh.hashes == exact.hashes);
    }
  if (all || std::strcmp(argv[1], "plan") == 0) TestPlanStillFails(e);
  if (all || std::strcmp(argv[1], "refusals") == 0) TestRefusals(e);
  tpamd_engine_destroy(e);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

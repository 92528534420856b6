// GPU test of Cartesian planner sets through the C-ABI (run by tests/test_gpu_cartesian_set.py):
// tpamd_planner_set_create_cartesian / _upload_ik_tables[_device] / _download_ik_table and
// tpamd_planner_set_plan on resident IK tables, against one oracle IK-table planner per planner
// (oracle/tp_oracle_plan.c: tpo_planner_set_ik_table + tpo_planner_plan), bit for bit.
//
// The synthetic family (planner seed s): W in 3..6 waypoints uniform in [-1, 1]^D -> the joint fit
// (rounding 0.2) -> kend; delta = f kend / (N - 1) with f in {0.4, 0.25} mixed inside a set; rows =
// round(kend / delta) + N + 1; the q table is the spline sampled at r delta (end-padded);
// J[r][c][d] = 0.2 sin(q_d (c + 1) + 0.31 d) + (c == d); v_max in [0.5, 1.1], a_max in [1.2, 3.0],
// v_trans in [0.3, 0.6], v_rot in [0.8, 1.2]. N = 300, 4 ms step, 750 ms horizon, a replan every
// 200 ms until every planner is at its end.
//   family    1. after every Plan, every planner's summary and full trajectory equal its oracle's;
//             every oracle planner returns TPO_PLAN_OK at every step and ends with target_reached
//             (asserted, nothing is left out); 9. the PCIe bytes of every Plan
//   modified  2. at the 4th Plan a third of the planners get their table again with path_state 2
//             and the trajectory's velocity at the start time; 5. one of the runs starts with
//             table_capacity = N and re-uploads longer (end-padded) tables, so the capacity grows
//             twice: the untouched planners' tables and plans stay as they were
//   failures  4. a table one row too short for the last window (TPAMD_PLAN_INTERNAL at the Plan where
//             the oracle returns TPO_PLAN_INTERNAL), an initial velocity off the start tangent
//             (TPAMD_PLAN_INVALID_ARGUMENT); 8. the joint-only entries and the call-level errors on
//             this set return TPAMD_E_INVALID_ARGUMENT; the neighbours stay bit-equal to their oracles
//   device    6. tables in device memory, uploaded on a non-blocking stream, against a twin set
//             loaded through the host entry
//   kinds     8. the IK-table entries on a joint set
// `--cpu-check` runs the oracle alone over the same families and asserts the conditions of 1 and 2
// (every planner OK at every step, target reached); it makes no GPU call, and
// tests/test_cartesian_set_cpu.py runs it.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "../../include/tpamd.h"
#include "../../oracle/tp_oracle.h"
#include "test_support.h"

static const int kN = 300;
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

// One planner of the family.
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

// `pad` more rows that repeat the last one (the spline is end-padded there already)
static Table Padded(const Table &t, int pad) {
  Table r = t;
  r.rows = t.rows + pad;
  r.q.resize((size_t)r.rows * t.D);
  for (int i = t.rows; i < r.rows; i++) std::memcpy(&r.q[(size_t)i * t.D], &t.q[(size_t)(t.rows - 1) * t.D], t.D * 8);
  FakeJacobian(r.q.data(), r.rows, t.D, &r.J);
  CHECK(Same(r.J.data(), t.J.data(), t.J.size()));
  return r;
}

static tpo_planner *MakeOracle(const Table &t, int method, const double *iv, int state) {
  tpo_planner *p = tpo_planner_create(t.D, kN, t.delta, kSafety, 4 * kMs, method, kMaxIter, kMaxIvError);
  tpo_planner_set_limits(p, t.vmax.data(), t.amax.data());
  if (iv) tpo_planner_set_initial_velocity(p, iv);
  tpo_planner_set_ik_table(p, t.q.data(), t.J.data(), t.rows, t.path_end, t.vt, t.vr, state);
  return p;
}

// upload the tables of the listed planners (host entry)
static int Upload(tpamd_planner_set *set, const std::vector<int32_t> &ids, const std::vector<const Table *> &t,
                  const std::vector<double> *iv, int state, bool null_ids = false) {
  const int n = (int)t.size(), D = t[0]->D;
  std::vector<int32_t> off(n + 1, 0), st(n, state);
  for (int k = 0; k < n; k++) off[k + 1] = off[k] + t[k]->rows;
  std::vector<double> q((size_t)off[n] * D), J((size_t)off[n] * 6 * D), pe(n), vm((size_t)n * D), am((size_t)n * D), vt(n),
      vr(n), dl(n);
  for (int k = 0; k < n; k++) {
    std::memcpy(&q[(size_t)off[k] * D], t[k]->q.data(), t[k]->q.size() * 8);
    std::memcpy(&J[(size_t)off[k] * 6 * D], t[k]->J.data(), t[k]->J.size() * 8);
    std::memcpy(&vm[(size_t)k * D], t[k]->vmax.data(), D * 8);
    std::memcpy(&am[(size_t)k * D], t[k]->amax.data(), D * 8);
    pe[k] = t[k]->path_end; vt[k] = t[k]->vt; vr[k] = t[k]->vr; dl[k] = t[k]->delta;
  }
  return tpamd_planner_set_upload_ik_tables(set, n, null_ids ? nullptr : ids.data(), off.data(), q.data(), J.data(),
                                            pe.data(), vm.data(), am.data(), vt.data(), vr.data(), dl.data(),
                                            iv ? iv->data() : nullptr, st.data());
}

static tpamd_planner_set *MakeSet(tpamd_engine *e, int B, int D, int method, int table_capacity) {
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 0;
  cfg.history_capacity = 0; cfg.trajectory_capacity = 32768;
  cfg.sampling_method = method; cfg.max_planning_iterations = kMaxIter;
  cfg.constraint_safety = kSafety; cfg.max_initial_velocity_error = kMaxIvError;
  cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *set = nullptr;
  CHECK(tpamd_planner_set_create_cartesian(e, &cfg, table_capacity, &set) == 0);
  return set;
}

// all trajectories of a set, packed
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

static void ParallelFor(int n, const std::function<void(int)> &fn) {
  const int T = 16;
  std::vector<std::thread> th;
  for (int k = 0; k < T; k++)
    th.emplace_back([&, k] { for (int i = k; i < n; i += T) fn(i); });
  for (auto &x : th) x.join();
}

// the velocity of the oracle's trajectory at the sample closest to start
static std::vector<double> VelocityAt(const tpo_planner *o, int D, int64_t start) {
  const int M = tpo_planner_num_samples(o);
  const double *tm = tpo_planner_time(o);
  int best = 0;
  for (int i = 1; i < M; i++)
    if (std::fabs(tm[i] - start / 1e9) < std::fabs(tm[best] - start / 1e9)) best = i;
  const double *v = tpo_planner_velocities(o) + (size_t)best * D;
  return std::vector<double>(v, v + D);
}

struct RunOptions {
  int B = 256, D = 7, method = 0;
  unsigned long long seed0 = 1;
  int table_capacity = 0;          // 0: enough for every table
  bool modify = false;             // test 2: re-upload a third with path_state 2 at the 4th Plan
  int pad = 0;                     // ... with this many rows more
  bool failures = false;           // test 4 / 8: planner 5 one row short, planner 9 off-tangent velocity
  bool cpu_only = false;
  const char *name = "";
};

// One receding-horizon run of a set against its oracles. Returns the number of Plan calls.
static int Run(tpamd_engine *e, const RunOptions &o) {
  const int B = o.B, D = o.D;
  std::vector<Table> fam = MakeFamily(B, D, o.seed0);
  std::vector<tpo_planner *> orc(B, nullptr);
  std::vector<double> bad_iv;
  int short_planner = -1, iv_planner = -1;
  if (o.failures) {
    // the last window of planner 5: its oracle run on the whole table ends at s = path_horizon of
    // that window; a table that ends one row before that window's last row is one row too short
    short_planner = 5; iv_planner = 9;
    tpo_planner *p = MakeOracle(fam[short_planner], o.method, nullptr, 1);
    int64_t start = 0;
    for (int step = 0; step < 300 && !tpo_planner_target_reached(p); step++) {
      CHECK(tpo_planner_plan(p, start, 750 * kMs) == TPO_PLAN_OK);
      start = std::min<int64_t>(tpo_planner_end_time(p), start + 200 * kMs);
    }
    CHECK(tpo_planner_target_reached(p));
    const int M = tpo_planner_num_samples(p);
    const int last = (int)std::lround(tpo_planner_path_parameter(p)[M - 1] / fam[short_planner].delta);
    tpo_planner_destroy(p);
    CHECK(last >= kN && last < fam[short_planner].rows);
    Table &t = fam[short_planner];
    t.rows = last;                       // rows 0 .. last - 1
    t.q.resize((size_t)t.rows * D);
    t.J.resize((size_t)t.rows * 6 * D);
    bad_iv.assign(D, 0.0);
    bad_iv[0] = 0.3; bad_iv[1] = -0.2;
  }
  for (int b = 0; b < B; b++) orc[b] = MakeOracle(fam[b], o.method, b == iv_planner ? bad_iv.data() : nullptr, 1);
  tpamd_planner_set *set = nullptr;
  std::vector<int32_t> all(B);
  for (int b = 0; b < B; b++) all[b] = b;
  int longest = 0;
  for (const Table &t : fam) longest = std::max(longest, t.rows);
  if (!o.cpu_only) {
    set = MakeSet(e, B, D, o.method, o.table_capacity ? o.table_capacity : longest);
    if (!set) return 0;
    std::vector<const Table *> ptr(B);
    for (int b = 0; b < B; b++) ptr[b] = &fam[b];
    std::vector<double> iv;
    if (o.failures) {
      iv.assign((size_t)B * D, 0.0);
      std::memcpy(&iv[(size_t)iv_planner * D], bad_iv.data(), D * 8);
    }
    CHECK(Upload(set, all, ptr, o.failures ? &iv : nullptr, 1, /*null_ids=*/true) == 0);
    // the resident tables are the uploaded ones
    int same = 0;
    for (int b = 0; b < B; b++) {
      int32_t rows = -1;
      std::vector<double> q(fam[b].q.size()), J(fam[b].J.size());
      CHECK(tpamd_planner_set_download_ik_table(set, b, &rows, nullptr, nullptr, 0) == 0 && rows == fam[b].rows);
      CHECK(tpamd_planner_set_download_ik_table(set, b, &rows, q.data(), J.data(), rows - 1) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(tpamd_planner_set_download_ik_table(set, b, &rows, q.data(), J.data(), rows) == 0);
      same += Same(q.data(), fam[b].q.data(), q.size()) && Same(J.data(), fam[b].J.data(), J.size());
    }
    CHECK(same == B);
  }
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<int> rc(B, 0), reached(B, 0);
  std::vector<char> diverged(B, 0);
  std::vector<tpamd_planner_summary> sm(B);
  Trajectories tr;
  int plans = 0, compared = 0, reported = 0, modified = 0, internal_at = -1, invalid_at = -1;
  long windows = 0;
  const size_t bytes0 = set ? tpamd_planner_set_device_bytes(set) : 0;
  for (int step = 0; step < 300; step++) {
    if (o.modify && step == 3) {
      // test 2 (and 5): every third planner gets its table again, as a modified path that starts
      // with the velocity its trajectory has at the next start
      std::vector<int32_t> ids;
      std::vector<Table> fresh;
      std::vector<double> iv;
      for (int b = 1; b < B; b += 3) {
        ids.push_back(b);
        fresh.push_back(o.pad ? Padded(fam[b], o.pad + 7 * (b % 5)) : fam[b]);
        const std::vector<double> v = VelocityAt(orc[b], D, start[b]);
        iv.insert(iv.end(), v.begin(), v.end());
        tpo_planner_set_initial_velocity(orc[b], v.data());
        const Table &t = fresh.back();
        tpo_planner_set_ik_table(orc[b], t.q.data(), t.J.data(), t.rows, t.path_end, t.vt, t.vr, 2);
      }
      modified = (int)ids.size();
      if (set) {
        // the untouched planners' tables before and after (the capacity grows when pad > 0)
        std::vector<const Table *> ptr;
        for (const Table &t : fresh) ptr.push_back(&t);
        CHECK(Upload(set, ids, ptr, &iv, 2) == 0);
        if (o.pad) CHECK(tpamd_planner_set_device_bytes(set) > bytes0);
        int same = 0, expect = 0;
        for (int b = 0; b < B; b++) {
          const bool touched = b % 3 == 1;
          const Table &t = touched ? fresh[(b - 1) / 3] : fam[b];
          int32_t rows = -1;
          std::vector<double> q(t.q.size()), J(t.J.size());
          CHECK(tpamd_planner_set_download_ik_table(set, b, &rows, q.data(), J.data(), t.rows) == 0 && rows == t.rows);
          same += Same(q.data(), t.q.data(), q.size()) && Same(J.data(), t.J.data(), J.size());
          expect++;
        }
        CHECK(same == expect);
      }
      for (size_t k = 0; k < ids.size(); k++) fam[ids[k]] = fresh[k];
    }
    if (o.failures && set && step == 2) {
      // test 8: none of these changes anything (the Plans below stay bit-equal to the oracles)
      const Table &t = fam[0];
      std::vector<int32_t> np1{4}, st1{1}, off2{0, 0, 0};
      std::vector<double> knots(7, 0.0), cps(4 * D, 0.0), vm(D, 1.0), am(D, 1.0), dl{0.01}, stop(1);
      std::vector<int64_t> tns{0};
      int32_t np = 0, status = 0;
      CHECK(tpamd_planner_set_upload_paths(set, 1, nullptr, knots.data(), cps.data(), vm.data(), am.data(), dl.data(),
                                           nullptr, st1.data()) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(tpamd_planner_set_upload_paths_ragged(set, 1, nullptr, np1.data(), knots.data(), cps.data(), vm.data(),
                                                  am.data(), dl.data(), nullptr, st1.data()) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(tpamd_planner_set_download_path(set, 0, &np, nullptr, nullptr, 0) == TPAMD_E_INVALID_ARGUMENT);
      std::vector<int32_t> woff{0, 2};
      std::vector<double> wps(2 * D, 0.1);
      CHECK(tpamd_planner_set_switch_paths(set, 1, nullptr, tns.data(), nullptr, woff.data(), wps.data(), stop.data(), &np,
                                           &status) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(tpamd_planner_set_set_waypoints(set, 1, nullptr, woff.data(), wps.data(), 0.2, vm.data(), am.data(), dl.data(),
                                            nullptr, &np, &status) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(tpamd_planner_set_set_waypoints_device(set, 1, nullptr, woff.data(), wps.data(), 0.2, vm.data(), am.data(),
                                                   dl.data(), nullptr, &np, &status, nullptr) == TPAMD_E_INVALID_ARGUMENT);
      // call-level errors of the upload
      auto upload1 = [&](const int32_t *ids, int count, std::vector<int32_t> off, double delta, int state) {
        std::vector<double> pe(2, t.path_end), vt(2, t.vt), vr(2, t.vr), d2(2, delta), vm2, am2, q, J;
        std::vector<int32_t> st2(2, state);
        for (int k = 0; k < 2; k++) {
          vm2.insert(vm2.end(), t.vmax.begin(), t.vmax.end());
          am2.insert(am2.end(), t.amax.begin(), t.amax.end());
          q.insert(q.end(), t.q.begin(), t.q.end());
          J.insert(J.end(), t.J.begin(), t.J.end());
        }
        return tpamd_planner_set_upload_ik_tables(set, count, ids, off.data(), q.data(), J.data(), pe.data(), vm2.data(),
                                                  am2.data(), vt.data(), vr.data(), d2.data(), nullptr, st2.data());
      };
      const int32_t R = t.rows;
      const int32_t id_ok[2] = {0, 1}, id_rep[2] = {1, 1}, id_bad[2] = {0, B}, id_neg[2] = {-1, 0};
      CHECK(upload1(id_ok, 2, {0, kN - 1, kN - 1 + R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);   // fewer than N rows
      CHECK(upload1(id_ok, 2, {0, R, 2 * R}, 0.0, 1) == TPAMD_E_INVALID_ARGUMENT);                 // delta <= 0
      CHECK(upload1(id_ok, 2, {0, R, 2 * R}, -t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(upload1(id_rep, 2, {0, R, 2 * R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);            // repeated id
      CHECK(upload1(id_bad, 2, {0, R, 2 * R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);            // bad id
      CHECK(upload1(id_neg, 2, {0, R, 2 * R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(upload1(id_ok, 2, {1, R, 2 * R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);             // offsets[0] != 0
      CHECK(upload1(id_ok, 2, {0, 2 * R, R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);             // decreasing
      CHECK(upload1(id_ok, 2, {0, R, 2 * R}, t.delta, 3) == TPAMD_E_INVALID_ARGUMENT);             // state
      CHECK(upload1(id_ok, -1, {0, R, 2 * R}, t.delta, 1) == TPAMD_E_INVALID_ARGUMENT);
      CHECK(upload1(id_ok, 0, {0}, t.delta, 1) == 0);                                              // nothing listed
    }
    // the oracles
    ParallelFor(B, [&](int b) { rc[b] = tpo_planner_plan(orc[b], start[b], horizon[b]); });
    plans++;
    for (int b = 0; b < B; b++) windows += tpo_planner_windows(orc[b]);
    if (!o.failures)
      for (int b = 0; b < B; b++) CHECK(rc[b] == TPO_PLAN_OK);     // the condition of tests 1 and 2
    if (set) {
      CHECK(tpamd_planner_set_plan(set, start.data(), horizon.data(), sm.data()) == 0);
      CHECK(Download(set, B, D, &tr));
      int max_windows = 0;
      for (int b = 0; b < B; b++) {
        max_windows = std::max(max_windows, sm[b].windows);
        if (diverged[b]) continue;
        if (rc[b] != TPO_PLAN_OK) {
          // a failed planner: the status at this call, then it is compared no further
          CHECK(o.failures && sm[b].status == rc[b]);
          if (b == short_planner && rc[b] == TPO_PLAN_INTERNAL && sm[b].status == TPAMD_PLAN_INTERNAL) internal_at = step;
          if (b == iv_planner && rc[b] == TPO_PLAN_INVALID_ARGUMENT && sm[b].status == TPAMD_PLAN_INVALID_ARGUMENT)
            invalid_at = step;
          diverged[b] = 1;
          continue;
        }
        const int bad = Compare(sm[b], tr, b, D, orc[b], rc[b]);
        CHECK(bad == 0);
        if (bad && ++reported <= 10)
          std::printf("  %s step %d planner %d: differences 0x%x (status %d / oracle %d, samples %d / %d, windows %d / %d)\n",
                      o.name, step, b, bad, sm[b].status, rc[b], sm[b].num_samples, tpo_planner_num_samples(orc[b]),
                      sm[b].windows, tpo_planner_windows(orc[b]));
        compared++;
      }
      // test 9: 24 B up; one summary record per planner, one word pair for the prologue and one per
      // window iteration, one per resample attempt (one: the trajectory buffers never grow here) down
      if (!o.failures) {
        size_t up = 0, down = 0;
        tpamd_planner_set_last_plan_bytes(set, &up, &down);
        CHECK(up == (size_t)24 * B);
        CHECK(down == (size_t)56 * B + 8 * ((size_t)max_windows + 1) + 8);
      }
    }
    int all_done = 1;
    for (int b = 0; b < B; b++) {
      if (rc[b] != TPO_PLAN_OK) continue;               // failed planners keep their start
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
  if (!o.failures) CHECK(at_end == B);                  // every planner ends with target_reached
  if (o.failures) {
    CHECK(at_end == B - 2);
    if (set) {
      CHECK(internal_at > 0);                           // at the last window's Plan, not before
      CHECK(invalid_at == 0);
    }
  }
  if (o.modify) CHECK(modified >= B / 3 - 1);
  std::printf("%s: D %d %s B %d: %d Plan calls, %ld windows, %d planner-plans compared, %d at the end%s\n", o.name, D,
              o.method ? "skip" : "uniform", B, plans, windows, compared, at_end, g_fail ? " (FAILURES)" : "");
  if (o.failures && set) std::printf("  failures: internal at Plan %d, invalid argument at Plan %d\n", internal_at, invalid_at);
  for (auto *p : orc) tpo_planner_destroy(p);
  if (set) tpamd_planner_set_destroy(set);
  return plans;
}

// test 6: tables in device memory on a non-blocking stream against the host entry
static void TestDeviceUpload(tpamd_engine *e) {
  const int B = 64, D = 7;
  std::vector<Table> fam = MakeFamily(B, D, 52000);
  int longest = 0;
  for (const Table &t : fam) longest = std::max(longest, t.rows);
  tpamd_planner_set *host = MakeSet(e, B, D, 0, longest), *dev = MakeSet(e, B, D, 0, kN);   // dev grows first
  if (!host || !dev) return;
  std::vector<int32_t> ids(B), off(B + 1, 0), st(B, 1);
  for (int b = 0; b < B; b++) ids[b] = B - 1 - b;        // listed in reverse order
  std::vector<const Table *> ptr(B);
  for (int k = 0; k < B; k++) { ptr[k] = &fam[ids[k]]; off[k + 1] = off[k] + ptr[k]->rows; }
  CHECK(Upload(host, ids, ptr, nullptr, 1) == 0);
  std::vector<double> q((size_t)off[B] * D), J((size_t)off[B] * 6 * D), pe(B), vm((size_t)B * D), am((size_t)B * D), vt(B), vr(B),
      dl(B);
  for (int k = 0; k < B; k++) {
    const Table &t = *ptr[k];
    std::memcpy(&q[(size_t)off[k] * D], t.q.data(), t.q.size() * 8);
    std::memcpy(&J[(size_t)off[k] * 6 * D], t.J.data(), t.J.size() * 8);
    std::memcpy(&vm[(size_t)k * D], t.vmax.data(), D * 8);
    std::memcpy(&am[(size_t)k * D], t.amax.data(), D * 8);
    pe[k] = t.path_end; vt[k] = t.vt; vr[k] = t.vr; dl[k] = t.delta;
  }
  hipStream_t stream = nullptr;
  HIP_OK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
  double *dq = nullptr, *dJ = nullptr, *dsmall = nullptr;
  int32_t *dst = nullptr;
  const size_t nsmall = (size_t)B * (4 + 2 * D);
  HIP_OK(hipMalloc((void **)&dq, q.size() * 8));
  HIP_OK(hipMalloc((void **)&dJ, J.size() * 8));
  HIP_OK(hipMalloc((void **)&dsmall, nsmall * 8));
  HIP_OK(hipMalloc((void **)&dst, B * 4));
  std::vector<double> small;
  for (const auto *v : {&pe, &vt, &vr, &dl, &vm, &am}) small.insert(small.end(), v->begin(), v->end());
  HIP_OK(hipMemcpyAsync(dq, q.data(), q.size() * 8, hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemcpyAsync(dJ, J.data(), J.size() * 8, hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemcpyAsync(dsmall, small.data(), nsmall * 8, hipMemcpyHostToDevice, stream));
  HIP_OK(hipMemcpyAsync(dst, st.data(), B * 4, hipMemcpyHostToDevice, stream));
  const double *dpe = dsmall, *dvt = dsmall + B, *dvr = dsmall + 2 * B, *ddl = dsmall + 3 * B, *dvm = dsmall + 4 * B,
               *dam = dsmall + 4 * B + (size_t)B * D;
  CHECK(tpamd_planner_set_upload_ik_tables_device(dev, B, ids.data(), off.data(), dq, dJ, dpe, dvm, dam, dvt, dvr, ddl,
                                                  nullptr, dst, stream) == 0);
  // the Plan right behind it (null stream) is ordered after the upload
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<tpamd_planner_summary> s1(B), s2(B);
  Trajectories t1, t2;
  int same = 0, plans = 0;
  for (int step = 0; step < 12; step++) {
    CHECK(tpamd_planner_set_plan(dev, start.data(), horizon.data(), s1.data()) == 0);
    CHECK(tpamd_planner_set_plan(host, start.data(), horizon.data(), s2.data()) == 0);
    CHECK(Download(dev, B, D, &t1) && Download(host, B, D, &t2));
    bool eq = std::memcmp(s1.data(), s2.data(), B * sizeof(tpamd_planner_summary)) == 0 && t1.off == t2.off &&
              Same(t1.time.data(), t2.time.data(), t1.time.size()) && Same(t1.s.data(), t2.s.data(), t1.s.size()) &&
              Same(t1.sd.data(), t2.sd.data(), t1.sd.size()) && Same(t1.sdd.data(), t2.sdd.data(), t1.sdd.size()) &&
              Same(t1.q.data(), t2.q.data(), t1.q.size()) && Same(t1.qd.data(), t2.qd.data(), t1.qd.size()) &&
              Same(t1.qdd.data(), t2.qdd.data(), t1.qdd.size());
    CHECK(eq);
    same += eq;
    plans++;
    for (int b = 0; b < B; b++) {
      CHECK(s1[b].status == TPAMD_PLAN_OK && s1[b].num_samples > 0);
      if (!s1[b].target_reached) start[b] = std::min<int64_t>(s1[b].end_time_ns, start[b] + 200 * kMs);
    }
  }
  int tables = 0;
  for (int b = 0; b < B; b++) {
    int32_t rows = 0;
    std::vector<double> tq(fam[b].q.size()), tJ(fam[b].J.size());
    CHECK(tpamd_planner_set_download_ik_table(dev, b, &rows, tq.data(), tJ.data(), fam[b].rows) == 0 && rows == fam[b].rows);
    tables += Same(tq.data(), fam[b].q.data(), tq.size()) && Same(tJ.data(), fam[b].J.data(), tJ.size());
  }
  CHECK(tables == B);
  std::printf("device upload against host upload: %d of %d Plan calls equal, %d tables equal\n", same, plans, tables);
  // what the host cannot check in device arrays, the kernel does: a delta that is not > 0 or a state
  // other than 1 / 2 leaves that planner without a path; the others are loaded
  {
    const int n = 4;
    tpamd_planner_set *s4 = MakeSet(e, n, D, 0, longest);
    std::vector<double> d4(dl.begin(), dl.begin() + n);
    std::vector<int32_t> st4(n, 1), off4(off.begin(), off.begin() + n + 1);
    d4[1] = -d4[1];
    st4[2] = 3;
    HIP_OK(hipMemcpyAsync(dsmall + 3 * B, d4.data(), n * 8, hipMemcpyHostToDevice, stream));
    HIP_OK(hipMemcpyAsync(dst, st4.data(), n * 4, hipMemcpyHostToDevice, stream));
    CHECK(s4 && tpamd_planner_set_upload_ik_tables_device(s4, n, nullptr, off4.data(), dq, dJ, dpe, dvm, dam, dvt, dvr, ddl,
                                                          nullptr, dst, stream) == 0);
    std::vector<int64_t> s0(n, 0), h0(n, 750 * kMs);
    std::vector<tpamd_planner_summary> sm4(n);
    CHECK(s4 && tpamd_planner_set_plan(s4, s0.data(), h0.data(), sm4.data()) == 0);
    CHECK(sm4[0].status == TPAMD_PLAN_OK && sm4[3].status == TPAMD_PLAN_OK && sm4[0].num_samples > 0);
    CHECK(sm4[1].status == TPAMD_PLAN_FAILED_PRECONDITION && sm4[2].status == TPAMD_PLAN_FAILED_PRECONDITION);
    std::printf("device upload with a bad delta and a bad state: statuses %d %d %d %d\n", sm4[0].status, sm4[1].status,
                sm4[2].status, sm4[3].status);
    if (s4) tpamd_planner_set_destroy(s4);
  }
  tpamd_planner_set_destroy(dev);
  tpamd_planner_set_destroy(host);
  HIP_OK(hipFree(dq)); HIP_OK(hipFree(dJ)); HIP_OK(hipFree(dsmall)); HIP_OK(hipFree(dst));
  HIP_OK(hipStreamDestroy(stream));
}

// test 8: the IK-table entries on a joint set change nothing
static void TestKindsOnJointSet(tpamd_engine *e) {
  const int B = 8, D = 6;
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 16;
  cfg.sampling_method = 0; cfg.max_planning_iterations = 200; cfg.constraint_safety = kSafety;
  cfg.max_initial_velocity_error = kMaxIvError; cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *a = nullptr, *b = nullptr;
  CHECK(tpamd_planner_set_create(e, &cfg, &a) == 0 && tpamd_planner_set_create(e, &cfg, &b) == 0);
  if (!a || !b) return;
  Rng rng(99);
  std::vector<int32_t> off(B + 1), np(B), st(B);
  std::vector<double> wps, vm((size_t)B * D), am((size_t)B * D), dl(B, 0.02);
  for (int k = 0; k < B; k++) {
    off[k] = (int32_t)(wps.size() / D);
    for (int i = 0; i < 4 * D; i++) wps.push_back(rng.uniform(-1.0, 1.0));
  }
  off[B] = (int32_t)(wps.size() / D);
  for (auto &v : vm) v = rng.uniform(0.5, 1.1);
  for (auto &v : am) v = rng.uniform(1.2, 3.0);
  for (tpamd_planner_set *s : {a, b})
    CHECK(tpamd_planner_set_set_waypoints(s, B, nullptr, off.data(), wps.data(), 0.2, vm.data(), am.data(), dl.data(),
                                          nullptr, np.data(), st.data()) == 0);
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<tpamd_planner_summary> s1(B), s2(B);
  CHECK(tpamd_planner_set_plan(a, start.data(), horizon.data(), s1.data()) == 0);
  CHECK(tpamd_planner_set_plan(b, start.data(), horizon.data(), s2.data()) == 0);
  // the IK-table entries on set a
  Table t = MakeTable(7, D, 0.4);
  std::vector<const Table *> ptr{&t};
  std::vector<int32_t> id0{0};
  CHECK(Upload(a, id0, ptr, nullptr, 1) == TPAMD_E_INVALID_ARGUMENT);
  int32_t rows = 0;
  CHECK(tpamd_planner_set_download_ik_table(a, 0, &rows, nullptr, nullptr, 0) == TPAMD_E_INVALID_ARGUMENT);
  {
    std::vector<int32_t> o2{0, t.rows}, one{1};
    CHECK(tpamd_planner_set_upload_ik_tables_device(a, 1, nullptr, o2.data(), t.q.data(), t.J.data(), &t.path_end,
                                                    t.vmax.data(), t.amax.data(), &t.vt, &t.vr, &t.delta, nullptr, one.data(),
                                                    nullptr) == TPAMD_E_INVALID_ARGUMENT);
  }
  for (int b2 = 0; b2 < B; b2++) start[b2] = 200 * kMs;
  CHECK(tpamd_planner_set_plan(a, start.data(), horizon.data(), s1.data()) == 0);
  CHECK(tpamd_planner_set_plan(b, start.data(), horizon.data(), s2.data()) == 0);
  Trajectories t1, t2;
  CHECK(Download(a, B, D, &t1) && Download(b, B, D, &t2));
  const bool eq = std::memcmp(s1.data(), s2.data(), B * sizeof(tpamd_planner_summary)) == 0 && t1.off == t2.off &&
                  Same(t1.time.data(), t2.time.data(), t1.time.size()) && Same(t1.q.data(), t2.q.data(), t1.q.size()) &&
                  Same(t1.qd.data(), t2.qd.data(), t1.qd.size()) && Same(t1.qdd.data(), t2.qdd.data(), t1.qdd.size());
  CHECK(eq && t1.time.size() > 0);
  for (int k = 0; k < B; k++) CHECK(s1[k].status == TPAMD_PLAN_OK);
  std::printf("IK-table entries on a joint set: refused, plans %s\n", eq ? "unchanged" : "CHANGED");
  tpamd_planner_set_destroy(a);
  tpamd_planner_set_destroy(b);
}

int main(int argc, char **argv) {
  const bool cpu_only = argc > 1 && std::strcmp(argv[1], "--cpu-check") == 0;
  tpamd_engine *e = nullptr;
  if (!cpu_only) {
    CHECK(tpamd_engine_create(0, &e) == 0);
    if (!e) { std::printf("no engine\n"); return 1; }
  }
  // 1 / 9: the synthetic family, generic rows kernel (D = 5) and the fused kernels (6, 7)
  for (int D : {5, 6, 7})
    for (int method : {0, 1}) {
      RunOptions o;
      o.B = 256; o.D = D; o.method = method; o.seed0 = 1000 * D + 100000 * method; o.cpu_only = cpu_only;
      o.name = "family";
      Run(e, o);
    }
  // 2 / 5: modified state; the second run starts with table_capacity = N and grows twice
  {
    RunOptions o;
    o.B = 120; o.D = 7; o.method = 0; o.seed0 = 31000; o.modify = true; o.cpu_only = cpu_only; o.name = "modified";
    Run(e, o);
    o.D = 6; o.method = 1; o.seed0 = 32000; o.table_capacity = kN; o.pad = 1100; o.name = "modified + growth";
    Run(e, o);
    o.D = 5; o.method = 0; o.seed0 = 33000; o.table_capacity = 0; o.pad = 0; o.B = 60; o.name = "modified";
    Run(e, o);
  }
  if (!cpu_only) {
    // 4 / 8: per-planner failures and refused calls
    for (int D : {5, 7}) {
      RunOptions o;
      o.B = 32; o.D = D; o.method = D == 5 ? 1 : 0; o.seed0 = 41000 + D; o.failures = true; o.name = "failures";
      Run(e, o);
    }
    TestDeviceUpload(e);
    TestKindsOnJointSet(e);
    tpamd_engine_destroy(e);
  }
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

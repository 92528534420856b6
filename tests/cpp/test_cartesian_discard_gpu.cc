// GPU test of discarding consumed IK rows through the C-ABI (run by tests/test_gpu_cartesian_discard.py):
// tpamd_planner_set_discard_ik_rows / _ik_table_info / _download_ik_rows on streaming Cartesian sets,
// against one oracle IK-table planner per planner on the FULL table (oracle/tp_oracle_plan.c) and
// against a streaming twin that never discards. Every comparison is bit for bit: a discard changes
// where rows live, not what is computed.
//
// The helpers and the shapes (B = 32, N = 64, 4 ms step, 750 ms horizon, a replan every 200 ms) are
// those of tests/cpp/test_cartesian_stream_gpu.cc, which is included for them; the paths are its
// family's at a smaller delta, at least 8 windows each.
//   compact D        1. the compaction alone: tables of 3, 64 and 333 random rows (and 1 live row, see
//                       TestCompaction) mixed in one set, keep_from from {0, 1, 2, live/2, live-1,
//                       rows+5}, a second discard on top, an append behind, a growth
//   walk D method    2. a walk with an automatic discard after every Plan: exact-need host appends and 7
//                       rows of lookahead through the _device append; 4. the same with the discard
//                       between plan_streaming and the append, while planners wait
//   norealloc        3. an append that fits after a discard does not reallocate; one that does not, grows
//   above            5. a keep_from above the floor fails that planner alone until a fresh upload
//   refusals         6. refused calls change nothing; download_ik_table on a discarded planner
#define main test_cartesian_stream_gpu_main
#include "test_cartesian_stream_gpu.cc"
#undef main

static Table RandomTable(unsigned long long seed, int D, int rows) {
  Rng rng(seed);
  Table t;
  t.D = D; t.rows = rows;
  t.delta = 0.01; t.path_end = 0.01 * (rows - 1); t.vt = 0.5; t.vr = 1.0;
  t.q.resize((size_t)rows * D); t.J.resize((size_t)rows * 6 * D);
  for (auto &v : t.q) v = rng.uniform(-3.0, 3.0);
  for (auto &v : t.J) v = rng.uniform(-3.0, 3.0);
  t.vmax.assign(D, 1.0); t.amax.assign(D, 2.0);
  return t;
}

// The streaming driver's family with a smaller delta: a window covers 1/8 or 1/10 of its path, so
// every path takes at least 8 windows (successive windows overlap, a path of 8 window lengths needs
// more than 8 of them).
static std::vector<Table> MakeLongFamily(int B, int D, unsigned long long seed0) {
  std::vector<Table> f(B);
  for (int b = 0; b < B; b++) f[b] = MakeTable(seed0 + b, D, (b % 2) ? 0.1 : 0.125);
  return f;
}

struct Info { int32_t first = -1, rows = -1, cap = -1; };
static Info GetInfo(tpamd_planner_set *set, int b) {
  Info i;
  CHECK(tpamd_planner_set_ik_table_info(set, b, &i.first, &i.rows, &i.cap) == 0);
  return i;
}

// the live rows of planner b equal path rows first .. rows-1 of t
static bool LiveEquals(tpamd_planner_set *set, int b, const Table &t, int first, int rows) {
  const int D = t.D, live = rows - first;
  int32_t f = -1, l = -1;
  if (tpamd_planner_set_download_ik_rows(set, b, &f, &l, nullptr, nullptr, 0) != 0 || f != first || l != live) return false;
  std::vector<double> q((size_t)live * D), J((size_t)live * 6 * D);
  if (live > 1) {          // one row too few is refused, with the counts written
    f = l = -1;
    if (tpamd_planner_set_download_ik_rows(set, b, &f, &l, q.data(), J.data(), live - 1) != TPAMD_E_INVALID_ARGUMENT ||
        f != first || l != live)
      return false;
  }
  if (tpamd_planner_set_download_ik_rows(set, b, &f, &l, q.data(), J.data(), live) != 0) return false;
  return Same(q.data(), &t.q[(size_t)first * D], q.size()) && Same(J.data(), &t.J[(size_t)first * 6 * D], J.size());
}

static int Choice(int c, int first, int rows) {
  const int live = rows - first;
  const int pick[6] = {0, 1, 2, live / 2, live - 1, rows + 5 - first};
  return first + pick[c % 6];
}
static int Clamp(int keep, int first, int rows) { return std::min(std::max(keep, first), rows - 1); }

// 1. A set of N = 3 (no Plan runs here), so that tables of 3, 64 and 333 rows upload; a table of one
// row cannot be uploaded (a table has at least num_samples >= 3 rows), so type 0 is a 3-row table
// whose first discard leaves ONE live row, and the discards on top of it run on that one row.
static void TestCompaction(tpamd_engine *e, int D) {
  const int B = 32, kRows[4] = {3, 3, 64, 333};
  tpamd_planner_set_config cfg{};
  cfg.num_planners = B; cfg.num_dofs = D; cfg.num_samples = 3; cfg.trajectory_capacity = 64;
  cfg.max_planning_iterations = 10; cfg.constraint_safety = kSafety; cfg.max_initial_velocity_error = kMaxIvError;
  cfg.time_step_ns = 4 * kMs;
  tpamd_planner_set *set = nullptr;
  CHECK(tpamd_planner_set_create_cartesian(e, &cfg, 333, &set) == 0);
  if (!set) return;
  const int kExtra = 9;                          // rows kept back for the appends
  std::vector<Table> fam(B);
  std::vector<int32_t> ids(B);
  std::vector<const Table *> ptr(B);
  std::vector<int> rows(B), first(B, 0);
  for (int b = 0; b < B; b++) {
    rows[b] = kRows[b % 4];
    fam[b] = RandomTable(5000 + 100 * D + b, D, rows[b] + kExtra);
    ids[b] = b; ptr[b] = &fam[b];
  }
  CHECK(Upload(set, ids, ptr, rows) == 0);
  for (int b = 0; b < B; b++) {
    const Info i = GetInfo(set, b);
    CHECK(i.first == 0 && i.rows == rows[b] && i.cap == 333);
  }
  {
    // type 0: down to one live row (keep_from = rows - 1), listed by id
    std::vector<int32_t> id0, keep0;
    for (int b = 0; b < B; b += 4) { id0.push_back(b); keep0.push_back(rows[b] - 1); }
    std::vector<int32_t> out(id0.size(), -1);
    CHECK(tpamd_planner_set_discard_ik_rows(set, (int)id0.size(), id0.data(), keep0.data(), out.data()) == 0);
    for (size_t k = 0; k < id0.size(); k++) { CHECK(out[k] == rows[id0[k]] - 1); first[id0[k]] = out[k]; }
  }
  int ok = 0, overlap_case = 0, moved = 0;
  for (int round = 0; round < 2; round++) {
    // round 0: the six choices; round 1: a second discard on top, the choice shifted by one
    std::vector<int32_t> keep(B), out(B, -1);
    for (int b = 0; b < B; b++) {
      keep[b] = Choice(b / 4 + round, first[b], rows[b]);
      const int nf = Clamp(keep[b], first[b], rows[b]);
      if (D == 7 && rows[b] == 333 && nf - first[b] == 1) overlap_case++;
      moved += nf > first[b];
    }
    CHECK(tpamd_planner_set_discard_ik_rows(set, B, nullptr, keep.data(), out.data()) == 0);
    for (int b = 0; b < B; b++) {
      const int nf = Clamp(keep[b], first[b], rows[b]);
      CHECK(out[b] == nf && out[b] >= first[b]);
      first[b] = nf;
      const Info i = GetInfo(set, b);
      CHECK(i.first == first[b] && i.rows == rows[b] && i.cap == 333);
      const bool same = LiveEquals(set, b, fam[b], first[b], rows[b]);
      CHECK(same);
      ok += same;
    }
  }
  if (D == 7) CHECK(overlap_case >= 1);       // 333 rows, shift 1: source and destination overlap
  CHECK(moved > 8);
  // an append lands behind the last row (4 rows, host entry; then 5 through the _device entry): the
  // undiscarded 333-row tables grow the capacity, first_row and the live rows survive
  for (int part = 0; part < 2; part++) {
    std::vector<int> from(rows), count(B, part ? 5 : 4);
    CHECK(Append(set, fam, ids, from, count, part == 1) == 0);
    for (int b = 0; b < B; b++) rows[b] += count[b];
    for (int b = 0; b < B; b++) {
      const bool same = LiveEquals(set, b, fam[b], first[b], rows[b]);
      CHECK(same);
      ok += same;
    }
  }
  CHECK(GetInfo(set, 0).cap == 666);
  // a discard of everything but the last row on the grown table, ids reversed
  {
    std::vector<int32_t> rid(B), keep(B), out(B);
    for (int k = 0; k < B; k++) { rid[k] = B - 1 - k; keep[k] = rows[rid[k]] + 100; }
    CHECK(tpamd_planner_set_discard_ik_rows(set, B, rid.data(), keep.data(), out.data()) == 0);
    for (int k = 0; k < B; k++) {
      const int b = rid[k];
      CHECK(out[k] == rows[b] - 1);
      first[b] = out[k];
      const bool same = LiveEquals(set, b, fam[b], first[b], rows[b]);
      CHECK(same);
      ok += same;
    }
  }
  std::printf("compaction D %d: %d of %d live-row readouts equal the uploaded slices, %d overlapping 333-row shifts by 1\n",
              D, ok, 5 * B, overlap_case);
  tpamd_planner_set_destroy(set);
}

struct DiscardWalk {
  int D = 7, method = 0;
  unsigned long long seed0 = 1;
  int extra = 0;
  bool device_append = false;
  bool while_waiting = false;      // 4: discard between plan_streaming and the append as well
  const char *name = "";
};

// one Plan of a streaming set, the appends included; *peak follows the largest live + appended rows
static void StreamPlan(tpamd_planner_set *set, const std::vector<Table> &fam, const std::vector<int64_t> &start,
                       const std::vector<int64_t> &horizon, std::vector<tpamd_planner_summary> *ss, int extra,
                       bool device, bool discard_waiting, int *peak, int *suspensions) {
  const int B = (int)fam.size();
  std::vector<int32_t> nf(B), nc(B);
  int32_t waiting = -1;
  CHECK(tpamd_planner_set_plan_streaming(set, start.data(), horizon.data(), ss->data(), nf.data(), nc.data(), &waiting) == 0);
  for (int round = 0; waiting > 0; round++) {
    CHECK(round < 64);
    if (round >= 64) break;
    *suspensions += waiting;
    if (discard_waiting) CHECK(tpamd_planner_set_discard_ik_rows(set, B, nullptr, nullptr, nullptr) == 0);
    std::vector<int32_t> ids;
    std::vector<int> first, count;
    for (int b = 0; b < B; b++) {
      if (nc[b] == 0) continue;
      const Info i = GetInfo(set, b);
      CHECK(nf[b] == i.rows);
      const int c = std::min(nc[b] + extra, fam[b].rows - nf[b]);
      ids.push_back(b); first.push_back(nf[b]); count.push_back(c);
      if (peak) *peak = std::max(*peak, i.rows - i.first + c);
    }
    CHECK(Append(set, fam, ids, first, count, device) == 0);
    CHECK(tpamd_planner_set_plan_resume(set, ss->data(), nf.data(), nc.data(), &waiting) == 0);
  }
}

// 2 / 4. The discarding set against its oracles and its twin at every Plan until target_reached.
static void WalkWithDiscards(tpamd_engine *e, const DiscardWalk &o) {
  const int B = kB, D = o.D;
  std::vector<Table> fam = MakeLongFamily(B, D, o.seed0);
  std::vector<tpo_planner *> orc(B);
  for (int b = 0; b < B; b++) orc[b] = MakeOracle(fam[b], o.method);
  tpamd_planner_set *disc = MakeSet(e, B, D, o.method, kN), *twin = MakeSet(e, B, D, o.method, kN);
  if (!disc || !twin) return;
  CHECK(UploadAll(disc, fam, kN) == 0 && UploadAll(twin, fam, kN) == 0);
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<int> rc(B, 0), reached(B, 0);
  std::vector<tpamd_planner_summary> sd(B), st(B);
  std::vector<int32_t> first(B, 0), out(B);
  Trajectories td, tt;
  int peak = kN, susp_d = 0, susp_t = 0, plans = 0, equal = 0, discards = 0, advanced = 0;
  std::vector<int> windows(B, 0);
  for (int step = 0; step < 300; step++) {
    for (int b = 0; b < B; b++) rc[b] = tpo_planner_plan(orc[b], start[b], horizon[b]);
    StreamPlan(twin, fam, start, horizon, &st, o.extra, o.device_append, false, nullptr, &susp_t);
    StreamPlan(disc, fam, start, horizon, &sd, o.extra, o.device_append, o.while_waiting, &peak, &susp_d);
    CHECK(Download(twin, B, D, &tt) && Download(disc, B, D, &td));
    const bool eq = SameSets(st, tt, sd, td, B, D);
    CHECK(eq);
    equal += eq;
    for (int b = 0; b < B; b++) CHECK(rc[b] == TPO_PLAN_OK && Compare(sd[b], td, b, D, orc[b], rc[b]) == 0);
    for (int b = 0; b < B; b++) windows[b] += sd[b].windows;
    plans++;
    // the automatic discard after the completed Plan
    CHECK(tpamd_planner_set_discard_ik_rows(disc, B, nullptr, nullptr, out.data()) == 0);
    discards++;
    for (int b = 0; b < B; b++) {
      const Info i = GetInfo(disc, b);
      CHECK(out[b] == i.first && out[b] >= first[b] && out[b] <= i.rows - 1);
      advanced += out[b] > first[b];
      first[b] = out[b];
    }
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
  int at_end = 0, positive = 0, same_rows = 0;
  for (int b = 0; b < B; b++) at_end += reached[b];
  CHECK(at_end == B && equal == plans);
  const int fewest = *std::min_element(windows.begin(), windows.end());
  CHECK(fewest >= 8);                                  // every path is at least 8 windows long
  CHECK(susp_d == susp_t && susp_d > 0);               // a discard never changes which rows a planner asks for
  for (int b = 0; b < B; b++) {
    const Info d = GetInfo(disc, b), t = GetInfo(twin, b);
    positive += d.first > 0;
    CHECK(t.first == 0 && d.rows == t.rows);
    int32_t r = -1;
    std::vector<double> q((size_t)t.rows * D), J((size_t)t.rows * 6 * D);
    CHECK(tpamd_planner_set_download_ik_table(twin, b, &r, q.data(), J.data(), t.rows) == 0 && r == t.rows);
    Table tw;                                          // the twin's table as the reference of the live rows
    tw.D = D; tw.rows = r; tw.q = q; tw.J = J;
    same_rows += LiveEquals(disc, b, tw, d.first, d.rows);
  }
  const int cap_d = GetInfo(disc, 0).cap, cap_t = GetInfo(twin, 0).cap;
  CHECK(positive == B && same_rows == B);
  CHECK(cap_d < cap_t);
  CHECK(cap_d < 2 * peak);             // growth is by doubling from N: arithmetic, not a measurement
  CHECK(tpamd_planner_set_device_bytes(disc) < tpamd_planner_set_device_bytes(twin));
  std::printf("%s: D %d %s: %d Plans equal to the oracles and the twin, %d discards, %d first rows advanced, "
              "%d suspensions, at least %d windows per planner, table capacity %d against the twin's %d (peak live + appended %d), %d of %d planners "
              "with first_row > 0, %d at the end%s\n",
              o.name, D, o.method ? "skip" : "uniform", equal, discards, advanced, susp_d, fewest, cap_d, cap_t, peak, positive, B,
              at_end, g_fail ? " (FAILURES)" : "");
  for (auto *p : orc) tpo_planner_destroy(p);
  tpamd_planner_set_destroy(disc);
  tpamd_planner_set_destroy(twin);
}

// 3. no reallocation where the rows fit into capacity - live
static void TestNoRealloc(tpamd_engine *e) {
  const int B = 4, D = 7;
  tpamd_planner_set *set = MakeSet(e, B, D, 0, 128);
  if (!set) return;
  std::vector<Table> fam(B);
  for (int b = 0; b < B; b++) fam[b] = RandomTable(9100 + b, D, 300);
  CHECK(UploadAll(set, fam, 100) == 0);
  const double *q0 = nullptr, *J0 = nullptr, *q1 = nullptr, *J1 = nullptr;
  CHECK(tpamd_planner_set_ik_table_device_pointers(set, &q0, &J0) == 0 && q0 && J0);
  std::vector<int32_t> ids{0, 1, 2, 3}, keep{60, 60, 70, 99}, out(B);
  CHECK(tpamd_planner_set_discard_ik_rows(set, B, nullptr, keep.data(), out.data()) == 0);
  for (int b = 0; b < B; b++) CHECK(out[b] == keep[b]);
  // 40 live + 80 = 120 <= 128: before the discard this append needed 180 rows and a growth
  CHECK(Append(set, fam, ids, {100, 100, 100, 100}, {80, 80, 80, 80}, false) == 0);
  CHECK(tpamd_planner_set_ik_table_device_pointers(set, &q1, &J1) == 0);
  const bool stayed = q1 == q0 && J1 == J0 && GetInfo(set, 0).cap == 128;
  CHECK(stayed);
  for (int b = 0; b < B; b++) CHECK(LiveEquals(set, b, fam[b], keep[b], 180));
  // the _device entry: 8 more rows still fit (128), no growth
  CHECK(Append(set, fam, {0, 1}, {180, 180}, {8, 8}, true) == 0);
  CHECK(tpamd_planner_set_ik_table_device_pointers(set, &q1, &J1) == 0 && q1 == q0 && J1 == J0 && GetInfo(set, 0).cap == 128);
  CHECK(LiveEquals(set, 0, fam[0], 60, 188) && LiveEquals(set, 1, fam[1], 60, 188));
  // one row more does not fit: the capacity doubles, live rows and first_row stay
  CHECK(Append(set, fam, {0}, {188}, {1}, false) == 0);
  CHECK(tpamd_planner_set_ik_table_device_pointers(set, &q1, &J1) == 0);
  const bool grew = GetInfo(set, 0).cap == 256 && q1 != q0;
  CHECK(grew);
  CHECK(LiveEquals(set, 0, fam[0], 60, 189) && LiveEquals(set, 1, fam[1], 60, 188) && LiveEquals(set, 2, fam[2], 70, 180) &&
        LiveEquals(set, 3, fam[3], 99, 180));
  std::printf("no reallocation: the fitting appends %s the table, the next one %s\n", stayed ? "kept" : "MOVED",
              grew ? "grew it to 256 rows" : "DID NOT GROW IT");
  tpamd_planner_set_destroy(set);
}

// 5. a keep_from above the floor
static void TestAboveFloor(tpamd_engine *e) {
  const int B = kB, D = 7, p = 11;
  std::vector<Table> fam = MakeLongFamily(B, D, 64000);
  tpamd_planner_set *disc = MakeSet(e, B, D, 0, kN), *twin = MakeSet(e, B, D, 0, kN);
  if (!disc || !twin) return;
  CHECK(UploadAll(disc, fam, kN) == 0 && UploadAll(twin, fam, kN) == 0);
  std::vector<int64_t> start(B, 0), horizon(B, 750 * kMs);
  std::vector<tpamd_planner_summary> sd(B), st(B);
  Trajectories td, tt;
  int susp = 0, others_equal = 0, others = 0, failed = 0, recovered = 0;
  // phase 0: three Plans with automatic discards, then planner p keeps only its last row; phase 1:
  // until planner p's Plan runs a window (a Plan that only erases reads no table row and still equals
  // the twin's), which fails; phase 2: the Plan after the fresh upload; 3: done
  int phase = 0;
  for (int step = 0; step < 40 && phase < 3; step++) {
    StreamPlan(twin, fam, start, horizon, &st, 0, false, false, nullptr, &susp);
    StreamPlan(disc, fam, start, horizon, &sd, 0, false, false, nullptr, &susp);
    CHECK(Download(twin, B, D, &tt) && Download(disc, B, D, &td));
    const bool p_windowed = st[p].windows > 0;
    const bool p_differs = phase == 2 || (phase == 1 && p_windowed);
    for (int b = 0; b < B; b++) {
      if (b == p && p_differs) continue;
      const bool same = std::memcmp(&sd[b], &st[b], sizeof(tpamd_planner_summary)) == 0 && SamePlanner(td, tt, b, D);
      CHECK(same);
      if (phase >= 1 && b != p) { others++; others_equal += same; }
    }
    if (phase == 2) {
      CHECK(sd[p].status == TPAMD_PLAN_OK && sd[p].num_samples > 0 && sd[p].windows > 0);
      recovered = sd[p].status == TPAMD_PLAN_OK && sd[p].num_samples > 0;
      phase = 3;
    } else if (phase == 1 && p_windowed) {
      CHECK(sd[p].status == TPAMD_PLAN_INTERNAL && st[p].status == TPAMD_PLAN_OK && !st[p].target_reached);
      failed = sd[p].status == TPAMD_PLAN_INTERNAL;
      // a table from row 0 again: first_row is 0. The failed Plan left the planner as it leaves a
      // reference planner, its trajectory cut at the Plan's start, where no later Plan can start
      // (GetTimeOffsetAfter finds nothing after it): as there, a reset comes before the new path.
      CHECK(GetInfo(disc, p).first > 0);
      CHECK(Upload(disc, {p}, {&fam[p]}, {0}) == 0);
      CHECK(GetInfo(disc, p).first == 0 && GetInfo(disc, p).rows == fam[p].rows);
      const int32_t id = p;
      CHECK(tpamd_planner_set_reset(disc, 1, &id) == 0);
      CHECK(Upload(disc, {p}, {&fam[p]}, {0}) == 0);
      CHECK(GetInfo(disc, p).first == 0 && GetInfo(disc, p).rows == fam[p].rows);
      phase = 2;
    }
    CHECK(tpamd_planner_set_discard_ik_rows(disc, B, nullptr, nullptr, nullptr) == 0);
    if (phase == 0 && step == 2) {
      // planner p keeps only its last row: far above its floor, the caller's responsibility
      const int32_t id = p, keep = 1 << 30;
      int32_t out = -1;
      CHECK(tpamd_planner_set_discard_ik_rows(disc, 1, &id, &keep, &out) == 0);
      CHECK(out == GetInfo(disc, p).rows - 1 && out > 0);
      phase = 1;
    }
    for (int b = 0; b < B; b++)
      if (!st[b].target_reached) start[b] = std::min<int64_t>(st[b].end_time_ns, start[b] + 200 * kMs);
  }
  CHECK(phase == 3 && failed && recovered);
  CHECK(others >= 2 * (B - 1) && others_equal == others);
  std::printf("keep_from above the floor: %s for that planner, %s neighbour Plans (%d) equal to the twin, %s after a fresh upload\n",
              failed ? "TPAMD_PLAN_INTERNAL" : "NO ERROR", others_equal == others ? "all" : "NOT ALL", others, recovered ? "plans again" : "DOES NOT PLAN");
  tpamd_planner_set_destroy(disc);
  tpamd_planner_set_destroy(twin);
}

// 6. refused calls change nothing
static void TestDiscardRefusals(tpamd_engine *e) {
  const int D = 7;
  {
    tpamd_planner_set_config cfg{};
    cfg.num_planners = 4; cfg.num_dofs = D; cfg.num_samples = kN; cfg.num_points = 16;
    cfg.max_planning_iterations = 200; cfg.constraint_safety = kSafety; cfg.max_initial_velocity_error = kMaxIvError;
    cfg.time_step_ns = 4 * kMs;
    tpamd_planner_set *j = nullptr;
    CHECK(tpamd_planner_set_create(e, &cfg, &j) == 0);
    if (!j) return;
    int32_t a = 7, b = 7, c = 7;
    double x = 0;
    const double *pq = nullptr;
    CHECK(tpamd_planner_set_discard_ik_rows(j, 1, nullptr, nullptr, &a) == TPAMD_E_INVALID_ARGUMENT && a == 7);
    CHECK(tpamd_planner_set_ik_table_info(j, 0, &a, &b, &c) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_download_ik_rows(j, 0, &a, &b, &x, &x, 1) == TPAMD_E_INVALID_ARGUMENT);
    CHECK(tpamd_planner_set_ik_table_device_pointers(j, &pq, nullptr) == TPAMD_E_INVALID_ARGUMENT);
    tpamd_planner_set_destroy(j);
  }
  const int B = 6;
  tpamd_planner_set *set = MakeSet(e, B, D, 0, 128);
  if (!set) return;
  std::vector<Table> fam(B);
  for (int b = 0; b < B; b++) fam[b] = RandomTable(9300 + b, D, 100);
  std::vector<int32_t> five{0, 1, 2, 3, 4};
  std::vector<const Table *> ptr5{&fam[0], &fam[1], &fam[2], &fam[3], &fam[4]};
  CHECK(Upload(set, five, ptr5, std::vector<int>(5, 0)) == 0);          // planner 5 has no table
  const int32_t id1 = 1, keep1 = 30;
  CHECK(tpamd_planner_set_discard_ik_rows(set, 1, &id1, &keep1, nullptr) == 0);
  auto unchanged = [&]() {
    bool ok = true;
    for (int b = 0; b < 5; b++) ok = ok && LiveEquals(set, b, fam[b], b == 1 ? 30 : 0, 100);
    const Info i5 = GetInfo(set, 5);
    return ok && i5.first == 0 && i5.rows == 0 && i5.cap == 128;
  };
  CHECK(unchanged());
  const int32_t rep[2] = {0, 0}, bad[2] = {0, B}, neg[2] = {-1, 0}, none[2] = {0, 5}, keep[7] = {50, 50, 50, 50, 50, 50, 50};
  int32_t out[7] = {-5, -5, -5, -5, -5, -5, -5};
  CHECK(tpamd_planner_set_discard_ik_rows(set, 2, rep, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, 2, bad, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, 2, neg, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, 2, none, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, B, nullptr, keep, out) == TPAMD_E_INVALID_ARGUMENT);   // planner 5 among 0..5
  CHECK(tpamd_planner_set_discard_ik_rows(set, B + 1, nullptr, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, -1, nullptr, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(nullptr, 1, nullptr, keep, out) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_discard_ik_rows(set, 0, nullptr, nullptr, nullptr) == 0);                 // nothing listed
  for (int32_t v : out) CHECK(v == -5);
  const bool same = unchanged();
  CHECK(same);
  CHECK(tpamd_planner_set_ik_table_info(set, B, nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  CHECK(tpamd_planner_set_ik_table_info(set, -1, nullptr, nullptr, nullptr) == TPAMD_E_INVALID_ARGUMENT);
  // download_ik_table: the discarded planner gets the error and the total row count, another one its table
  int32_t r = -1;
  std::vector<double> q((size_t)100 * D), J((size_t)100 * 6 * D);
  const bool refused = tpamd_planner_set_download_ik_table(set, 1, &r, q.data(), J.data(), 100) == TPAMD_E_INVALID_ARGUMENT && r == 100;
  CHECK(refused);
  r = -1;
  CHECK(tpamd_planner_set_download_ik_table(set, 1, &r, nullptr, nullptr, 0) == TPAMD_E_INVALID_ARGUMENT && r == 100);
  r = -1;
  CHECK(tpamd_planner_set_download_ik_table(set, 2, &r, q.data(), J.data(), 100) == 0 && r == 100);
  CHECK(Same(q.data(), fam[2].q.data(), q.size()) && Same(J.data(), fam[2].J.data(), J.size()));
  // reset: first_row is 0 again
  CHECK(tpamd_planner_set_reset(set, 1, &id1) == 0);
  CHECK(GetInfo(set, 1).first == 0 && GetInfo(set, 1).rows == 0);
  std::printf("refused discards: tables %s; download_ik_table on a discarded planner: %s\n", same ? "unchanged" : "CHANGED",
              refused ? "error and the total row count" : "NOT REFUSED");
  tpamd_planner_set_destroy(set);
}

// No argument: everything. "compact D", "walk D method", "norealloc", "above", "refusals".
int main(int argc, char **argv) {
  const bool all = argc < 2;
  auto is = [&](const char *m) { return all || std::strcmp(argv[1], m) == 0; };
  tpamd_engine *e = nullptr;
  CHECK(tpamd_engine_create(0, &e) == 0);
  if (!e) { std::printf("no engine\n"); return 1; }
  for (int D : {5, 6, 7}) {
    if (is("compact") && (argc < 3 || std::atoi(argv[2]) == D)) TestCompaction(e, D);
    for (int method : {0, 1}) {
      if (!is("walk") || (argc >= 4 && (std::atoi(argv[2]) != D || std::atoi(argv[3]) != method))) continue;
      DiscardWalk o;
      o.D = D; o.method = method; o.seed0 = 70000 + 1000 * D + 100000 * method;
      o.name = "exact";
      WalkWithDiscards(e, o);
      o.extra = 7; o.device_append = true; o.name = "ahead";
      WalkWithDiscards(e, o);
      o.extra = 0; o.device_append = false; o.while_waiting = true; o.name = "waiting";
      WalkWithDiscards(e, o);
    }
  }
  if (is("norealloc")) TestNoRealloc(e);
  if (is("above")) TestAboveFloor(e);
  if (is("refusals")) TestDiscardRefusals(e);
  tpamd_engine_destroy(e);
  if (g_fail) { std::printf("%d FAILURES\n", g_fail); return 1; }
  std::printf("ALL OK\n");
  return 0;
}

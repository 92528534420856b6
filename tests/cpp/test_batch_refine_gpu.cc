// GPU test of RefineSolutions on BatchPathTiming and BatchWaypointTiming (run by
// tests/test_gpu_refine_mirror.py): 16 paths of the shapes (joints, samples, waypoints) = (7, 33, 4)
// and (16, 33, 4), two rounds.
//   * with the option off (never set, or set and switched off again) the results are bit-equal and
//     carry no refine or check vectors;
//   * with it on, every path is held against tpamd_time_joint_paths_refined_host called here on the
//     same arrays: a path whose slot ended OK with fewer violated rows than its coarse solve carries
//     the slot's arrays (2 n - 1 or 4 n - 3 samples) and the slot's record, every other path its
//     coarse arrays and record; a cured path has violations == 0;
//   * sample_offset / joint_offset follow samples_per_path, and the arrays have their total length;
//   * the waypoint batch, which times the same splines, gives the same result.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/tpamd.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_path_timing.h"
#include "../../x-edr-trajectory-planning_amd/host/batch_waypoint_timing.h"
#include "test_support.h"

using namespace trajectory_planning;

template <class T>
static bool Same(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
static bool SameRange(const std::vector<double> &a, size_t at, const double *b, size_t n) {
  return at + n <= a.size() && (n == 0 || std::memcmp(a.data() + at, b, n * sizeof(double)) == 0);
}

static const size_t kPaths = 16;
static const double kTimeStart = 0.5;
static const int kRounds = 2;

static bool SameResult(const BatchTimingResult &a, const BatchTimingResult &b) {
  return Same(a.status, b.status) && Same(a.last_extremal_index, b.last_extremal_index) &&
         Same(a.samples_per_path, b.samples_per_path) && Same(a.dofs_per_path, b.dofs_per_path) &&
         Same(a.sample_offset, b.sample_offset) && Same(a.joint_offset, b.joint_offset) && Same(a.time, b.time) &&
         Same(a.s, b.s) && Same(a.sd, b.sd) && Same(a.sdd, b.sdd) && Same(a.q, b.q) && Same(a.qd, b.qd) &&
         Same(a.qdd, b.qdd) && Same(a.violations, b.violations) && Same(a.worst_sample, b.worst_sample) &&
         Same(a.worst_row, b.worst_row) && Same(a.worst_excess, b.worst_excess) &&
         Same(a.refine_rounds, b.refine_rounds) && Same(a.refine_slot_code, b.refine_slot_code) &&
         a.num_samples == b.num_samples && a.num_dofs == b.num_dofs;
}
static bool NoOptionFields(const BatchTimingResult &r) {
  return r.violations.empty() && r.worst_sample.empty() && r.worst_row.empty() && r.worst_excess.empty() &&
         r.refine_rounds.empty() && r.refine_slot_code.empty();
}

static void RunShape(tpamd_engine *engine, size_t D, size_t N, size_t W, unsigned long long seed) {
  auto rnd = [&]() { seed = seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(seed >> 11) / 9007199254740992.0; };
  std::vector<std::shared_ptr<TimeableJointSplinePath>> paths;
  BatchWaypointTiming wt;
  for (size_t b = 0; b < kPaths; b++) {
    std::vector<VectorXd> wps;
    for (size_t w = 0; w < W; w++) {
      VectorXd q(D);
      for (size_t d = 0; d < D; d++) q[d] = 4.0 * rnd() - 2.0;
      wps.push_back(q);
    }
    std::vector<double> vmax(D), amax(D);
    for (size_t d = 0; d < D; d++) { vmax[d] = 1.0 + rnd(); amax[d] = 2.0 + 2.0 * rnd(); }
    auto options = [&](double delta) {
      return JointPathOptions().set_num_dofs(D).set_num_path_samples(N).set_rounding(0.2).set_constraint_safety(0.8)
          .set_delta_parameter(delta);
    };
    TimeableJointSplinePath probe(options(0.01));
    CHECK(probe.SetWaypoints({wps.data(), wps.size()}).ok());
    const double delta = probe.knots().back() / (double)(N - 1);
    auto p = std::make_shared<TimeableJointSplinePath>(options(delta));
    CHECK(p->SetMaxJointVelocity({vmax.data(), vmax.size()}).ok());
    CHECK(p->SetMaxJointAcceleration({amax.data(), amax.size()}).ok());
    CHECK(p->SetWaypoints({wps.data(), wps.size()}).ok());
    paths.push_back(p);
    CHECK(wt.AddPath(wps, options(delta), {vmax.data(), vmax.size()}, {amax.data(), amax.size()}).ok());
  }

  // ---- the option off
  BatchTimingResult off, on, again;
  BatchPathTiming pt;
  CHECK(pt.SetPaths(paths).ok());
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &off).ok());
  RefineOptions ro;
  ro.max_rounds = kRounds;
  pt.RefineSolutions(ro);
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &on).ok());
  ro.enabled = false;
  pt.RefineSolutions(ro);
  CHECK(pt.ComputeTimingProfiles(kTimeStart, &again).ok());
  CHECK(NoOptionFields(off) && NoOptionFields(again) && SameResult(off, again));

  // ---- the C-ABI on the same arrays (one group: every path has D joints, P points, N samples)
  const size_t B = kPaths, P = (size_t)paths[0]->num_control_points(), NS = 4 * N - 3, M = B;
  std::vector<double> knots(B * (P + 3)), cps(B * P * D), vmax(B * D), amax(B * D), zero(B, 0.0), dl(B), t0(B, kTimeStart);
  for (size_t b = 0; b < B; b++) {
    const auto &p = *paths[b];
    CHECK((size_t)p.num_control_points() == P);
    std::copy(p.knots().begin(), p.knots().end(), knots.begin() + b * (P + 3));
    std::copy(p.packed_control_points().begin(), p.packed_control_points().end(), cps.begin() + b * P * D);
    for (size_t d = 0; d < D; d++) { vmax[b * D + d] = p.GetMaxJointVelocity()[d]; amax[b * D + d] = p.GetMaxJointAcceleration()[d]; }
    dl[b] = p.GetPathSamplingDistance();
  }
  std::vector<double> c_time(B * N), c_s(B * N), c_sd(B * N), c_sdd(B * N), c_q(B * N * D), c_qd(B * N * D), c_qdd(B * N * D);
  std::vector<int32_t> c_status(B, -1), c_lei(B, 0), c_viol(B, -9), c_ws(B, -9), c_wr(B, -9);
  std::vector<double> c_ex(B, 0.0);
  std::vector<double> r_time(M * NS), r_s(M * NS), r_sd(M * NS), r_sdd(M * NS), r_q(M * NS * D), r_qd(M * NS * D), r_qdd(M * NS * D), r_delta(M), r_ex(M);
  std::vector<int32_t> r_status(M, -1), r_lei(M, 0), slot(B, -9), slot_path(M, -9), num_refined(1, -9), rounds(M, -9),
      num_samples(M, -9), r_viol(M, -9), r_ws(M, -9), r_wr(M, -9);
  const tpamd_joint_batch bt{(int32_t)B, (int32_t)D, (int32_t)N, (int32_t)P, 0, 0, 0.8};
  const tpamd_joint_inputs in{knots.data(), cps.data(), vmax.data(), amax.data(), zero.data(), dl.data(), zero.data(),
                              zero.data(), t0.data(), nullptr};
  const tpamd_path_outputs out{c_time.data(), c_s.data(), c_sd.data(), c_sdd.data(), c_q.data(), c_qd.data(), c_qdd.data(),
                               c_lei.data(), nullptr, c_status.data(), nullptr};
  const tpamd_refine_options opt{kRounds, (int32_t)NS, (int32_t)M, 0, 0.0};
  tpamd_refine_outputs ref{};
  ref.check = tpamd_check_outputs{c_viol.data(), c_ex.data(), c_ws.data(), c_wr.data(), nullptr};
  ref.slot = slot.data(); ref.slot_path = slot_path.data(); ref.num_refined = num_refined.data();
  ref.rounds = rounds.data(); ref.num_samples = num_samples.data(); ref.delta = r_delta.data();
  ref.refined = tpamd_path_outputs{r_time.data(), r_s.data(), r_sd.data(), r_sdd.data(), r_q.data(), r_qd.data(),
                                   r_qdd.data(), r_lei.data(), nullptr, r_status.data(), nullptr};
  ref.refined_check = tpamd_check_outputs{r_viol.data(), r_ex.data(), r_ws.data(), r_wr.data(), nullptr};
  CHECK(tpamd_time_joint_paths_refined_host(engine, &bt, &in, &out, &opt, &ref) == 0);

  // ---- the option on, path by path
  CHECK(on.status.size() == B && on.refine_rounds.size() == B && on.refine_slot_code.size() == B &&
        on.violations.size() == B && on.sample_offset.size() == B + 1 && on.joint_offset.size() == B + 1);
  int refined = 0, cured = 0, carried = 0, kept_coarse = 0, two = 0;
  for (size_t b = 0; b < B && g_fail == 0; b++) {
    const int k = slot[b];
    CHECK(on.refine_slot_code[b] == k);
    CHECK(on.refine_rounds[b] == (k >= 0 ? rounds[k] : 0));
    CHECK(on.dofs_per_path[b] == (int32_t)D);
    const size_t n = (size_t)on.samples_per_path[b], so = on.sample_offset[b], jo = on.joint_offset[b];
    CHECK(on.sample_offset[b + 1] == so + n && on.joint_offset[b + 1] == jo + n * D);
    const bool takes = k >= 0 && r_status[k] == 0 && r_viol[k] >= 0 && r_viol[k] < c_viol[b];
    if (k >= 0) {
      refined++;
      two += rounds[k] == 2;
      CHECK(rounds[k] >= 1 && rounds[k] <= kRounds);
      CHECK((size_t)num_samples[k] == (rounds[k] == 1 ? 2 * N - 1 : 4 * N - 3));
    }
    if (takes) {
      carried++;
      CHECK(n == (size_t)num_samples[k] && (n == 2 * N - 1 || n == 4 * N - 3));
      CHECK(on.status[b] == 0 && on.last_extremal_index[b] == r_lei[k]);
      CHECK(on.violations[b] == r_viol[k] && on.worst_sample[b] == r_ws[k] && on.worst_row[b] == r_wr[k] &&
            std::memcmp(&on.worst_excess[b], &r_ex[k], sizeof(double)) == 0);
      CHECK(SameRange(on.time, so, &r_time[k * NS], n) && SameRange(on.s, so, &r_s[k * NS], n) &&
            SameRange(on.sd, so, &r_sd[k * NS], n) && SameRange(on.sdd, so, &r_sdd[k * NS], n));
      CHECK(SameRange(on.q, jo, &r_q[k * NS * D], n * D) && SameRange(on.qd, jo, &r_qd[k * NS * D], n * D) &&
            SameRange(on.qdd, jo, &r_qdd[k * NS * D], n * D));
      if (r_viol[k] == 0) {
        cured++;
        CHECK(on.violations[b] == 0);
      }
    } else {
      // the coarse solution: what the result without the option carries for this path
      kept_coarse += k >= 0;
      CHECK(n == N && on.status[b] == c_status[b] && on.status[b] == off.status[b]);
      CHECK(on.last_extremal_index[b] == off.last_extremal_index[b]);
      CHECK(on.violations[b] == c_viol[b] && on.worst_sample[b] == c_ws[b] && on.worst_row[b] == c_wr[b] &&
            std::memcmp(&on.worst_excess[b], &c_ex[b], sizeof(double)) == 0);
      CHECK(SameRange(on.time, so, &off.time[off.sample_offset[b]], n) && SameRange(on.s, so, &off.s[off.sample_offset[b]], n) &&
            SameRange(on.sd, so, &off.sd[off.sample_offset[b]], n) && SameRange(on.sdd, so, &off.sdd[off.sample_offset[b]], n));
      CHECK(SameRange(on.q, jo, &off.q[off.joint_offset[b]], n * D) && SameRange(on.qd, jo, &off.qd[off.joint_offset[b]], n * D) &&
            SameRange(on.qdd, jo, &off.qdd[off.joint_offset[b]], n * D));
      if (on.status[b] == 0)
        CHECK(SameRange(on.time, so, &c_time[b * N], n) && SameRange(on.sdd, so, &c_sdd[b * N], n));
      // a refined path is left with its coarse arrays only if refinement did not reduce its violated rows
      if (k >= 0) CHECK(r_status[k] != 0 || r_viol[k] >= c_viol[b]);
    }
  }
  CHECK(on.time.size() == on.sample_offset[B] && on.s.size() == on.sample_offset[B] && on.sd.size() == on.sample_offset[B] &&
        on.sdd.size() == on.sample_offset[B]);
  CHECK(on.q.size() == on.joint_offset[B] && on.qd.size() == on.joint_offset[B] && on.qdd.size() == on.joint_offset[B]);
  CHECK(refined == num_refined[0] && refined >= 2 && cured >= 1);
  std::printf("BatchPathTiming (%zu, %zu, %zu): %d refined, %d in two rounds, %d carry the refined arrays, %d of them cured, "
              "%d keep the coarse arrays\n", D, N, W, refined, two, carried, cured, kept_coarse);

  // ---- the waypoint batch: the same splines, the same result
  BatchTimingResult woff, won, wagain;
  wt.CoverWholePath(true);
  CHECK(wt.ComputeTimingProfiles(kTimeStart, &woff).ok());
  ro.enabled = true;
  wt.RefineSolutions(ro);
  CHECK(wt.ComputeTimingProfiles(kTimeStart, &won).ok());
  ro.enabled = false;
  wt.RefineSolutions(ro);
  CHECK(wt.ComputeTimingProfiles(kTimeStart, &wagain).ok());
  CHECK(NoOptionFields(woff) && NoOptionFields(wagain) && SameResult(woff, wagain) && SameResult(woff, off));
  CHECK(SameResult(won, on));
  std::printf("BatchWaypointTiming (%zu, %zu, %zu): equal to BatchPathTiming: %s\n", D, N, W, SameResult(won, on) ? "yes" : "NO");
}

int main() {
  tpamd_engine *engine = nullptr;
  if (tpamd_engine_create(0, &engine) != 0) {
    std::printf("FAIL: no engine\n");
    return 1;
  }
  RunShape(engine, 7, 33, 4, 20271);
  RunShape(engine, 16, 33, 4, 20272);
  tpamd_engine_destroy(engine);
  if (g_fail == 0) std::printf("ALL OK\n");
  return g_fail ? 1 : 0;
}

#include "batch_path_timing.h"

#include <algorithm>
#include <limits>
#include <map>
#include <thread>
#include <tuple>

#include "engine_handle.h"

namespace trajectory_planning {

using ::tpamd::compat::InternalError;
using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::OkStatus;

Status BatchPathTiming::SetPaths(const std::vector<std::shared_ptr<TimeableJointSplinePath>> &paths) {
  if (paths.empty()) return InvalidArgumentError("no paths");
  for (const auto &p : paths) {
    if (!p) return InvalidArgumentError("null path");
    if (p->num_control_points() < 3) return InvalidArgumentError("path without a spline");
  }
  paths_ = paths;
  return OkStatus();
}

void PrepareCheckResult(bool on, size_t num_paths, BatchTimingResult *r) {
  r->violations.clear(); r->worst_sample.clear(); r->worst_row.clear(); r->worst_excess.clear();
  r->refine_rounds.clear(); r->refine_slot_code.clear();
  if (!on) return;
  r->violations.assign(num_paths, -1); r->worst_sample.assign(num_paths, -1); r->worst_row.assign(num_paths, -1);
  r->worst_excess.assign(num_paths, std::numeric_limits<double>::quiet_NaN());
}

tpamd_check_outputs CheckRecords::outputs() {
  return tpamd_check_outputs{violations.data(), worst_excess.data(), worst_sample.data(), worst_row.data(), nullptr};
}

void CheckRecords::scatter(const std::vector<size_t> &ids, BatchTimingResult *r) const {
  for (size_t i = 0; i < ids.size(); i++) {
    r->violations[ids[i]] = violations[i]; r->worst_sample[ids[i]] = worst_sample[i];
    r->worst_row[ids[i]] = worst_row[i]; r->worst_excess[ids[i]] = worst_excess[i];
  }
}

RefinedGroup::RefinedGroup(size_t B_, size_t N_, size_t D_, const RefineOptions &o)
    : B(B_), N(N_), D(D_), opt(o), check(B_), refined_check(0) {
  M = o.max_refined > 0 ? (size_t)o.max_refined : B;
  if (o.max_samples > 0) {
    NS = (size_t)o.max_samples;
  } else {
    NS = N;
    for (int r = 0; r < o.max_rounds && 2 * NS - 1 <= 8192; r++) NS = 2 * NS - 1;
  }
  refined_check = CheckRecords(M);
  slot.assign(B, -1); slot_path.assign(M, -1); num_refined.assign(1, 0);
  rounds.assign(M, 0); num_samples.assign(M, 0); status.assign(M, -1); lei.assign(M, 0);
  delta.assign(M, 0.0);
  time.resize(M * NS); s.resize(M * NS); sd.resize(M * NS); sdd.resize(M * NS);
  q.resize(M * NS * D); qd.resize(M * NS * D); qdd.resize(M * NS * D);
}

tpamd_refine_options RefinedGroup::options() const {
  return tpamd_refine_options{opt.max_rounds, (int32_t)NS, (int32_t)M, 0, opt.tolerance};
}

tpamd_refine_outputs RefinedGroup::outputs() {
  tpamd_refine_outputs o{};
  o.check = check.outputs();
  o.slot = slot.data(); o.slot_path = slot_path.data(); o.num_refined = num_refined.data();
  o.rounds = rounds.data(); o.num_samples = num_samples.data(); o.delta = delta.data();
  o.refined = tpamd_path_outputs{time.data(), s.data(), sd.data(), sdd.data(), q.data(), qd.data(), qdd.data(),
                                 lei.data(), nullptr, status.data(), nullptr};
  o.refined_check = refined_check.outputs();
  return o;
}

PathSolution RefinedGroup::Solution(size_t i, size_t samples, const tpamd_path_outputs &c,
                                    bool keep_last_extremal_index) const {
  PathSolution p;
  p.dofs = (int32_t)D;
  p.slot_code = slot[i];
  const int k = slot[i];
  if (k >= 0) p.rounds = rounds[k];
  const bool refined = k >= 0 && status[k] == 0 && refined_check.violations[k] >= 0 &&
                       refined_check.violations[k] < check.violations[i];
  // the arrays the path carries: row `row` of arrays of stride `stride`
  const size_t row = refined ? (size_t)k : i, stride = refined ? NS : N;
  const size_t n = refined ? (size_t)num_samples[k] : samples;
  const CheckRecords &rec = refined ? refined_check : check;
  p.status = refined ? status[k] : c.status[i];
  if (refined) p.last_extremal_index = lei[k];
  else if (keep_last_extremal_index) p.last_extremal_index = c.last_extremal_index[i];
  p.samples = (int32_t)n;
  p.violations = rec.violations[row]; p.worst_sample = rec.worst_sample[row]; p.worst_row = rec.worst_row[row];
  p.worst_excess = rec.worst_excess[row];
  p.time.assign(n, 0.0); p.s.assign(n, 0.0); p.sd.assign(n, 0.0); p.sdd.assign(n, 0.0);
  p.q.assign(n * D, 0.0); p.qd.assign(n * D, 0.0); p.qdd.assign(n * D, 0.0);
  if (p.status != 0) return p;
  const tpamd_path_outputs from = refined ? tpamd_path_outputs{const_cast<double *>(time.data()), const_cast<double *>(s.data()),
                                                               const_cast<double *>(sd.data()), const_cast<double *>(sdd.data()),
                                                               const_cast<double *>(q.data()), const_cast<double *>(qd.data()),
                                                               const_cast<double *>(qdd.data()), nullptr, nullptr, nullptr, nullptr}
                                          : c;
  std::copy_n(from.time + row * stride, n, p.time.begin());
  std::copy_n(from.s + row * stride, n, p.s.begin());
  std::copy_n(from.sd + row * stride, n, p.sd.begin());
  std::copy_n(from.sdd + row * stride, n, p.sdd.begin());
  std::copy_n(from.q + row * stride * D, n * D, p.q.begin());
  std::copy_n(from.qd + row * stride * D, n * D, p.qd.begin());
  std::copy_n(from.qdd + row * stride * D, n * D, p.qdd.begin());
  return p;
}

void PackRefinedResult(const std::vector<PathSolution> &paths, BatchTimingResult *r) {
  const size_t Bt = paths.size();
  r->status.resize(Bt); r->last_extremal_index.resize(Bt);
  r->samples_per_path.resize(Bt); r->dofs_per_path.resize(Bt);
  r->sample_offset.assign(Bt + 1, 0); r->joint_offset.assign(Bt + 1, 0);
  r->violations.resize(Bt); r->worst_sample.resize(Bt); r->worst_row.resize(Bt); r->worst_excess.resize(Bt);
  r->refine_rounds.resize(Bt); r->refine_slot_code.resize(Bt);
  r->num_samples = 0; r->num_dofs = 0;
  r->time.clear(); r->s.clear(); r->sd.clear(); r->sdd.clear(); r->q.clear(); r->qd.clear(); r->qdd.clear();
  for (size_t b = 0; b < Bt; b++) {
    const PathSolution &p = paths[b];
    r->status[b] = p.status; r->last_extremal_index[b] = p.last_extremal_index;
    r->samples_per_path[b] = p.samples; r->dofs_per_path[b] = p.dofs;
    r->sample_offset[b + 1] = r->sample_offset[b] + (size_t)p.samples;
    r->joint_offset[b + 1] = r->joint_offset[b] + (size_t)p.samples * (size_t)p.dofs;
    r->num_samples = std::max(r->num_samples, (int)p.samples);
    r->num_dofs = std::max(r->num_dofs, (int)p.dofs);
    r->violations[b] = p.violations; r->worst_sample[b] = p.worst_sample; r->worst_row[b] = p.worst_row;
    r->worst_excess[b] = p.worst_excess;
    r->refine_rounds[b] = p.rounds; r->refine_slot_code[b] = p.slot_code;
    r->time.insert(r->time.end(), p.time.begin(), p.time.end());
    r->s.insert(r->s.end(), p.s.begin(), p.s.end());
    r->sd.insert(r->sd.end(), p.sd.begin(), p.sd.end());
    r->sdd.insert(r->sdd.end(), p.sdd.begin(), p.sdd.end());
    r->q.insert(r->q.end(), p.q.begin(), p.q.end());
    r->qd.insert(r->qd.end(), p.qd.begin(), p.qd.end());
    r->qdd.insert(r->qdd.end(), p.qdd.begin(), p.qdd.end());
  }
}

namespace {
struct GroupKey {
  size_t dofs, points, bucket;
  double safety;
  bool operator<(const GroupKey &o) const {
    return std::tie(dofs, points, bucket, safety) < std::tie(o.dofs, o.points, o.bucket, o.safety);
  }
};
// host arrays of one group, in the layout of the C-ABI's joint form
struct GroupArrays {
  std::vector<size_t> ids;
  size_t B = 0, D = 0, P = 0, N = 0;
  bool ragged = false;
  double safety = 0.8;
  std::vector<double> knots, cps, vmax, amax, ps, dl, sd0, sdd0, t0;
  std::vector<int32_t> ns;
  std::vector<double> time, s, sd, sdd, q, qd, qdd;
  std::vector<int32_t> status, lei;
  std::vector<double> sd2;   // CheckSolutions only
};
}  // namespace

Status BatchPathTiming::SetDevices(const std::vector<int> &devices) {
  const int visible = ::tpamd::device_count();
  for (size_t i = 0; i < devices.size(); i++) {
    if (devices[i] < 0 || devices[i] >= visible) return InvalidArgumentError("no such device");
    for (size_t j = 0; j < i; j++)
      if (devices[j] == devices[i]) return InvalidArgumentError("device listed twice");
  }
  devices_ = devices;
  return OkStatus();
}

Status BatchPathTiming::ComputeTimingProfiles(double time_start_sec, BatchTimingResult *r) {
  if (paths_.empty()) return InvalidArgumentError("SetPaths first");
  const size_t Bt = paths_.size();
  r->status.assign(Bt, -1); r->last_extremal_index.assign(Bt, 0);
  r->samples_per_path.resize(Bt); r->dofs_per_path.resize(Bt);
  r->sample_offset.assign(Bt + 1, 0); r->joint_offset.assign(Bt + 1, 0);
  r->num_samples = 0; r->num_dofs = 0;
  std::vector<double> cost(Bt);
  for (size_t b = 0; b < Bt; b++) {
    const auto &p = *paths_[b];
    const size_t n = p.NumPathSamples(), d = p.NumDofs();
    r->samples_per_path[b] = (int32_t)n; r->dofs_per_path[b] = (int32_t)d;
    r->sample_offset[b + 1] = r->sample_offset[b] + n;
    r->joint_offset[b + 1] = r->joint_offset[b] + n * d;
    r->num_samples = std::max(r->num_samples, (int)n);
    r->num_dofs = std::max(r->num_dofs, (int)d);
    cost[b] = (double)n * (2.0 * d) * (2.0 * d);            // samples x rows^2
  }
  r->time.resize(r->sample_offset[Bt]); r->s.resize(r->sample_offset[Bt]);
  r->sd.resize(r->sample_offset[Bt]); r->sdd.resize(r->sample_offset[Bt]);
  r->q.resize(r->joint_offset[Bt]); r->qd.resize(r->joint_offset[Bt]); r->qdd.resize(r->joint_offset[Bt]);

  PrepareCheckResult(check_solutions_, Bt, r);

  const std::vector<int> devices = devices_.empty() ? std::vector<int>{::tpamd::default_device()} : devices_;
  const int nd = (int)devices.size();
  std::vector<int32_t> begin(nd + 1);
  tpamd_shard_bounds_balanced((int)Bt, cost.data(), nd, begin.data());
  // one host thread per device; each block writes its own part of the (packed) result
  // RefineSolutions: every block fills its paths' entries here, and the result is packed afterwards
  std::vector<PathSolution> refined(refine_.enabled ? Bt : 0);
  std::vector<PathSolution> *rp = refine_.enabled ? &refined : nullptr;
  std::vector<Status> st(nd, OkStatus());
  std::vector<std::thread> threads;
  for (int k = 1; k < nd; k++)
    threads.emplace_back([&, k] { st[k] = ComputeBlock(devices[k], begin[k], begin[k + 1], time_start_sec, r, rp); });
  st[0] = ComputeBlock(devices[0], begin[0], begin[1], time_start_sec, r, rp);
  for (auto &t : threads) t.join();
  for (const Status &s : st)
    if (!s.ok()) return s;
  if (rp) PackRefinedResult(refined, r);
  return OkStatus();
}

Status BatchPathTiming::ComputeBlock(int device, size_t lo, size_t hi, double time_start_sec,
                                     BatchTimingResult *r, std::vector<PathSolution> *refined) const {
  if (hi <= lo) return OkStatus();
  ::tpamd::EngineLease lease = ::tpamd::acquire_engine(device);
  tpamd_engine *engine = lease.get();
  if (!engine) return InternalError("no GPU engine");
  std::map<GroupKey, std::vector<size_t>> keyed;
  for (size_t b = lo; b < hi; b++) {
    const auto &p = *paths_[b];
    const size_t n = p.NumPathSamples();
    const size_t bucket = sample_bucket_ > 0 ? (n + sample_bucket_ - 1) / sample_bucket_ : 0;
    keyed[GroupKey{p.NumDofs(), (size_t)p.num_control_points(), bucket, p.options().constraint_safety()}]
        .push_back(b);
  }
  std::vector<GroupArrays> groups;
  groups.reserve(keyed.size());
  for (const auto &kv : keyed) {
    groups.emplace_back();
    GroupArrays &g = groups.back();
    g.ids = kv.second;
    g.B = g.ids.size(); g.D = kv.first.dofs; g.P = kv.first.points; g.safety = kv.first.safety;
    for (size_t b : g.ids) {
      g.ragged = g.ragged || (g.N != 0 && paths_[b]->NumPathSamples() != g.N);
      g.N = std::max(g.N, paths_[b]->NumPathSamples());
    }
    const size_t B = g.B, D = g.D, P = g.P, N = g.N;
    g.knots.resize(B * (P + 3)); g.cps.resize(B * P * D); g.vmax.resize(B * D); g.amax.resize(B * D);
    g.ps.assign(B, 0.0); g.dl.resize(B); g.sd0.assign(B, 0.0); g.sdd0.assign(B, 0.0); g.t0.assign(B, time_start_sec);
    g.ns.resize(B);
    for (size_t i = 0; i < B; i++) {
      const auto &p = *paths_[g.ids[i]];
      std::copy(p.knots().begin(), p.knots().end(), g.knots.begin() + i * (P + 3));
      std::copy(p.packed_control_points().begin(), p.packed_control_points().end(), g.cps.begin() + i * P * D);
      for (size_t d = 0; d < D; d++) {
        g.vmax[i * D + d] = p.GetMaxJointVelocity()[d];
        g.amax[i * D + d] = p.GetMaxJointAcceleration()[d];
      }
      g.dl[i] = p.GetPathSamplingDistance();
      g.ns[i] = (int32_t)p.NumPathSamples();
    }
    // start velocity: projection of the requested joint velocity on q'(0)
    // (path_timing_trajectory.cc:360-372); needs the first sample only
    {
      std::vector<double> q(B * D), q1(B * D), q2(B * D);
      const int rc = tpamd_sample_joint_paths_host(engine, (int)B, (int)D, 1, (int)P, g.knots.data(), g.cps.data(),
                                                   g.ps.data(), g.dl.data(), q.data(), q1.data(), q2.data());
      if (rc != 0) return InternalError(tpamd_error_string(rc));
      for (size_t i = 0; i < B; i++) {
        double nrm2 = 0, dot = 0;
        for (size_t d = 0; d < D; d++) {
          nrm2 += q1[i * D + d] * q1[i * D + d];
          dot += paths_[g.ids[i]]->GetInitialVelocity()[d] * q1[i * D + d];
        }
        if (nrm2 > 100 * std::numeric_limits<double>::epsilon()) g.sd0[i] = std::max(dot / nrm2, 0.0);
      }
    }
    g.time.resize(B * N); g.s.resize(B * N); g.sd.resize(B * N); g.sdd.resize(B * N);
    g.q.resize(B * N * D); g.qd.resize(B * N * D); g.qdd.resize(B * N * D);
    g.status.assign(B, -1); g.lei.assign(B, 0);
    if (check_solutions_ || refined) g.sd2.resize(B * N);
  }
  // all groups of this device in ONE call: they run side by side on the engine's lanes
  std::vector<tpamd_joint_batch> batches;
  std::vector<tpamd_joint_inputs> ins;
  std::vector<tpamd_path_outputs> outs;
  for (GroupArrays &g : groups) {
    batches.push_back(tpamd_joint_batch{(int)g.B, (int)g.D, (int)g.N, (int)g.P, 0, 0, g.safety});
    ins.push_back(tpamd_joint_inputs{g.knots.data(), g.cps.data(), g.vmax.data(), g.amax.data(), g.ps.data(),
                                     g.dl.data(), g.sd0.data(), g.sdd0.data(), g.t0.data(),
                                     g.ragged ? g.ns.data() : nullptr});
    outs.push_back(tpamd_path_outputs{g.time.data(), g.s.data(), g.sd.data(), g.sdd.data(), g.q.data(),
                                      g.qd.data(), g.qdd.data(), g.lei.data(), nullptr, g.status.data(),
                                      g.sd2.empty() ? nullptr : g.sd2.data()});
  }
  if (refined) {
    // one group at a time through the refined entry: solve, check, re-time the violators
    for (size_t k = 0; k < groups.size(); k++) {
      const GroupArrays &g = groups[k];
      RefinedGroup rg(g.B, g.N, g.D, refine_);
      const tpamd_refine_options opt = rg.options();
      const tpamd_refine_outputs ref = rg.outputs();
      const int rc = tpamd_time_joint_paths_refined_host(engine, &batches[k], &ins[k], &outs[k], &opt, &ref);
      if (rc != 0) return InternalError(tpamd_error_string(rc));
      for (size_t i = 0; i < g.B; i++) (*refined)[g.ids[i]] = rg.Solution(i, (size_t)g.ns[i], outs[k]);
    }
    return OkStatus();
  }
  {
    const int rc = tpamd_time_joint_groups_host(engine, (int)groups.size(), batches.data(), ins.data(), outs.data());
    if (rc != 0) return InternalError(tpamd_error_string(rc));
  }
  if (check_solutions_)
    for (size_t k = 0; k < groups.size(); k++) {
      const GroupArrays &g = groups[k];
      const tpamd_solution sol{g.sd2.data(), nullptr, g.sdd.data(), g.status.data()};
      CheckRecords rec(g.B);
      const tpamd_check_outputs cko = rec.outputs();
      const int rc = tpamd_check_joint_paths_host(engine, &batches[k], &ins[k], nullptr, &sol, &cko);
      if (rc != 0) return InternalError(tpamd_error_string(rc));
      rec.scatter(g.ids, r);
    }
  for (const GroupArrays &g : groups) {     // padded group layout -> packed result
    const size_t N = g.N, D = g.D;
    for (size_t i = 0; i < g.B; i++) {
      const size_t b = g.ids[i], n = (size_t)g.ns[i];
      r->status[b] = g.status[i]; r->last_extremal_index[b] = g.lei[i];
      if (g.status[i] != 0) continue;
      std::copy_n(g.time.begin() + i * N, n, r->time.begin() + r->sample_offset[b]);
      std::copy_n(g.s.begin() + i * N, n, r->s.begin() + r->sample_offset[b]);
      std::copy_n(g.sd.begin() + i * N, n, r->sd.begin() + r->sample_offset[b]);
      std::copy_n(g.sdd.begin() + i * N, n, r->sdd.begin() + r->sample_offset[b]);
      std::copy_n(g.q.begin() + i * N * D, n * D, r->q.begin() + r->joint_offset[b]);
      std::copy_n(g.qd.begin() + i * N * D, n * D, r->qd.begin() + r->joint_offset[b]);
      std::copy_n(g.qdd.begin() + i * N * D, n * D, r->qdd.begin() + r->joint_offset[b]);
    }
  }
  return OkStatus();
}

}  // namespace trajectory_planning

#include "batch_cartesian_timing.h"

#include <algorithm>
#include <thread>

#include "engine_handle.h"

namespace trajectory_planning {

using ::tpamd::compat::InternalError;
using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::OkStatus;

Status BatchCartesianTiming::SetPaths(std::vector<CartesianPathSamples> paths) {
  if (paths.empty()) return InvalidArgumentError("no paths");
  for (const auto &p : paths) {
    if (p.ik_positions.size() < 3) return InvalidArgumentError("a path needs at least 3 samples");
    const size_t D = p.ik_positions[0].size();
    if (D == 0 || p.max_joint_velocity.size() != D || p.max_joint_acceleration.size() != D)
      return InvalidArgumentError("limits must have one entry per joint");
    for (const auto &q : p.ik_positions)
      if (q.size() != D) return InvalidArgumentError("IK positions of one path must share a size");
    if (!p.jacobian) return InvalidArgumentError("missing Jacobian callback");
    if (!(p.delta_parameter > 0.0)) return InvalidArgumentError("delta_parameter must be positive");
  }
  paths_ = std::move(paths);
  return OkStatus();
}

Status BatchCartesianTiming::SetDevices(const std::vector<int> &devices) {
  const int visible = ::tpamd::device_count();
  for (size_t i = 0; i < devices.size(); i++) {
    if (devices[i] < 0 || devices[i] >= visible) return InvalidArgumentError("no such device");
    for (size_t j = 0; j < i; j++)
      if (devices[j] == devices[i]) return InvalidArgumentError("device listed twice");
  }
  devices_ = devices;
  return OkStatus();
}

Status BatchCartesianTiming::ComputeTimingProfiles(double time_start_sec, BatchTimingResult *r) {
  if (paths_.empty()) return InvalidArgumentError("SetPaths first");
  const size_t Bt = paths_.size();
  r->status.assign(Bt, -1); r->last_extremal_index.assign(Bt, 0);
  r->samples_per_path.resize(Bt); r->dofs_per_path.resize(Bt);
  r->sample_offset.assign(Bt + 1, 0); r->joint_offset.assign(Bt + 1, 0);
  r->num_samples = 0; r->num_dofs = 0;
  std::vector<double> cost(Bt);
  for (size_t b = 0; b < Bt; b++) {
    const size_t n = paths_[b].ik_positions.size(), d = paths_[b].ik_positions[0].size();
    r->samples_per_path[b] = (int32_t)n; r->dofs_per_path[b] = (int32_t)d;
    r->sample_offset[b + 1] = r->sample_offset[b] + n;
    r->joint_offset[b + 1] = r->joint_offset[b] + n * d;
    r->num_samples = std::max(r->num_samples, (int)n);
    r->num_dofs = std::max(r->num_dofs, (int)d);
    cost[b] = (double)n * (2.0 * d + 2.0) * (2.0 * d + 2.0);
  }
  r->time.resize(r->sample_offset[Bt]); r->s.resize(r->sample_offset[Bt]);
  r->sd.resize(r->sample_offset[Bt]); r->sdd.resize(r->sample_offset[Bt]);
  r->q.resize(r->joint_offset[Bt]); r->qd.resize(r->joint_offset[Bt]); r->qdd.resize(r->joint_offset[Bt]);
  PrepareCheckResult(check_solutions_, Bt, r);
  const std::vector<int> devices = devices_.empty() ? std::vector<int>{::tpamd::default_device()} : devices_;
  const int nd = (int)devices.size();
  std::vector<int32_t> begin(nd + 1);
  tpamd_shard_bounds_balanced((int)Bt, cost.data(), nd, begin.data());
  std::vector<Status> st(nd, OkStatus());
  std::vector<int> calls(nd, 0);
  std::vector<std::thread> threads;
  for (int k = 1; k < nd; k++)
    threads.emplace_back(
        [&, k] { st[k] = ComputeBlock(devices[k], begin[k], begin[k + 1], time_start_sec, r, &calls[k]); });
  st[0] = ComputeBlock(devices[0], begin[0], begin[1], time_start_sec, r, &calls[0]);
  for (auto &t : threads) t.join();
  engine_calls_ = 0;
  for (int c : calls) engine_calls_ += c;
  for (const Status &s : st)
    if (!s.ok()) return s;
  return OkStatus();
}

Status BatchCartesianTiming::ComputeBlock(int device, size_t lo, size_t hi, double time_start_sec,
                                          BatchTimingResult *r, int *engine_calls) const {
  *engine_calls = 0;
  if (hi <= lo) return OkStatus();
  ::tpamd::EngineLease lease = ::tpamd::acquire_engine(device);
  tpamd_engine *engine = lease.get();
  if (!engine) return InternalError("no GPU engine");
  std::vector<size_t> dofs(paths_.size()), samples(paths_.size());
  std::vector<double> safety(paths_.size());
  for (size_t b = lo; b < hi; b++) {
    dofs[b] = paths_[b].ik_positions[0].size();
    samples[b] = paths_[b].ik_positions.size();
    safety[b] = paths_[b].constraint_safety;
  }

  for (const std::vector<size_t> &ids : CartesianTimingBuckets(dofs, samples, safety, lo, hi)) {
    // one ragged call: the rows of the bucket's paths packed path after path, outputs of the
    // stride of its longest path
    const size_t B = ids.size(), D = dofs[ids[0]];
    size_t N = 0, rows = 0;
    std::vector<int32_t> count(B), first(B);
    for (size_t g = 0; g < B; g++) {
      count[g] = (int32_t)samples[ids[g]];
      first[g] = (int32_t)rows;
      rows += samples[ids[g]];
      N = std::max(N, samples[ids[g]]);
    }
    if (rows >= ((size_t)1 << 31)) return InvalidArgumentError("too many samples in one bucket");
    std::vector<double> q(rows * D), J(rows * 6 * D), vmax(B * D), amax(B * D), vt(B), vr(B), ps(B),
        dl(B), sd0(B), sdd0(B, 0.0), t0(B, time_start_sec);
    for (size_t g = 0; g < B; g++) {
      const CartesianPathSamples &p = paths_[ids[g]];
      for (size_t i = 0; i < (size_t)count[g]; i++) {
        const size_t row = (size_t)first[g] + i;
        std::copy(p.ik_positions[i].begin(), p.ik_positions[i].end(), q.begin() + row * D);
        // the user's callback, once per sample, as ConstraintSetup does (:576)
        const Status st = p.jacobian(p.ik_positions[i], &J[row * 6 * D]);
        if (!st.ok()) return st;
      }
      for (size_t d = 0; d < D; d++) {
        vmax[g * D + d] = p.max_joint_velocity[d];
        amax[g * D + d] = p.max_joint_acceleration[d];
      }
      vt[g] = p.max_translational_velocity; vr[g] = p.max_rotational_velocity;
      ps[g] = p.path_start; dl[g] = p.delta_parameter; sd0[g] = p.start_velocity;
    }
    std::vector<double> time(B * N), s(B * N), sd(B * N), sdd(B * N), qd(B * N * D), qdd(B * N * D);
    std::vector<int32_t> status(B, -1), lei(B, 0);
    std::vector<double> sd2(check_solutions_ ? B * N : 0);
    tpamd_cartesian_batch batch{(int)B, (int)D, (int)N, 0, safety[ids[0]]};
    tpamd_cartesian_inputs in{q.data(), J.data(), vmax.data(), amax.data(), vt.data(), vr.data(),
                              ps.data(), dl.data(), sd0.data(), sdd0.data(), t0.data()};
    tpamd_path_outputs out{time.data(), s.data(), sd.data(), sdd.data(), nullptr, qd.data(), qdd.data(),
                           lei.data(), nullptr, status.data(), check_solutions_ ? sd2.data() : nullptr};
    {
      const int rc = tpamd_time_cartesian_paths_ragged_host(engine, &batch, &in, count.data(), first.data(),
                                                            (int64_t)rows, &out);
      ++*engine_calls;
      if (rc != 0) return InternalError(tpamd_error_string(rc));
    }
    if (check_solutions_) {
      const tpamd_solution sol{sd2.data(), nullptr, sdd.data(), status.data()};
      CheckRecords rec(B);
      const tpamd_check_outputs cko = rec.outputs();
      const int rc = tpamd_check_cartesian_paths_host(engine, &batch, &in, count.data(), first.data(), (int64_t)rows,
                                                      &sol, &cko);
      if (rc != 0) return InternalError(tpamd_error_string(rc));
      rec.scatter(ids, r);
    }
    for (size_t g = 0; g < B; g++) {
      const size_t b = ids[g], n = (size_t)count[g];
      r->status[b] = status[g]; r->last_extremal_index[b] = lei[g];
      std::copy_n(q.begin() + (size_t)first[g] * D, n * D, r->q.begin() + r->joint_offset[b]);
      if (status[g] != 0) continue;
      std::copy_n(time.begin() + g * N, n, r->time.begin() + r->sample_offset[b]);
      std::copy_n(s.begin() + g * N, n, r->s.begin() + r->sample_offset[b]);
      std::copy_n(sd.begin() + g * N, n, r->sd.begin() + r->sample_offset[b]);
      std::copy_n(sdd.begin() + g * N, n, r->sdd.begin() + r->sample_offset[b]);
      std::copy_n(qd.begin() + g * N * D, n * D, r->qd.begin() + r->joint_offset[b]);
      std::copy_n(qdd.begin() + g * N * D, n * D, r->qdd.begin() + r->joint_offset[b]);
    }
  }
  return OkStatus();
}

}  // namespace trajectory_planning

#include "batch_waypoint_timing.h"

#include <algorithm>
#include <map>
#include <utility>

#include "engine_handle.h"

namespace trajectory_planning {

using ::tpamd::compat::InternalError;
using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::OkStatus;

Status BatchWaypointTiming::AddPath(const std::vector<VectorXd> &waypoints, const JointPathOptions &options,
                                    Span<const double> max_velocity, Span<const double> max_acceleration) {
  const size_t D = options.num_dofs(), N = options.num_path_samples();
  if (D < 1 || D > 16) return InvalidArgumentError("num_dofs must be 1..16");
  if (N < 3 || N > 8192) return InvalidArgumentError("num_path_samples must be 3..8192");
  if (max_velocity.size() != D || max_acceleration.size() != D)
    return InvalidArgumentError("a limit of the wrong dimension");
  for (const VectorXd &w : waypoints)
    if ((size_t)w.size() != D) return InvalidArgumentError("a waypoint of the wrong dimension");
  Path p;
  p.W = waypoints.size(); p.D = D; p.N = N;
  p.rounding = options.rounding(); p.safety = options.constraint_safety(); p.delta = options.delta_parameter();
  for (const VectorXd &w : waypoints) p.waypoints.insert(p.waypoints.end(), w.begin(), w.end());
  p.vmax.assign(max_velocity.begin(), max_velocity.end());
  p.amax.assign(max_acceleration.begin(), max_acceleration.end());
  paths_.push_back(std::move(p));
  return OkStatus();
}

void BatchWaypointTiming::Clear() { paths_.clear(); }

Status BatchWaypointTiming::ComputeTimingProfiles(double time_start_sec, BatchTimingResult *r) {
  if (paths_.empty()) return InvalidArgumentError("AddPath first");
  const size_t Bt = paths_.size();
  r->status.assign(Bt, -1); r->last_extremal_index.assign(Bt, 0);
  r->samples_per_path.resize(Bt); r->dofs_per_path.resize(Bt);
  r->sample_offset.assign(Bt + 1, 0); r->joint_offset.assign(Bt + 1, 0);
  r->num_samples = 0; r->num_dofs = 0;
  for (size_t b = 0; b < Bt; b++) {
    const size_t n = paths_[b].N, d = paths_[b].D;
    r->samples_per_path[b] = (int32_t)n; r->dofs_per_path[b] = (int32_t)d;
    r->sample_offset[b + 1] = r->sample_offset[b] + n;
    r->joint_offset[b + 1] = r->joint_offset[b] + n * d;
    r->num_samples = std::max(r->num_samples, (int)n);
    r->num_dofs = std::max(r->num_dofs, (int)d);
  }
  r->time.resize(r->sample_offset[Bt]); r->s.resize(r->sample_offset[Bt]);
  r->sd.resize(r->sample_offset[Bt]); r->sdd.resize(r->sample_offset[Bt]);
  r->q.resize(r->joint_offset[Bt]); r->qd.resize(r->joint_offset[Bt]); r->qdd.resize(r->joint_offset[Bt]);
  PrepareCheckResult(check_solutions_, Bt, r);
  num_points_.assign(Bt, 0); path_end_.assign(Bt, 0.0); delta_used_.assign(Bt, 0.0);
  engine_calls_ = 0;
  std::vector<PathSolution> refined(refine_.enabled ? Bt : 0);

  ::tpamd::EngineLease lease = ::tpamd::acquire_engine(::tpamd::default_device());
  tpamd_engine *engine = lease.get();
  if (!engine) return InternalError("no GPU engine");
  // the kernels are specialised on the joint count and a call has one constraint safety: nothing else
  // separates paths (not the waypoint count, not the sample count)
  std::map<std::pair<size_t, double>, std::vector<size_t>> groups;
  for (size_t b = 0; b < Bt; b++) groups[{paths_[b].D, paths_[b].safety}].push_back(b);
  for (const auto &kv : groups) {
    const std::vector<size_t> &ids = kv.second;
    const size_t B = ids.size(), D = kv.first.first;
    size_t N = 0;
    bool ragged = false;
    for (size_t b : ids) {
      ragged = ragged || (N != 0 && paths_[b].N != N);
      N = std::max(N, paths_[b].N);
    }
    std::vector<int32_t> offsets(B + 1, 0), ns(B), status(B, -1), lei(B, 0), np(B, 0);
    std::vector<double> wps, rounding(B), vmax(B * D), amax(B * D), delta(B), t0(B, time_start_sec), end(B), used(B);
    for (size_t i = 0; i < B; i++) {
      const Path &p = paths_[ids[i]];
      offsets[i + 1] = offsets[i] + (int32_t)p.W;
      wps.insert(wps.end(), p.waypoints.begin(), p.waypoints.end());
      rounding[i] = p.rounding; delta[i] = p.delta; ns[i] = (int32_t)p.N;
      std::copy(p.vmax.begin(), p.vmax.end(), vmax.begin() + i * D);
      std::copy(p.amax.begin(), p.amax.end(), amax.begin() + i * D);
    }
    std::vector<double> time(B * N), s(B * N), sd(B * N), sdd(B * N), q(B * N * D), qd(B * N * D), qdd(B * N * D);
    // CheckSolutions: the fitted splines in their slots of S control points, and sd2
    size_t S = 4;
    for (size_t b : ids) S = std::max(S, paths_[b].W <= 1 ? (size_t)4 : 3 * paths_[b].W - 2);
    std::vector<double> sd2(check_solutions_ || refine_.enabled ? B * N : 0), knots(check_solutions_ ? B * (S + 3) : 0),
        cps(check_solutions_ ? B * S * D : 0);
    const tpamd_waypoint_batch bt{(int32_t)B, (int32_t)D, (int32_t)N, 0, kv.first.second};
    const tpamd_waypoint_inputs in{offsets.data(), wps.data(), rounding.data(), vmax.data(), amax.data(),
                                   ragged ? ns.data() : nullptr, cover_whole_path_ ? nullptr : delta.data(),
                                   nullptr, t0.data()};
    const tpamd_path_outputs out{time.data(), s.data(), sd.data(), sdd.data(), q.data(), qd.data(), qdd.data(),
                                 lei.data(), nullptr, status.data(), sd2.empty() ? nullptr : sd2.data()};
    const tpamd_waypoint_fit_outputs fit{np.data(), end.data(), used.data(), check_solutions_ ? knots.data() : nullptr,
                                         check_solutions_ ? cps.data() : nullptr};
    if (refine_.enabled) {
      // the refined entry: solve, check, re-time the violators; the result is packed after all groups
      RefinedGroup rg(B, N, D, refine_);
      const tpamd_refine_options opt = rg.options();
      const tpamd_refine_outputs ref = rg.outputs();
      const int rrc = tpamd_time_waypoint_paths_refined_host(engine, &bt, &in, &out, &fit, &opt, &ref);
      engine_calls_++;
      if (rrc != 0) return InternalError(tpamd_error_string(rrc));
      for (size_t i = 0; i < B; i++) {
        num_points_[ids[i]] = np[i]; path_end_[ids[i]] = end[i]; delta_used_[ids[i]] = used[i];
        refined[ids[i]] = rg.Solution(i, (size_t)ns[i], out, status[i] != TPAMD_PATH_NO_WAYPOINTS);
      }
      continue;
    }
    const int rc = tpamd_time_waypoint_paths_host(engine, &bt, &in, &out, &fit);
    engine_calls_++;
    if (rc != 0) return InternalError(tpamd_error_string(rc));
    if (check_solutions_) {
      const std::vector<double> zero(B, 0.0);
      const tpamd_joint_batch jb{(int32_t)B, (int32_t)D, (int32_t)N, (int32_t)S, 0, 0, kv.first.second};
      const tpamd_joint_inputs ji{knots.data(), cps.data(), vmax.data(), amax.data(), zero.data(), used.data(),
                                  nullptr, nullptr, nullptr, ragged ? ns.data() : nullptr};
      const tpamd_solution sol{sd2.data(), nullptr, sdd.data(), status.data()};
      CheckRecords rec(B);
      const tpamd_check_outputs cko = rec.outputs();
      const int crc = tpamd_check_joint_paths_host(engine, &jb, &ji, np.data(), &sol, &cko);
      if (crc != 0) return InternalError(tpamd_error_string(crc));
      rec.scatter(ids, r);
    }
    for (size_t i = 0; i < B; i++) {     // padded group layout -> packed result
      const size_t b = ids[i], n = (size_t)ns[i];
      r->status[b] = status[i];
      num_points_[b] = np[i]; path_end_[b] = end[i]; delta_used_[b] = used[i];
      if (status[i] == TPAMD_PATH_NO_WAYPOINTS) continue;
      r->last_extremal_index[b] = lei[i];
      if (status[i] != 0) continue;
      std::copy_n(time.begin() + i * N, n, r->time.begin() + r->sample_offset[b]);
      std::copy_n(s.begin() + i * N, n, r->s.begin() + r->sample_offset[b]);
      std::copy_n(sd.begin() + i * N, n, r->sd.begin() + r->sample_offset[b]);
      std::copy_n(sdd.begin() + i * N, n, r->sdd.begin() + r->sample_offset[b]);
      std::copy_n(q.begin() + i * N * D, n * D, r->q.begin() + r->joint_offset[b]);
      std::copy_n(qd.begin() + i * N * D, n * D, r->qd.begin() + r->joint_offset[b]);
      std::copy_n(qdd.begin() + i * N * D, n * D, r->qdd.begin() + r->joint_offset[b]);
    }
  }
  if (refine_.enabled) PackRefinedResult(refined, r);
  return OkStatus();
}

}  // namespace trajectory_planning

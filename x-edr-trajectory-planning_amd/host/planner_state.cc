#include "planner_state.h"

#include <cstring>
#include <memory>

#include "../csrc/tpamd_state.h"
#include "timeable_path_joint_spline.h"

namespace trajectory_planning {

using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::OkStatus;
using ::tpamd::compat::UnimplementedError;
using namespace ::tpamd;   // the record: StateRecordHeader, StatePlannerView, kSec*

namespace {

uint64_t Bits(double x) {
  uint64_t u;
  std::memcpy(&u, &x, 8);
  return u;
}
double FromBits(uint64_t u) {
  double x;
  std::memcpy(&x, &u, 8);
  return x;
}
const uint64_t *Words(const std::vector<double> &v) { return v.empty() ? nullptr : (const uint64_t *)v.data(); }
std::vector<double> Flat(const std::vector<VectorXd> &rows) {
  std::vector<double> r;
  for (const VectorXd &x : rows) r.insert(r.end(), x.begin(), x.end());
  return r;
}
std::vector<double> Vec(const VectorXd &x) { return std::vector<double>(x.begin(), x.end()); }
void Take(const StatePlannerView &v, int section, size_t count, std::vector<double> *out) {
  out->resize(count);
  if (count) std::memcpy(out->data(), v.sec[section], count * 8);
}
void TakeRows(const StatePlannerView &v, int section, size_t rows, size_t D, std::vector<VectorXd> *out) {
  out->assign(rows, VectorXd(D));
  const double *src = (const double *)v.sec[section];
  for (size_t i = 0; i < rows; i++)
    for (size_t d = 0; d < D; d++) (*out)[i][d] = src[i * D + d];
}

SetShape ShapeOf(const PathTimingTrajectoryOptions &o, double constraint_safety) {
  SetShape s{};
  s.kind = kStateJoint;
  s.num_dofs = (int32_t)o.GetNumDofs();
  s.num_samples = (int32_t)o.GetNumPathSamples();
  s.sampling_method = o.GetTimeSamplingMethod() == PathTimingTrajectoryOptions::TimeSamplingMethod::kUniformlyInTime ? 0 : 1;
  s.time_step_ns = o.GetTimeStep().nanos();
  s.constraint_safety_bits = Bits(constraint_safety);
  s.max_initial_velocity_error_bits = Bits(o.GetMaxInitialVelocityError());
  return s;
}

}  // namespace

Status PlannerStateFromHost(const PathTimingTrajectory &p, std::vector<unsigned char> *record, double constraint_safety) {
  if (!record) return InvalidArgumentError("no record");
  const TimeableJointSplinePath *path = nullptr;
  if (p.path_ != nullptr) {
    path = dynamic_cast<const TimeableJointSplinePath *>(p.path_.get());
    if (!path) return UnimplementedError("only a TimeableJointSplinePath planner has a state record");
  }
  const bool has = path && path->path_state_ != TimeablePath::State::kNoPath && path->control_points_.size() >= 3;
  StatePlannerView v{};
  StateRecordHeader &h = v.head;
  h.shape = ShapeOf(p.options_, has ? path->options_.constraint_safety() : constraint_safety);
  const size_t N = p.options_.GetNumPathSamples();
  h.num_points = has ? (int32_t)path->control_points_.size() : 0;
  h.history_count = (int32_t)p.time_at_path_samples_.size();
  h.trajectory_count = (int32_t)p.time_.size();
  h.table_rows = h.first_row = 0;
  h.has_path = has;
  h.path_state = has ? (int32_t)path->path_state_ : 0;
  h.initial_plan = p.initial_plan_;
  h.planned_to_end = p.planned_to_end_;
  h.target_reached = p.target_reached_;
  h.w_lei = p.initial_plan_ ? p.profile_.GetLastExtremalIndex() : 0;
  h.path_horizon = Bits(p.path_horizon_);
  h.path_start = Bits(p.path_start_);
  h.path_start_velocity = Bits(p.path_start_velocity_);
  h.path_time_start = Bits(p.path_time_start_);
  h.start_time_ns = ::tpamd::compat::ToUnixNanos(p.start_time_);
  h.end_time_ns = ::tpamd::compat::ToUnixNanos(p.end_time_);
  h.final_decel_start_ns = ::tpamd::compat::ToUnixNanos(p.final_decel_start_);
  h.delta = has ? Bits(path->options_.delta_parameter()) : 0;
  h.path_end = h.vtrans = h.vrot = 0;
  std::vector<double> vmax, amax, iv, w_time, q, qd, qdd;
  if (has) {
    vmax = Vec(path->max_joint_velocity_);
    amax = Vec(path->max_joint_acceleration_);
    iv = Vec(path->initial_velocity_);
    v.sec[kSecKnots] = Words(path->knots_);
    v.sec[kSecCp] = Words(path->packed_control_points_);
    v.sec[kSecVmax] = Words(vmax);
    v.sec[kSecAmax] = Words(amax);
    v.sec[kSecIv] = Words(iv);
  }
  v.sec[kSecHTime] = Words(p.time_at_path_samples_);
  v.sec[kSecHS] = Words(p.path_parameter_at_path_samples_);
  v.sec[kSecHSd] = Words(p.path_velocity_at_path_samples_);
  v.sec[kSecHSdd] = Words(p.path_acceleration_at_path_samples_);
  v.sec[kSecHQ] = Words(p.position_at_path_samples_);
  v.sec[kSecHQd] = Words(p.velocity_at_path_samples_);
  v.sec[kSecHQdd] = Words(p.acceleration_at_path_samples_);
  if (p.initial_plan_) {
    const auto &t = p.profile_.GetTimeSamples();
    if ((size_t)t.size() != N) return InvalidArgumentError("the planner's profile does not hold a window");
    w_time.assign(t.data(), t.data() + N);
    v.sec[kSecWTime] = Words(w_time);
  }
  q = Flat(p.positions_);
  qd = Flat(p.velocities_);
  qdd = Flat(p.accelerations_);
  v.sec[kSecTTime] = Words(p.time_);
  v.sec[kSecTS] = Words(p.path_parameter_);
  v.sec[kSecTSd] = Words(p.path_parameter_derivative_);
  v.sec[kSecTSdd] = Words(p.second_path_parameter_derivative_);
  v.sec[kSecTQ] = Words(q);
  v.sec[kSecTQd] = Words(qd);
  v.sec[kSecTQdd] = Words(qdd);
  const uint64_t bytes = state_record_encode(v, nullptr, 0);
  record->assign((size_t)bytes, 0);
  state_record_encode(v, record->data(), record->size());
  return OkStatus();
}

Status PlannerStateToHost(const void *record, size_t len, PathTimingTrajectory *p) {
  if (!p) return InvalidArgumentError("no planner");
  if (!record || len < sizeof(StateRecordHeader)) return InvalidArgumentError("not a planner state record");
  TimeableJointSplinePath *held = p->path_ ? dynamic_cast<TimeableJointSplinePath *>(p->path_.get()) : nullptr;
  if (p->path_ && !held) return UnimplementedError("only a TimeableJointSplinePath planner takes a state record");
  // 8-byte aligned copy: the sections are read as words
  std::vector<uint64_t> copy((len + 7) / 8);
  std::memcpy(copy.data(), record, len);
  const StateRecordHeader head = state_record_header(copy.data());
  const double safety = held ? held->options_.constraint_safety() : FromBits(head.shape.constraint_safety_bits);
  if (state_record_validate(copy.data(), len, ShapeOf(p->options_, safety)) != kStateOk)
    return InvalidArgumentError("not a planner state record for this planner");
  const StatePlannerView v = state_record_decode(copy.data());
  const StateRecordHeader &h = v.head;
  const size_t D = p->options_.GetNumDofs(), N = p->options_.GetNumPathSamples();
  const size_t P = (size_t)h.num_points, hc = (size_t)h.history_count, tc = (size_t)h.trajectory_count;
  if (h.has_path) {
    const double delta = FromBits(h.delta);
    std::shared_ptr<TimeableJointSplinePath> path;
    if (held && Bits(held->options_.delta_parameter()) == h.delta && held->options_.num_dofs() == D &&
        held->options_.num_path_samples() == N) {
      path = std::static_pointer_cast<TimeableJointSplinePath>(p->path_);
    } else {
      path = std::make_shared<TimeableJointSplinePath>(JointPathOptions()
                                                           .set_num_dofs(D)
                                                           .set_num_path_samples(N)
                                                           .set_delta_parameter(delta)
                                                           .set_constraint_safety(safety)
                                                           .set_rounding(held ? held->options_.rounding() : 0.2));
    }
    path->waypoints_.clear();
    Take(v, kSecKnots, P + 3, &path->knots_);
    Take(v, kSecCp, P * D, &path->packed_control_points_);
    TakeRows(v, kSecCp, P, D, &path->control_points_);
    for (size_t d = 0; d < D; d++) {
      path->max_joint_velocity_[d] = FromBits(v.sec[kSecVmax][d]);
      path->max_joint_acceleration_[d] = FromBits(v.sec[kSecAmax][d]);
      path->initial_velocity_[d] = FromBits(v.sec[kSecIv][d]);
    }
    path->path_state_ = (TimeablePath::State)h.path_state;
    if (path->path_state_ == TimeablePath::State::kPathWasSampled) {     // as AdoptSamples leaves them
      path->parameter_start_ = FromBits(h.path_start);
      path->parameter_end_ = N * delta;
    }
    p->path_ = path;
  } else {
    p->path_ = nullptr;
  }
  p->initial_plan_ = h.initial_plan != 0;
  p->planned_to_end_ = h.planned_to_end != 0;
  p->target_reached_ = h.target_reached != 0;
  p->path_horizon_ = FromBits(h.path_horizon);
  p->path_start_ = FromBits(h.path_start);
  p->path_start_velocity_ = FromBits(h.path_start_velocity);
  p->path_start_acceleration_ = 0.0;
  p->path_time_start_ = FromBits(h.path_time_start);
  p->start_time_ = ::tpamd::compat::FromUnixNanos(h.start_time_ns);
  p->end_time_ = ::tpamd::compat::FromUnixNanos(h.end_time_ns);
  p->final_decel_start_ = ::tpamd::compat::FromUnixNanos(h.final_decel_start_ns);
  Take(v, kSecHTime, hc, &p->time_at_path_samples_);
  Take(v, kSecHS, hc, &p->path_parameter_at_path_samples_);
  Take(v, kSecHSd, hc, &p->path_velocity_at_path_samples_);
  Take(v, kSecHSdd, hc, &p->path_acceleration_at_path_samples_);
  Take(v, kSecHQ, hc * D, &p->position_at_path_samples_);
  Take(v, kSecHQd, hc * D, &p->velocity_at_path_samples_);
  Take(v, kSecHQdd, hc * D, &p->acceleration_at_path_samples_);
  if (h.initial_plan) {
    std::vector<double> w_time, zero(N, 0.0);
    Take(v, kSecWTime, N, &w_time);
    p->profile_.AdoptSolution((int)N, (int)(2 * D), p->path_start_, p->path_horizon_, w_time.data(), zero.data(),
                              zero.data(), zero.data(), zero.data(), h.w_lei, 0.0);
  }
  Take(v, kSecTTime, tc, &p->time_);
  Take(v, kSecTS, tc, &p->path_parameter_);
  Take(v, kSecTSd, tc, &p->path_parameter_derivative_);
  Take(v, kSecTSdd, tc, &p->second_path_parameter_derivative_);
  TakeRows(v, kSecTQ, tc, D, &p->positions_);
  TakeRows(v, kSecTQd, tc, D, &p->velocities_);
  TakeRows(v, kSecTQdd, tc, D, &p->accelerations_);
  p->check_record_ = EmptyPlannerCheck();
  return OkStatus();
}

}  // namespace trajectory_planning

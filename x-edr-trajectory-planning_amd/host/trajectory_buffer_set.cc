// TrajectoryBufferSet: the batched TrajectoryBuffer methods on the C-ABI's buffer set.
#include "trajectory_buffer_set.h"

#include <limits>

namespace trajectory_planning {

using ::tpamd::compat::FailedPreconditionError;
using ::tpamd::compat::InternalError;
using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::NotFoundError;
using ::tpamd::compat::OkStatus;
using ::tpamd::compat::OutOfRangeError;

namespace {

Status FromCode(int code) {
  switch (code) {
    case TPAMD_PLAN_OK: return OkStatus();
    case TPAMD_PLAN_FAILED_PRECONDITION: return FailedPreconditionError("No samples.");
    case TPAMD_PLAN_OUT_OF_RANGE: return OutOfRangeError("time or index outside the samples");
    case TPAMD_PLAN_INVALID_ARGUMENT: return InvalidArgumentError("invalid arguments or samples");
    case TPAMD_PLAN_NOT_FOUND: return NotFoundError("No safe stopping trajectory found (likely not enough time).");
    default: return InternalError("buffer operation failed (" + std::to_string(code) + ")");
  }
}
std::vector<Status> FromCodes(const std::vector<int32_t> &st) {
  std::vector<Status> out;
  for (int32_t c : st) out.push_back(FromCode(c));
  return out;
}
Status Call(int rc) { return rc == 0 ? OkStatus() : InternalError(tpamd_error_string(rc)); }

}  // namespace

TrajectoryBufferSet::TrajectoryBufferSet(size_t num_buffers, size_t num_dofs, TrajectoryBufferOptions options,
                                         size_t capacity, int device)
    : num_buffers_(num_buffers), num_dofs_(num_dofs) {
  lease_ = ::tpamd::acquire_engine(device);
  if (!lease_) {
    init_status_ = FailedPreconditionError("no engine: TrajectoryBufferSet needs a GPU");
    return;
  }
  Init(lease_.get(), options, capacity);
}

TrajectoryBufferSet::TrajectoryBufferSet(const PathTimingTrajectorySet &planners, size_t num_buffers, size_t num_dofs,
                                         TrajectoryBufferOptions options, size_t capacity)
    : num_buffers_(num_buffers), num_dofs_(num_dofs), planners_(&planners) {
  if (!planners.status().ok() || !planners.engine()) {
    init_status_ = FailedPreconditionError("the planner set has no engine");
    return;
  }
  Init(planners.engine(), options, capacity);
}

void TrajectoryBufferSet::Init(tpamd_engine *engine, TrajectoryBufferOptions options, size_t capacity) {
  if (!(options.timestep_tolerance > 0)) {   // TrajectoryBuffer::Create
    init_status_ = FailedPreconditionError("timestep_tolerance (" + std::to_string(options.timestep_tolerance) +
                                           ") not positive");
    return;
  }
  const int rc = tpamd_buffer_set_create(engine, (int)num_buffers_, (int)num_dofs_, (int)capacity,
                                         options.timestep_tolerance, &set_);
  if (rc != 0) init_status_ = InternalError(std::string("tpamd_buffer_set_create: ") + tpamd_error_string(rc));
}

TrajectoryBufferSet::~TrajectoryBufferSet() { tpamd_buffer_set_destroy(set_); }

Status TrajectoryBufferSet::Reserve(size_t size) {
  if (!init_status_.ok()) return init_status_;
  return Call(tpamd_buffer_set_reserve(set_, (int)size));
}

size_t TrajectoryBufferSet::DeviceBytes() const { return tpamd_buffer_set_device_bytes(set_); }

Status TrajectoryBufferSet::Ids(const std::vector<size_t> &buffers, std::vector<int32_t> *ids) const {
  if (!init_status_.ok()) return init_status_;
  ids->resize(buffers.size());
  for (size_t k = 0; k < buffers.size(); k++) {
    if (buffers[k] >= num_buffers_) return InvalidArgumentError("no such buffer");
    (*ids)[k] = (int32_t)buffers[k];
  }
  return OkStatus();
}

std::vector<Status> TrajectoryBufferSet::InsertSegments(const std::vector<size_t> &buffers,
                                                        const std::vector<SampledTrajectory> &segments) {
  const size_t n = buffers.size(), D = num_dofs_;
  std::vector<int32_t> ids;
  Status call = Ids(buffers, &ids);
  if (call.ok() && segments.size() != n) call = InvalidArgumentError("one segment per buffer");
  std::vector<int64_t> offsets(n + 1, 0);
  std::vector<double> tm, q, qd, qdd;
  for (size_t k = 0; call.ok() && k < n; k++) {
    const SampledTrajectory &s = segments[k];
    const size_t rows = s.times.size();
    if (s.positions.size() != rows || s.velocities.size() != rows || s.accelerations.size() != rows) {
      call = InvalidArgumentError("positions, velocities, accelerations and times differ in size.");
      break;
    }
    for (size_t i = 0; i < rows; i++) {
      if (s.positions[i].size() != D || s.velocities[i].size() != D || s.accelerations[i].size() != D) {
        call = InvalidArgumentError("a sample has the wrong dimension");
        break;
      }
      tm.push_back(s.times[i]);
      q.insert(q.end(), s.positions[i].begin(), s.positions[i].end());
      qd.insert(qd.end(), s.velocities[i].begin(), s.velocities[i].end());
      qdd.insert(qdd.end(), s.accelerations[i].begin(), s.accelerations[i].end());
    }
    offsets[k + 1] = (int64_t)tm.size();
  }
  std::vector<int32_t> st(n, 0);
  if (call.ok() && n > 0) {
    // non-null arrays for a call whose segments are all empty
    if (tm.empty()) { tm.resize(1); q.resize(D); qd.resize(D); qdd.resize(D); }
    call = Call(tpamd_buffer_set_insert(set_, (int)n, ids.data(), offsets.data(), tm.data(), q.data(), qd.data(),
                                        qdd.data(), st.data()));
  }
  if (!call.ok()) return std::vector<Status>(n, call);
  return FromCodes(st);
}

std::vector<Status> TrajectoryBufferSet::InsertFromPlannerSet(const PathTimingTrajectorySet &set,
                                                              const std::vector<size_t> &buffers,
                                                              const std::vector<size_t> &planners) {
  const size_t n = buffers.size();
  std::vector<int32_t> ids, pids(planners.size());
  Status call = Ids(buffers, &ids);
  if (call.ok() && (&set != planners_ || !set.native_handle()))
    call = InvalidArgumentError("not the planner set this buffer set was made on");
  if (call.ok() && planners.size() != n) call = InvalidArgumentError("one planner per buffer");
  for (size_t k = 0; call.ok() && k < n; k++) {
    if (planners[k] >= set.size()) call = InvalidArgumentError("no such planner");
    pids[k] = (int32_t)planners[k];
  }
  std::vector<int32_t> st(n, 0);
  if (call.ok() && n > 0)
    call = Call(tpamd_buffer_set_insert_from_planner_set(set_, set.native_handle(), (int)n, ids.data(), pids.data(),
                                                         st.data()));
  if (!call.ok()) return std::vector<Status>(n, call);
  return FromCodes(st);
}

std::vector<Status> TrajectoryBufferSet::AppendSamples(const std::vector<size_t> &buffers,
                                                       const std::vector<double> &times,
                                                       const std::vector<VectorXd> &positions,
                                                       const std::vector<VectorXd> &velocities,
                                                       const std::vector<VectorXd> &accelerations) {
  const size_t n = buffers.size(), D = num_dofs_;
  std::vector<int32_t> ids;
  Status call = Ids(buffers, &ids);
  if (call.ok() && (times.size() != n || positions.size() != n || velocities.size() != n || accelerations.size() != n))
    call = InvalidArgumentError("one sample per buffer");
  std::vector<double> q, qd, qdd;
  for (size_t k = 0; call.ok() && k < n; k++) {
    if (positions[k].size() != D || velocities[k].size() != D || accelerations[k].size() != D) {
      call = InvalidArgumentError("a sample has the wrong dimension");
      break;
    }
    q.insert(q.end(), positions[k].begin(), positions[k].end());
    qd.insert(qd.end(), velocities[k].begin(), velocities[k].end());
    qdd.insert(qdd.end(), accelerations[k].begin(), accelerations[k].end());
  }
  std::vector<int32_t> st(n, 0);
  if (call.ok() && n > 0)
    call = Call(tpamd_buffer_set_append_sample(set_, (int)n, ids.data(), times.data(), q.data(), qd.data(), qdd.data(),
                                               st.data()));
  if (!call.ok()) return std::vector<Status>(n, call);
  std::vector<Status> out = FromCodes(st);
  for (Status &s : out)
    if (s.code() == ::tpamd::compat::StatusCode::kInvalidArgument) s = InvalidArgumentError("time must be > times_.back().");
  return out;
}

Status TrajectoryBufferSet::DiscardSegmentsBefore(const std::vector<size_t> &buffers, const std::vector<Time> &time) {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (time.size() != buffers.size()) return InvalidArgumentError("one time per buffer");
  std::vector<int64_t> ns;
  for (Time t : time) ns.push_back(::tpamd::compat::ToUnixNanos(t));
  return Call(tpamd_buffer_set_discard_before(set_, (int)ids.size(), ids.data(), ns.data(), nullptr));
}

Status TrajectoryBufferSet::DiscardSegmentsBefore(const std::vector<size_t> &buffers,
                                                  const std::vector<double> &time_sec) {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (time_sec.size() != buffers.size()) return InvalidArgumentError("one time per buffer");
  return Call(tpamd_buffer_set_discard_before(set_, (int)ids.size(), ids.data(), nullptr, time_sec.data()));
}

std::vector<Status> TrajectoryBufferSet::StopBeforeTimes(const std::vector<size_t> &buffers,
                                                         const std::vector<Time> &time,
                                                         const std::vector<VectorXd> &max_acceleration,
                                                         double time_step) {
  const size_t n = buffers.size(), D = num_dofs_;
  std::vector<int32_t> ids;
  Status call = Ids(buffers, &ids);
  if (call.ok() && (time.size() != n || max_acceleration.size() != n))
    call = InvalidArgumentError("one time and one max_acceleration per buffer");
  std::vector<int64_t> ns;
  std::vector<double> amax;
  for (size_t k = 0; call.ok() && k < n; k++) {
    if (max_acceleration[k].size() != D) {
      call = InvalidArgumentError("max_acceleration has the wrong dimension");
      break;
    }
    ns.push_back(::tpamd::compat::ToUnixNanos(time[k]));
    amax.insert(amax.end(), max_acceleration[k].begin(), max_acceleration[k].end());
  }
  std::vector<int32_t> st(n, 0);
  if (call.ok() && n > 0)
    call = Call(tpamd_buffer_set_stop_before_time(set_, (int)n, ids.data(), ns.data(), nullptr, amax.data(), time_step,
                                                  st.data()));
  if (!call.ok()) return std::vector<Status>(n, call);
  return FromCodes(st);
}

Status TrajectoryBufferSet::GetSetpoints(const std::vector<size_t> &buffers, const std::vector<Time> &start,
                                         Duration step, int ticks, TrajectorySetpoints *out) const {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (!out || start.size() != buffers.size()) return InvalidArgumentError("one start time per buffer");
  if (step.nanos() <= 0 || ticks < 1) return InvalidArgumentError("step and ticks must be positive");
  const size_t n = buffers.size(), D = num_dofs_, T = (size_t)ticks;
  std::vector<int64_t> s;
  for (Time t : start) s.push_back(::tpamd::compat::ToUnixNanos(t));
  const double nan = std::numeric_limits<double>::quiet_NaN();
  out->num_planners = n; out->num_ticks = T; out->num_dofs = D;
  out->positions.assign(n * T * D, nan);
  out->velocities.assign(n * T * D, nan);
  out->accelerations.assign(n * T * D, nan);
  out->status.assign(n * T, OkStatus());
  if (n == 0) return OkStatus();
  std::vector<int32_t> st(n * T);
  const int rc = tpamd_buffer_set_sample_at_ticks(set_, (int)n, ids.data(), s.data(), step.nanos(), ticks,
                                                  out->positions.data(), out->velocities.data(),
                                                  out->accelerations.data(), st.data());
  if (rc != 0) return Call(rc);
  for (size_t i = 0; i < n * T; i++)
    if (st[i] != TPAMD_PLAN_OK)
      out->status[i] = st[i] == TPAMD_PLAN_OUT_OF_RANGE ? OutOfRangeError("Time outside the trajectory") : FromCode(st[i]);
  return OkStatus();
}

Status TrajectoryBufferSet::AddOffsetsToTimestamps(const std::vector<size_t> &buffers,
                                                   const std::vector<Duration> &offset) {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (offset.size() != buffers.size()) return InvalidArgumentError("one offset per buffer");
  std::vector<int64_t> ns;
  for (Duration d : offset) ns.push_back(d.nanos());
  return Call(tpamd_buffer_set_add_offset(set_, (int)ids.size(), ids.data(), ns.data(), nullptr));
}

Status TrajectoryBufferSet::AddOffsetsToTimestamps(const std::vector<size_t> &buffers,
                                                   const std::vector<double> &offset) {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (offset.size() != buffers.size()) return InvalidArgumentError("one offset per buffer");
  return Call(tpamd_buffer_set_add_offset(set_, (int)ids.size(), ids.data(), nullptr, offset.data()));
}

Status TrajectoryBufferSet::Clear(const std::vector<size_t> &buffers) {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  return Call(tpamd_buffer_set_clear(set_, (int)ids.size(), ids.data()));
}

Status TrajectoryBufferSet::GetInfo(const std::vector<size_t> &buffers, const std::vector<Time> &time,
                                    std::vector<TrajectoryBufferInfo> *out) const {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  const size_t n = buffers.size();
  if (!out || (!time.empty() && time.size() != n)) return InvalidArgumentError("one time per buffer, or none");
  std::vector<int64_t> ns, start(n), end(n);
  for (Time t : time) ns.push_back(::tpamd::compat::ToUnixNanos(t));
  std::vector<int32_t> count(n), seq(n), up(n, 0);
  const int rc = tpamd_buffer_set_info(set_, (int)n, ids.data(), time.empty() ? nullptr : ns.data(), count.data(),
                                       seq.data(), start.data(), end.data(), time.empty() ? nullptr : up.data());
  if (rc != 0) return Call(rc);
  out->assign(n, TrajectoryBufferInfo());
  for (size_t k = 0; k < n; k++) {
    TrajectoryBufferInfo &o = (*out)[k];
    o.num_samples = (size_t)count[k];
    o.sequence_number = seq[k];
    o.start_time = ::tpamd::compat::FromUnixNanos(start[k]);
    o.end_time = ::tpamd::compat::FromUnixNanos(end[k]);
    o.positions_up_to_time = (size_t)up[k];
  }
  return OkStatus();
}

Status TrajectoryBufferSet::GetSamples(const std::vector<size_t> &buffers, std::vector<SampledTrajectory> *out) const {
  std::vector<int32_t> ids;
  if (Status s = Ids(buffers, &ids); !s.ok()) return s;
  if (!out) return InvalidArgumentError("no output");
  const size_t n = buffers.size(), D = num_dofs_;
  out->assign(n, SampledTrajectory());
  if (n == 0) return OkStatus();
  // the total is known after a first call without room; the second brings the rows
  std::vector<int64_t> offsets(n + 1, 0);
  std::vector<double> tm(1), q(D), qd(D), qdd(D);
  int rc = tpamd_buffer_set_download(set_, (int)n, ids.data(), offsets.data(), 0, tm.data(), q.data(), qd.data(),
                                     qdd.data());
  if (rc != 0 && (rc != TPAMD_E_INVALID_ARGUMENT || offsets[n] <= 0)) return Call(rc);
  const size_t rows = (size_t)offsets[n];
  if (rows > 0) {
    tm.resize(rows); q.resize(rows * D); qd.resize(rows * D); qdd.resize(rows * D);
    rc = tpamd_buffer_set_download(set_, (int)n, ids.data(), offsets.data(), (int64_t)rows, tm.data(), q.data(),
                                   qd.data(), qdd.data());
    if (rc != 0) return Call(rc);
  }
  for (size_t k = 0; k < n; k++) {
    SampledTrajectory &o = (*out)[k];
    for (size_t i = (size_t)offsets[k]; i < (size_t)offsets[k + 1]; i++) {
      o.times.push_back(tm[i]);
      o.positions.push_back(VectorXd(&q[i * D], D));
      o.velocities.push_back(VectorXd(&qd[i * D], D));
      o.accelerations.push_back(VectorXd(&qdd[i * D], D));
    }
  }
  return OkStatus();
}

}  // namespace trajectory_planning

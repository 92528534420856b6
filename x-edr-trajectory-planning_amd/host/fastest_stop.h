// The fastest stop along a timed path: ComputeFastestStop (path_timing_trajectory.cc:75-172)
// and the index / status logic of PathTimingTrajectory::GetPathStopParameter (:235-287),
// restated as scalar host code. PathTimingTrajectory::GetPathStopParameter runs it on the
// planner's host trajectory; the GPU kernel (csrc/tpamd_stop.h) is bit-identical to it.
// Non-finite inputs are outside the contract.
#ifndef TPAMD_HOST_FASTEST_STOP_H_
#define TPAMD_HOST_FASTEST_STOP_H_

#include <vector>

namespace trajectory_planning {

// append_time / append_rate_squared / append_diff_rate_squared of the reference, one entry per
// sample from the start sample to the stop sample (both included).
struct FastestStopProfile {
  std::vector<double> time, rate_squared, diff_rate_squared;
};

// ComputeFastestStop on `sample_count` >= 1 samples: time[i], the velocity and acceleration rows
// velocities[i][0..num_dofs), accelerations[i][0..num_dofs), and the stop accelerations
// max_acceleration[num_dofs]. Returns the index (relative to sample 0) of the sample at which the
// time scaling reaches rest, or the last one; *total_duration receives the stopping time.
int ComputeFastestStop(int sample_count, int num_dofs, const double *time, const double *const *velocities,
                       const double *const *accelerations, const double *max_acceleration,
                       double *total_duration, FastestStopProfile *profile /* may be null */);

// GetPathStopParameter on one row of flat arrays, as tpamd_fastest_stop_* does: time, s
// [count], qd, qdd [count][num_dofs]. Returns a TPAMD_PLAN_* code: TPAMD_PLAN_INVALID_ARGUMENT
// if no sample is at or after query_time (stop_parameter 0, stop_index -1, duration 0).
int FastestStopAtTime(int count, int num_dofs, const double *time, const double *s, const double *qd,
                      const double *qdd, const double *max_acceleration, double query_time,
                      double *stop_parameter, int *stop_index, double *duration,
                      FastestStopProfile *profile /* may be null */);

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_FASTEST_STOP_H_

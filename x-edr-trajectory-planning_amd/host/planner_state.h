// The planner state record (csrc/tpamd_state.h) of a host PathTimingTrajectory whose path is a
// TimeableJointSplinePath: the bridge between the reference-named planner class and a planner set
// (PathTimingTrajectorySet::AdoptPlanner / ReleasePlanner). This encoder is written from the host
// planner's own members, not from the set's arrays: a record built here equals, byte for byte, the
// record the device exports for a set planner that was given the same calls.
#ifndef TPAMD_HOST_PLANNER_STATE_H_
#define TPAMD_HOST_PLANNER_STATE_H_

#include <vector>

#include "path_timing_trajectory.h"

namespace trajectory_planning {

// The planner's state as one record. A planner without a path gives the record of a planner
// without a path; a path of another kind than TimeableJointSplinePath is refused (Unimplemented).
// constraint_safety: what a planner without a path states in the record's shape (a path states its own).
Status PlannerStateFromHost(const PathTimingTrajectory &planner, std::vector<unsigned char> *record,
                            double constraint_safety = 0.8);

// `planner` takes the state of `record` (len bytes; validated first against the planner's options:
// dofs, path samples, sampling method, time step, initial-velocity tolerance, and the constraint
// safety of the path it holds, if it holds one). It ends as the planner that was encoded would
// continue: path (a TimeableJointSplinePath; the one the planner holds is filled in place if its
// options fit, else a new one is made and GetPath-style accessors of the old object no longer
// refer to this planner), limits, initial velocity, path state, window history, planner scalars and
// trajectory. Not restored, because no record carries them: the waypoints the spline was fitted
// from (GetWaypoints is empty), the path samples of the last window (the next window samples
// again), the profile's arrays other than the time samples and the last extremal index, and the
// check record. Nothing changes if the record is refused (InvalidArgument).
Status PlannerStateToHost(const void *record, size_t len, PathTimingTrajectory *planner);

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_PLANNER_STATE_H_

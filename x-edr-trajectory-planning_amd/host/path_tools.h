// path_tools.h -- the reference's trajectory_planning/path_tools.h for the host mirror:
// ProjectPointOnPath (path_tools.h:26-100; it lives in spline_edit.h, where the path switch uses it)
// and ComputeStoppingPoint (path_tools.cc:25-74). The batch forms run on the device
// (include/tpamd.h tpamd_compute_stopping_points_*, tpamd_project_points_on_paths_*), bit-identical
// to these; PathTimingTrajectorySet::RetargetWaypointPaths applies them to moving planners.
#ifndef TPAMD_HOST_PATH_TOOLS_H_
#define TPAMD_HOST_PATH_TOOLS_H_

#include "compat.h"
#include "spline_edit.h"        // ProjectedPointResult, ProjectPointOnPath

namespace trajectory_planning {

// Returns a point computed from the location where the robot could come to a stop with linear
// motion when starting at `position` with `velocity` and not exceeding the given
// `acceleration_limit`. The returned point is shifted further along the offset from `position` to
// the stopping location to account for `corner_rounding`, which ensures that if the returned point
// is used as a waypoint the path timing problem is feasible within the acceleration limits.
::tpamd::compat::StatusOr<VectorXd> ComputeStoppingPoint(Span<const double> position, Span<const double> velocity,
                                                         Span<const double> acceleration_limit,
                                                         double corner_rounding);

}  // namespace trajectory_planning

#endif  // TPAMD_HOST_PATH_TOOLS_H_

#include "path_tools.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace trajectory_planning {

using ::tpamd::compat::InvalidArgumentError;
using ::tpamd::compat::StatusOr;

namespace {

// PolyLineToBspline3WaypointsCornerOffset (splines/spline_utils.cc:25-45)
VectorXd CornerOffset(const VectorXd &delta, double radius) {
  const size_t n = delta.size();
  VectorXd offset(n);
  const double norm = delta.norm();
  for (size_t i = 0; i < n; i++) offset[i] = norm > 1e-6 ? delta[i] / norm : 0.0;
  const double kSpacing = 4.0;  // spline_utils.h:44-46
  if (norm > kSpacing * radius) {
    for (size_t i = 0; i < n; i++) offset[i] = offset[i] * radius;
  } else {
    for (size_t i = 0; i < n; i++) offset[i] = offset[i] * (1.0 / kSpacing) * norm;
  }
  return offset;
}

// eigenmath::ScaleDownToLimits is outside the reference tree; restated: the vector scaled
// uniformly, by the smallest limit / |value| over the components that exceed their limit, so that
// none does.
VectorXd ScaleDownToLimits(const VectorXd &value, const VectorXd &limits) {
  double factor = 1.0;
  for (size_t i = 0; i < value.size(); i++) {
    const double a = std::fabs(value[i]);
    if (a > limits[i]) factor = std::min(factor, limits[i] / a);
  }
  VectorXd out(value.size());
  for (size_t i = 0; i < value.size(); i++) out[i] = value[i] * factor;
  return out;
}

}  // namespace

StatusOr<VectorXd> ComputeStoppingPoint(Span<const double> position, Span<const double> velocity,
                                        Span<const double> acceleration_limit, double corner_rounding) {
  if (position.size() != velocity.size()) return InvalidArgumentError("position.size != velocity.size.");
  if (position.size() != acceleration_limit.size()) return InvalidArgumentError("position.size != acceleration.size.");
  const size_t n = position.size();
  const VectorXd pos(position.data(), n), vel(velocity.data(), n), acc(acceleration_limit.data(), n);
  double min_acc = std::numeric_limits<double>::infinity(), max_acc = -std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < n; i++) {
    min_acc = std::min(min_acc, acc[i]);
    max_acc = std::max(max_acc, acc[i]);
  }
  if (min_acc <= 0.0) return InvalidArgumentError("Acceleration limits must be strictly positive.");
  if (vel.maxAbs() < std::numeric_limits<double>::epsilon() * 100) return pos;

  // Maximum stopping deceleration that is collinear to `velocity` and within `acceleration_limit`.
  const double norm = vel.norm();
  VectorXd direction(n);
  for (size_t i = 0; i < n; i++) direction[i] = -(vel[i] / norm) * max_acc;
  const VectorXd stopping_deceleration = ScaleDownToLimits(direction, acc);
  // vel + time * stopping_deceleration is a scalar equation in the direction of vel: all components
  // are zero at the same time, found after projecting onto vel.
  const double stop_time = -vel.squaredNorm() / vel.dot(stopping_deceleration);
  VectorXd stopping_delta(n);
  for (size_t i = 0; i < n; i++) stopping_delta[i] = stop_time * (vel[i] + 0.5 * stop_time * stopping_deceleration[i]);
  // An additional offset for the spline's corner rounding: with the returned point as a waypoint
  // the spline is a straight line from `position` until `position + stopping_delta`.
  const VectorXd corner_rounding_distance = CornerOffset(stopping_delta, corner_rounding);
  VectorXd out(n);
  for (size_t i = 0; i < n; i++) out[i] = pos[i] + stopping_delta[i] + corner_rounding_distance[i];
  return out;
}

}  // namespace trajectory_planning

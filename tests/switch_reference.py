"""An independent statement of the spline edits that run on the device: the online path switch
(k_pset_switch, csrc/tpamd_switch.h) and the waypoint fit (k_pset_set_waypoints, csrc/tpamd_fit.h).
Plain Python, numpy, fractions and mpmath; nothing is imported from the product, and nothing here
was written from csrc/ or host/.

A. A restatement in Python floats (IEEE doubles), every operation in the order of the reference's
   sources, each function citing the lines it follows. It gives the same bits as an implementation
   that follows the same sources.
B. Property checkers (check_switch, check_fit, check_velocity) that take the inputs and outputs of
   any implementation and do not depend on an order of operations: both curves are evaluated
   exactly (fractions.Fraction of the doubles), so the checks add no rounding of their own.
C. Deterministic case generators shared by the CPU and the GPU tests.

What bit parity rests on (assumptions, since the code is outside the reference tree):
  * eigenmath::DistanceFromLineSegment(a, b, p, &distance, &t) is taken as: ab = b - a,
    t = (p - a).ab / ab.ab (0 for a zero-length segment), limited to t <= 1 and NOT limited below
    (SwitchToWaypointPath tells "before the first waypoint" by a negative line parameter,
    timeable_path_joint_spline.cc:234-240), distance = |a + max(t, 0) ab - p|. This is what
    path_tools_test.cc:56-115 pins (t = 0 on the first point, 1 on the last, 0.4 between, and the
    distance). eigenmath::InterpolateLinear(t, a, b) is taken as the lerp a + t (b - a), and the
    five-argument form as a + ((time - t0) / (t1 - t0)) (b - a); for the bracket (n-1, n-1) at the
    last time stamp, where t1 == t0, the sample itself. Bit parity of the projection and of the
    velocity rests on these forms; the property checkers cover them independently (least distance
    by a brute-force pass in exact arithmetic, the lerp against the exact lerp).
  * Eigen's norm() and dot products are taken as sequential sums (a scalar, unvectorised Eigen)
    and nothing is contracted to a fused multiply-add.

Deviations of the device from the reference, which the restatement follows where marked (R):
  * (R) TruncateSplineAt (bspline.h:404-428) calls the knot insertion that solves for the new
    control points with Eigen's colPivHouseholderQr (bspline.h:280-401). The device and this file
    use the closed form of the same insertion (bspline.h:244-278, NURBS A5.1). Both keep the
    curve; they differ by the solver's rounding, which cannot be restated.
  * The device takes the knot capacity as max(2 K + 3 W + 8, 100) at each switch (K knots, W new
    waypoints); the reference fixes it at the fit (timeable_path_joint_spline.cc:261-266). The
    restatement takes the capacity as an argument; device_capacity(K, W) gives the device's.
  * A failed edit leaves the planner unchanged on the device. The reference leaves a truncated
    spline and kModifiedPath. The restatement returns the status alone.
  * (R) A stop exactly on an interior knot gives that knot multiplicity 4, the join a double knot
    and basis[1] not above 0: the reference CHECK-fails (bspline.h:486). The device returns
    FAILED_PRECONDITION with nothing changed, and so does the restatement.
  * (R) ExtendWithControlPoints with fewer than 2 points is UnimplementedError; the device's
    status for it is INTERNAL. No waypoint left after the switch position (an empty polyline,
    which the reference would dereference, spline_utils.cc:53) is INVALID_ARGUMENT.
  * (R) "No path to switch from" (no knots) is FAILED_PRECONDITION; the device checks the spline
    as BSplineT::Init / SetKnotVector would (bspline_base.cc:106-132) before the edit.

Tolerances of check_switch (B.1, B.2) are measured on the restatement itself, never on a kernel:
MEASURED_RESIDUALS holds the worst residual over every successful switch of make_rounds(D) for
D = 1..16 (three rounds of 67 planners each, stops down to 1e-9 to either side of a knot), relative
to max(1, largest |control point|); TOLERANCES is 8 times that, for other seeds and joint counts.
tests/test_switch_reference_cpu.py re-measures and holds the recorded figures to the measurement.
"""
import bisect
import math
from fractions import Fraction

import mpmath
import numpy as np

OK, FAILED_PRECONDITION, OUT_OF_RANGE, INVALID_ARGUMENT, INTERNAL = 0, 1, 2, 3, 4
STATUS_NAMES = {0: "ok", 1: "failed_precondition", 2: "out_of_range", 3: "invalid_argument", 4: "internal"}
INF = float("inf")
ROUNDING = 0.2                   # PathOptions::rounding() default
EPSILON = 1e-3                   # kEpsilon, timeable_path_joint_spline.cc:229
U = 2.0 ** -53                   # unit roundoff of a double

# Worst residuals of the restatement over make_rounds(D), D = 1..16 (see the module docstring), and
# the bounds the checkers use.
MEASURED_RESIDUALS = {"kept": 8.0e-17, "join": 3.6e-16}
TOLERANCES = {k: 8 * v for k, v in MEASURED_RESIDUALS.items()}


class SwitchCheckError(AssertionError):
    pass


def _require(cond, *what):
    if not cond:
        raise SwitchCheckError(" ".join(str(w) for w in what))


# =========================================================================== A. the restatement
class Spline:
    """BSplineT<SplineTraitsXd> of degree 2: knots_[0 .. num_knots), points_[0 .. num_points),
    umin_, umax_ and the capacity of the arrays allocated in Init (bspline.h:144-175)."""

    def __init__(self, knots, points, capacity):
        self.knots = [float(x) for x in knots]
        self.points = [[float(x) for x in p] for p in points]
        self.capacity = int(capacity)
        self.umin, self.umax = self.knots[0], self.knots[-1]     # SetKnotVector, bspline_base.cc:138-157

    num_knots = property(lambda self: len(self.knots))
    num_points = property(lambda self: len(self.points))


def device_capacity(num_knots, W):
    return max(2 * num_knots + 3 * W + 8, 100)


def check_knot_vector(knots, points, capacity):
    """BSplineBase::Init / SetKnotVector / SetControlPoints (bspline_base.cc:33-57, :106-132,
    bspline.h:196-205) for degree 2: the status a spline of these arrays would be refused with."""
    nk = len(knots)
    if nk < 6 or nk > capacity:
        return OUT_OF_RANGE
    if len(points) != nk - 3:
        return INVALID_ARGUMENT
    for i in range(1, nk):
        if knots[i - 1] > knots[i]:
            return INVALID_ARGUMENT
    return OK


def _div(a, b):
    """a / b as IEEE 754 has it where Python raises: x / 0 is an infinity, 0 / 0 a NaN (a stop
    on a knot evaluates the truncated curve with 0 / 0, as the C++ does, and goes on)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or a != a:
        return float("nan")
    return math.copysign(INF, a) * math.copysign(1.0, b)


def knot_span(s, u):
    """BSplineBase::KnotSpan, bspline_base.cc:218-246: u equal to the last knot gives
    num_points - 1; otherwise std::lower_bound over knots[degree .. num_knots - degree) with the
    comparator a <= b, i.e. the first knot there that is not <= u, minus one."""
    nk = s.num_knots
    if nk == 0:
        return 0
    if u == s.knots[nk - 1]:
        return s.num_points - 1
    one_past = nk - 2
    for i in range(2, nk - 2):
        if not (s.knots[i] <= u):
            one_past = i
            break
    return one_past - 1


def update_basis(s, span, u):
    """BSplineBase::UpdateBasis, bspline_base.cc:249-265 (NURBS A2.2), p = 2."""
    p = 2
    basis = [0.0] * (p + 1)
    left, right = [0.0] * (p + 1), [0.0] * (p + 1)
    basis[0] = 1.0
    for j in range(1, p + 1):
        left[j] = u - s.knots[span + 1 - j]      # knots_(seqN(span, p, -1))
        right[j] = s.knots[span + j] - u
    for j in range(1, p + 1):
        saved = 0.0
        for r in range(j):
            tmp = _div(basis[r], right[r + 1] + left[j - r])
            basis[r] = saved + right[r + 1] * tmp
            saved = left[j - r] * tmp
        basis[j] = saved
    return basis


def eval_curve(s, u):
    """BSplineT::EvalCurve, bspline.h:514-536: (status, value)."""
    if u < s.umin or u > s.umax:
        return OUT_OF_RANGE, None
    span = knot_span(s, u)
    basis = update_basis(s, span, u)
    D = len(s.points[0])
    value = [0.0] * D
    for i in range(3):
        p = s.points[span - 2 + i]
        for d in range(D):
            value[d] += basis[i] * p[d]
    return OK, value


def can_insert_knot(s, knot, multiplicity):
    """BSplineBase::CanInsertKnot, bspline_base.cc:166-195."""
    if multiplicity > 2 + 1:
        return INVALID_ARGUMENT
    if s.num_knots + multiplicity > s.capacity:
        return FAILED_PRECONDITION
    if s.num_knots < 2:
        return FAILED_PRECONDITION
    if knot <= s.knots[0] or knot >= s.knots[s.num_knots - 1]:
        return INVALID_ARGUMENT
    return OK


def insert_knot_once(s, knot):
    """BSplineT::InsertKnotAndUpdateControlPointsRef(knot), bspline.h:244-278, and
    InsertKnotIntoKnotVector, bspline_base.cc:197-213."""
    span = knot_span(s, knot)
    D = len(s.points[0])
    # copy_backward(points + span, points + num_points, points + num_points + 1): span keeps its value
    s.points.insert(span, list(s.points[span]))
    scratch = []
    for i in range(2):
        k = span + i - 2 + 1
        alpha = _div(knot - s.knots[k], s.knots[k + 2] - s.knots[k])
        scratch.append([alpha * s.points[k][d] + (1.0 - alpha) * s.points[k - 1][d] for d in range(D)])
    for i in range(2):
        s.points[span - 2 + 1 + i] = scratch[i]
    # copy_backward(knots + span, knots + num_knots, ... + 1), then knots[span + 1] = knot
    s.knots.insert(span + 1, knot)


def insert_knot(s, knot, multiplicity):
    """BSplineT::InsertKnotAndUpdateControlPoints[Ref](knot, multiplicity), bspline.h:224-242."""
    st = can_insert_knot(s, knot, multiplicity)
    if st != OK:
        return st
    for _ in range(multiplicity):
        insert_knot_once(s, knot)
    return OK


def truncate_spline_at(s, u_end):
    """BSplineT::TruncateSplineAt, bspline.h:404-428."""
    if u_end >= s.umax:
        return OK
    if u_end <= s.umin:
        s.umin, s.umax = INF, -INF
        s.knots, s.points = [], []
        return OK
    st = insert_knot(s, u_end, 2 + 1)
    if st != OK:
        return st
    span = knot_span(s, u_end)
    del s.knots[span + 1:]
    del s.points[len(s.knots) - 3:]
    s.umax = u_end
    return OK


def extend_with_control_points(s, points):
    """BSplineT::ExtendWithControlPoints, bspline.h:431-511. The knots of the new part are
    setLinSpaced(old_knot_range, new_knot_range): they start at old_knot_range, not at
    knots[0] + old_knot_range (:472-473), while the last three are knots[0] + new_knot_range (:475)."""
    num_knots, num_points, m = s.num_knots, s.num_points, len(points)
    new_num_points = num_points + m
    added_knots = (m + 1 + 2 + 1) - 2 * 2
    new_num_knots = num_knots + added_knots
    if num_knots < 6:
        return FAILED_PRECONDITION
    if new_num_points > s.capacity - 3:
        return FAILED_PRECONDITION
    if new_num_knots > s.capacity:
        return FAILED_PRECONDITION
    if m < 2:
        return INTERNAL                      # UnimplementedError
    u_join = s.knots[num_knots - 1]
    old_knot_range = s.knots[num_knots - 1] - s.knots[0]
    old_inner_knot_count = num_knots - 2 * 2 - 1
    new_inner_knot_count = new_num_knots - 2 * 2 - 1
    new_knot_range = (old_knot_range * new_inner_knot_count) / old_inner_knot_count
    linspace_upper_bound = new_num_knots - 2
    linspace_start_index = num_knots - 2 - 1
    linspace_size = linspace_upper_bound - linspace_start_index
    s.knots.extend([0.0] * added_knots)
    # Eigen's linspaced_op for low <= high: low + i * ((high - low) / (size - 1)), the last one = high
    step = (new_knot_range - old_knot_range) / (1 if linspace_size <= 1 else linspace_size - 1)
    for i in range(linspace_size):
        s.knots[linspace_start_index + i] = new_knot_range if i == linspace_size - 1 else old_knot_range + i * step
    for i in range(3):
        s.knots[new_num_knots - 3 + i] = s.knots[0] + new_knot_range
    s.umax = s.knots[new_num_knots - 1]
    span = knot_span(s, u_join)              # num_points_ is still the old count; u_join is not the last knot
    modified = num_points - 1
    basis = update_basis(s, span, u_join)
    if not basis[1] > 0:
        return FAILED_PRECONDITION           # CHECK(basis[1] > 0), bspline.h:486
    D = len(s.points[0])
    s.points[modified] = [1.0 / basis[1] * (s.points[modified][d] - basis[0] * s.points[modified - 1][d])
                          for d in range(D)]
    for p in points:
        s.points.append(list(p))
    return OK


def _norm(v):
    sq = 0.0
    for x in v:
        sq += x * x
    return float(np.sqrt(sq))


def corner_offset(delta, radius):
    """PolyLineToBspline3WaypointsCornerOffset, spline_utils.cc:25-45 (kMinWaypointSpacingFactor 4)."""
    norm = _norm(delta)
    offset = [x / norm for x in delta] if norm > 1e-6 else [0.0] * len(delta)
    if norm > 4.0 * radius:
        return [x * radius for x in offset]
    return [x * (1.0 / 4.0) * norm for x in offset]


def polyline_to_bspline3_waypoints(corners, radius):
    """PolyLineToBspline3Waypoints (VectorXd), spline_utils.cc:47-102."""
    if len(corners) == 1:
        return [list(corners[0]) for _ in range(4)]
    n = 3 * len(corners) - 2
    out = [None] * n
    for i, c in enumerate(corners):
        out[3 * i] = list(c)
    sub = lambda a, b: [x - y for x, y in zip(a, b)]
    add = lambda a, b: [x + y for x, y in zip(a, b)]
    for i in range(1, len(corners) - 1):
        k = 3 * i
        out[k + 1] = add(out[k], corner_offset(sub(out[k + 3], out[k]), radius))
        out[k - 1] = add(out[k], corner_offset(sub(out[k - 3], out[k]), radius))
    out[1] = add(out[0], corner_offset(sub(out[3], out[0]), radius))
    out[n - 2] = add(out[n - 1], corner_offset(sub(out[n - 4], out[n - 1]), radius))
    return out


def distance_from_line_segment(a, b, p):
    """eigenmath::DistanceFromLineSegment as assumed in the module docstring: (distance, t)."""
    ab2 = ap_ab = 0.0
    for x, y, z in zip(a, b, p):
        ab2 += (y - x) * (y - x)
        ap_ab += (z - x) * (y - x)
    t = ap_ab / ab2 if ab2 > 0.0 else 0.0
    if t > 1.0:
        t = 1.0
    tc = 0.0 if t < 0.0 else t
    return _norm([(x + tc * (y - x)) - z for x, y, z in zip(a, b, p)]), t


def project_point_on_path(waypoints, point):
    """ProjectPointOnPath, path_tools.h:57-100: (status, index, line_parameter, projected_point)."""
    if not waypoints:
        return INVALID_ARGUMENT, 0, 0.0, None
    if len(waypoints) == 1:
        return OK, 0, 0.0, list(waypoints[0])
    best, index, line_parameter = np.finfo(np.float64).max, 0, 0.0
    for i in range(len(waypoints) - 1):
        distance, t = distance_from_line_segment(waypoints[i], waypoints[i + 1], point)
        if distance < best:
            best, line_parameter, index = distance, t, i
    a, b = waypoints[index], waypoints[index + 1]
    return OK, index, line_parameter, [x + line_parameter * (y - x) for x, y in zip(a, b)]


def switch_to_waypoint_path(knots, points, keep_path_until, waypoints, capacity=None, rounding=ROUNDING):
    """TimeableJointSplinePath::SwitchToWaypointPath, timeable_path_joint_spline.cc:209-250.
    Returns dict(status, knots, points) and what the edit went through (np_kept, index,
    line_parameter, projected_kept, first_waypoint, num_new, switch_position)."""
    res = dict(status=OK, knots=None, points=None)
    keep_path_until = float(keep_path_until)
    waypoints = [[float(x) for x in w] for w in waypoints]
    if len(knots) == 0:
        return dict(res, status=FAILED_PRECONDITION)
    if capacity is None:
        capacity = device_capacity(len(knots), len(waypoints))
    st = check_knot_vector(knots, points, capacity)
    if st != OK:
        return dict(res, status=st)
    s = Spline(knots, points, capacity)
    st = truncate_spline_at(s, keep_path_until)
    if st != OK:
        return dict(res, status=st)
    st, switch_position = eval_curve(s, keep_path_until)
    if st != OK:
        return dict(res, status=st)
    res.update(np_kept=s.num_points, switch_position=switch_position)
    st, index, line_parameter, projected = project_point_on_path(waypoints, switch_position)
    if st != OK:
        return dict(res, status=st)
    new_waypoints = []
    inf_norm = 0.0
    for x, y in zip(switch_position, projected):
        inf_norm = max(inf_norm, abs(x - y))
    if inf_norm > EPSILON:
        new_waypoints.append(projected)
    first_waypoint = index + 1 if line_parameter >= 0 else index
    new_waypoints.extend(list(w) for w in waypoints[first_waypoint:])
    res.update(index=index, line_parameter=line_parameter, projected_kept=inf_norm > EPSILON,
               first_waypoint=first_waypoint, num_new=len(new_waypoints), inf_norm=inf_norm)
    if not new_waypoints:
        return dict(res, status=INVALID_ARGUMENT)
    control_points = polyline_to_bspline3_waypoints(new_waypoints, rounding)
    st = extend_with_control_points(s, control_points)
    if st != OK:
        return dict(res, status=st)
    return dict(res, knots=s.knots, points=s.points)


def fit_spline_to_waypoints(waypoints, rounding=ROUNDING):
    """TimeableJointSplinePath::FitSplineToWaypoints, timeable_path_joint_spline.cc:252-292, with
    MakeUniformKnotVector (bspline_base.cc:356-399) on [0, 1]: (status, knots, control_points). An
    empty list is "Control point vector empty." (bspline.h:181)."""
    if not waypoints:
        return INVALID_ARGUMENT, None, None
    cp = polyline_to_bspline3_waypoints(waypoints, rounding)
    nknots = len(cp) + 2 + 1
    knots = [0.0] * nknots
    spacing = (1.0 / (nknots - 2.0 * (2 + 1.0) + 1.0)) * (1.0 - 0.0)
    for i in range(3, nknots - 3):
        knots[i] = knots[i - 1] + spacing
    for i in range(nknots - 3, nknots):
        knots[i] = 1.0
    length = 0.0
    for i in range(len(cp) - 1):
        length += _norm([y - x for x, y in zip(cp[i], cp[i + 1])])
    weighted = max(length * 1.0, 0.1)
    return OK, [k * weighted for k in knots], cp


def get_offset_bracket(times, time_sec):
    """TrajectoryBuffer::GetOffsetBracket, trajectory_buffer.cc:233-251: (status, lower, upper)."""
    if len(times) == 0:
        return FAILED_PRECONDITION, 0, 0
    if time_sec < times[0] or time_sec > times[-1]:
        return OUT_OF_RANGE, 0, 0
    upper = len(times)
    for i, t in enumerate(times):            # std::upper_bound
        if t > time_sec:
            upper = i
            break
    if upper == len(times):
        return OK, upper - 1, upper - 1
    return OK, upper - 1, upper


def velocity_at_time(times, velocities, time_sec):
    """TrajectoryBuffer::GetVelocityAtTime, trajectory_buffer.cc:269-278: (status, velocity)."""
    st, lo, up = get_offset_bracket(times, time_sec)
    if st != OK:
        return st, None
    if lo == up:
        return OK, [float(x) for x in velocities[lo]]
    f = (time_sec - times[lo]) / (times[up] - times[lo])
    return OK, [float(a) + f * (float(b) - float(a)) for a, b in zip(velocities[lo], velocities[up])]


def points_bound(P, W):
    """What a switch may give a spline of P points and W new waypoints: P + 3 inserted knots and
    the polygon of W + 1 waypoints (the projected point included)."""
    return P + 3 + 3 * (W + 1) - 2


# =========================================================================== B. property checkers
def _fr(rows):
    return [[Fraction(float(x)) for x in r] for r in rows]


def exact_curve(knots, points, u):
    """The degree-2 B-spline curve at u in exact arithmetic (Cox-de Boor, a term with a zero
    denominator is zero). knots / points: Fractions; u: a Fraction inside the knot range."""
    nk, npts = len(knots), len(points)
    if u == knots[nk - 1]:
        span = npts - 1
    else:
        span = bisect.bisect_right(knots, u, 2, nk - 2) - 1
    N = [Fraction(1), Fraction(0), Fraction(0)]
    for j in (1, 2):
        saved = Fraction(0)
        for r in range(j):
            right, left = knots[span + r + 1] - u, u - knots[span + 1 - (j - r)]
            den = right + left
            tmp = N[r] / den if den != 0 else Fraction(0)
            N[r] = saved + right * tmp
            saved = left * tmp
        N[j] = saved
    D = len(points[0])
    return [sum(N[i] * points[span - 2 + i][d] for i in range(3)) for d in range(D)]


def _exact_projection(waypoints, point):
    """Brute force over all segments in exact arithmetic: per segment (squared distance to the
    segment, the line parameter limited to <= 1 only, the point a + t (b - a))."""
    out = []
    for a, b in zip(waypoints[:-1], waypoints[1:]):
        ab = [y - x for x, y in zip(a, b)]
        ab2 = sum(x * x for x in ab)
        t = sum((z - x) * w for x, z, w in zip(a, point, ab)) / ab2 if ab2 else Fraction(0)
        t = min(t, Fraction(1))
        tc = max(t, Fraction(0))
        d2 = sum((x + tc * w - z) ** 2 for x, w, z in zip(a, ab, point))
        out.append((d2, t, [x + t * w for x, w in zip(a, ab)]))
    return out


def kept_points(old_knots, keep):
    """Control points a truncation at `keep` leaves: the old knots strictly below it (or all)."""
    if keep >= old_knots[-1]:
        return len(old_knots) - 3
    return sum(1 for k in old_knots if k < keep)


def check_switch(old_knots, old_points, keep, waypoints, new_knots, new_points, tolerances=None, residuals=None,
                 decision_slack=1e-9):
    """The meaning of a successful switch (old spline with a zero first knot, stop parameter
    `keep` inside (umin, umax], W >= 1 waypoints -> new spline), whatever computed it:
      1. on [first knot, last new knot strictly below the join) the new curve is the old one
         (three exact evaluations per non-empty span fix a quadratic). The last kept span is
         left out: its knots move from (u, u, u) to (u, u + h, u + 2 h) by design;
      2. the new curve at the join is the old curve at the stop parameter;
      3. the knots do not decrease and are strictly increasing from the knot before the join to
         the first of the three end knots (no interior multiplicity: C1 at the join and after);
      4. the new curve's end and the last control point are the last waypoint exactly;
      5. the point count is kept + max(3 n - 2, 4) for the n new waypoints, within points_bound;
      6.-8. there is a segment of least distance (exact, brute force) from the switch position to
         the given polyline such that the projected point a + t (b - a) is the first new waypoint
         exactly when its infinity-norm distance is above 1e-3, and the given waypoints follow
         from index + 1 for t >= 0, from index for t < 0. The implementation decides these in
         doubles on a switch position that carries rounding, so the checker allows for it: a
         segment within a relative 1e-12 of the least squared distance counts as least, and a
         decision within `decision_slack` of its threshold (t against 0, the infinity norm against
         1e-3) may go either way. The result's "in_slack" says whether the case used any of that;
         the shared cases never do (tests/test_switch_reference_cpu.py asserts it).
    Residuals of 1. and 2. are relative to max(1, largest |control point|); the largest seen are
    recorded in `residuals` ("kept", "join")."""
    tol = TOLERANCES if tolerances is None else tolerances
    D, W, P = len(old_points[0]), len(waypoints), len(old_points)
    ok, op = [Fraction(float(x)) for x in old_knots], _fr(old_points)
    nk_, np_ = [Fraction(float(x)) for x in new_knots], _fr(new_points)
    _require(len(new_knots) == len(new_points) + 3, "knot count", len(new_knots), len(new_points))
    scale = max(1.0, max(abs(float(x)) for r in old_points for x in r), max(abs(float(x)) for r in new_points for x in r))
    kept = kept_points([float(x) for x in old_knots], float(keep))
    _require(3 <= kept <= len(new_points) - 4, "kept points", kept, len(new_points))
    nk_kept = kept + 3
    join = nk_kept - 3                                   # new_knots[join] is the join
    u_keep = min(Fraction(float(keep)), ok[-1])
    # 3. the knots
    for i in range(1, len(nk_)):
        _require(nk_[i - 1] <= nk_[i], "knots decrease at", i)
    for i in range(join, len(nk_) - 2):
        _require(nk_[i - 1] < nk_[i], "knots not strictly increasing at", i, float(nk_[i - 1]), float(nk_[i]))
    _require(nk_[0] == ok[0] and nk_[join] == u_keep - ok[0], "join knot", float(nk_[join]), float(u_keep))
    # 1. the kept part
    worst = 0.0
    for i in range(2, join - 1):                         # spans [k_i, k_i+1) with k_i+1 <= new_knots[join - 1]
        _require(nk_[i] == ok[i] and nk_[i + 1] == ok[i + 1], "kept knot changed", i)
        if nk_[i] == nk_[i + 1]:
            continue
        for f in (Fraction(0), Fraction(1, 3), Fraction(2, 3)):
            u = nk_[i] + f * (nk_[i + 1] - nk_[i])
            a, b = exact_curve(ok, op, u), exact_curve(nk_, np_, u)
            worst = max(worst, max(abs(float(x - y)) for x, y in zip(a, b)) / scale)
    _require(worst <= tol["kept"], "kept part differs", worst, tol["kept"])
    # 2. the join
    at = exact_curve(ok, op, u_keep)
    got = exact_curve(nk_, np_, nk_[join])
    r_join = max(abs(float(x - y)) for x, y in zip(at, got)) / scale
    _require(r_join <= tol["join"], "join differs", r_join, tol["join"])
    if residuals is not None:
        residuals["kept"] = max(residuals.get("kept", 0.0), worst)
        residuals["join"] = max(residuals.get("join", 0.0), r_join)
    # 4. the end
    last = [Fraction(float(x)) for x in waypoints[-1]]
    _require(np_[-1] == last, "last control point is not the last waypoint")
    _require(exact_curve(nk_, np_, nk_[-1]) == last, "the curve does not end on the last waypoint")
    # 5. the count
    m = len(new_points) - kept
    _require(m >= 4 and (m == 4 or (m + 2) % 3 == 0), "added points", m)
    _require(len(new_points) <= points_bound(P, W), "points bound", len(new_points), points_bound(P, W))
    if m > 4:
        counts = [(m + 2) // 3]
    else:
        counts = [1, 2] if all(np_[kept + i] == np_[kept] for i in range(4)) else [2]     # two equal waypoints look like one
    # 6.-8. the projection and which waypoints are kept
    wf = _fr(waypoints)
    if W == 1:
        candidates = [(Fraction(0), Fraction(0), wf[0], 0)]
    else:
        segs = _exact_projection(wf, at)
        dmin = min(s[0] for s in segs)
        candidates = [s + (i,) for i, s in enumerate(segs) if s[0] <= dmin * (1 + Fraction(1, 10 ** 12))]
    reasons = []
    for n in counts:
        new_wps = [np_[kept + 3 * i] for i in range(n)] if m > 4 or n == 2 else [np_[kept]]
        for d2, t, proj, index in candidates:
            inf_norm = max(abs(x - y) for x, y in zip(at, proj))
            for has_proj in (True, False):
                if has_proj and inf_norm <= Fraction(EPSILON) - Fraction(decision_slack):
                    continue
                if not has_proj and inf_norm > Fraction(EPSILON) + Fraction(decision_slack):
                    continue
                for first in ((index + 1, index) if abs(t) <= decision_slack else (index + 1,) if t >= 0 else (index,)):
                    if W == 1:
                        first = 1
                    if n != int(has_proj) + W - first:
                        reasons.append(("count", n, has_proj, first, index))
                        continue
                    if new_wps[int(has_proj):] != wf[first:]:
                        reasons.append(("waypoints", index, first))
                        continue
                    if has_proj:
                        err = max(abs(float(x - y)) for x, y in zip(new_wps[0], proj))
                        if err > 64 * U * max(1.0, float(abs(t))) * scale:
                            reasons.append(("projected point", index, err))
                            continue
                    # in_slack: the case sits where the checker lets a decision go either way
                    in_slack = (W > 1 and any(c[0] != dmin for c in candidates)) or \
                        0 < abs(t) <= decision_slack or abs(inf_norm - Fraction(EPSILON)) <= decision_slack
                    return dict(kept=kept, num_new=n, index=index, has_proj=has_proj, first=first,
                                residual_kept=worst, residual_join=r_join, in_slack=bool(in_slack))
    raise SwitchCheckError("no least-distance segment explains the new waypoints: %s" % (reasons[:6],))


def check_fit(waypoints, rounding, knots, points):
    """The meaning of a fit of W >= 1 waypoints:
      1. control points 0, 3, 6, ... are the waypoints (W = 1: four copies);
      2. the curve starts on the first waypoint and ends on the last (exact evaluation);
      3. the knots are uniform: three equal at either end, knot i = (i - 2) / (K - 5) of the last
         within (2 (K - 5) + 2) 2^-53 of the last knot (the spacing 1 / (K - 5) carries one
         rounding, the running sum of j <= K - 5 terms at most j more, each relative to a partial
         sum <= 1, and the scaling one more);
      4. the last knot is max(L, 0.1) with L the length of the control polygon given by `points`,
         computed with 50 digits. For P points of D joints the double sum carries per segment one
         rounding per difference, one per square, D - 1 for the sum and (halved by the root) one
         for the root, i.e. at most ((D + 1) / 2 + 1) 2^-53 relative, and P - 2 roundings for the
         sum of the segments: the bound is (D / 2 + P + 1) 2^-53 L, times 1.01 for second order."""
    W, P, K = len(waypoints), len(points), len(knots)
    D = len(waypoints[0])
    _require(P == (4 if W == 1 else 3 * W - 2) and K == P + 3, "sizes", W, P, K)
    for i, w in enumerate(waypoints):
        _require([float(x) for x in points[3 * i]] == [float(x) for x in w], "control point", 3 * i, "is not waypoint", i)
    if W == 1:
        _require(all(list(p) == list(points[0]) for p in points), "one waypoint: four copies")
    fk, fp = [Fraction(float(x)) for x in knots], _fr(points)
    _require(exact_curve(fk, fp, fk[0]) == fp[0] == [Fraction(float(x)) for x in waypoints[0]], "start")
    _require(exact_curve(fk, fp, fk[-1]) == fp[-1] == [Fraction(float(x)) for x in waypoints[-1]], "end")
    last = float(knots[-1])
    _require(knots[0] == knots[1] == knots[2] == 0.0 and knots[-3] == knots[-2] == last, "end knots")
    for i in range(3, K - 3):
        want = Fraction(i - 2, K - 5) * Fraction(last)
        _require(abs(float(Fraction(float(knots[i])) - want)) <= (2 * (K - 5) + 2) * U * last, "knot", i, "not uniform")
    with mpmath.workdps(50):
        L = mpmath.mpf(0)
        for a, b in zip(points[:-1], points[1:]):
            L += mpmath.sqrt(sum((mpmath.mpf(float(y)) - mpmath.mpf(float(x))) ** 2 for x, y in zip(a, b)))
        bound = 1.01 * (D / 2.0 + P + 1) * U * float(L)
        want = max(L, mpmath.mpf("0.1"))
        _require(abs(mpmath.mpf(last) - want) <= bound + (U * 0.1 if L < 0.1 + bound else 0), "last knot", last, float(want))
    # rounded corners stay on the segments' lines, in order (W >= 2)
    for i in range(W - 1):
        a, b = fp[3 * i], fp[3 * i + 3]
        for j in (1, 2):
            c = fp[3 * i + j]
            ab2 = sum((y - x) ** 2 for x, y in zip(a, b))
            if ab2 == 0:
                continue
            t = sum((z - x) * (y - x) for x, y, z in zip(a, b, c)) / ab2
            _require(0 <= t <= 1, "inner point outside its segment", i, j, float(t))
            off = max(abs(float(x + t * (y - x) - z)) for x, y, z in zip(a, b, c))
            _require(off <= 8 * U * max(1.0, max(abs(float(x)) for x in a + b)), "inner point off its segment", i, j, off)


def check_velocity(times, velocities, time_sec, status, velocity):
    """GetVelocityAtTime: no samples FAILED_PRECONDITION, a time outside the samples OUT_OF_RANGE;
    else the bracket is (i - 1, i) for the first time stamp i above time_sec (upper_bound), the
    last sample alone at the last time stamp, and the value the exact lerp
    a + (t - t_l) / (t_u - t_l) (b - a) within the roundings of its double evaluation: t - t_l,
    t_u - t_l and their quotient give the fraction f to 3 x 2^-53 relative, b - a and the product
    add one each, the final sum one more of the result: (5 |f (b - a)| + |v|) 2^-53, times 1.01."""
    n = len(times)
    if n == 0:
        _require(status == FAILED_PRECONDITION, "no samples", status)
        return
    if time_sec < times[0] or time_sec > times[-1]:
        _require(status == OUT_OF_RANGE, "outside", status)
        return
    _require(status == OK, "status", status)
    up = bisect.bisect_right([float(t) for t in times], time_sec)
    if up == n:
        _require([float(x) for x in velocity] == [float(x) for x in velocities[n - 1]], "last sample")
        return
    lo = up - 1
    f = (Fraction(time_sec) - Fraction(float(times[lo]))) / (Fraction(float(times[up])) - Fraction(float(times[lo])))
    for a, b, v in zip(velocities[lo], velocities[up], velocity):
        a, b = Fraction(float(a)), Fraction(float(b))
        want = a + f * (b - a)
        bound = 1.01 * U * (5 * abs(float(f * (b - a))) + abs(float(want)))
        _require(abs(float(Fraction(float(v)) - want)) <= bound, "lerp", float(v), float(want), bound)


# =========================================================================== C. case generators
NUM_PLANNERS, NUM_LISTED = 70, 67        # B and the listed planners: two waves, three live lanes in the last
WMAX, W0MAX = 6, 7                       # the largest W of a switch call; the largest first fit (P = 19)
KNOT_SHIFT = 0.004                       # the first knot of the "nonzero_first_knot" planner

# label -> expected status; every label occurs for every D (make_planners)
CATEGORIES = [
    ("inside", OK), ("on_knot", FAILED_PRECONDITION), ("past_knot", OK), ("before_knot", OK), ("first_span", OK),
    ("last_span", OK), ("at_umin", OUT_OF_RANGE), ("below_umin", OUT_OF_RANGE), ("at_umax", OK),
    ("past_umax", OUT_OF_RANGE), ("no_waypoints", INVALID_ARGUMENT), ("one_waypoint", OK), ("wmax", OK),
    ("near_projection", OK), ("negative_t_all_kept", OK), ("last_segment", OK), ("repeated_waypoint", OK),
    ("only_waypoint_is_switch_position", INVALID_ARGUMENT), ("nonzero_first_knot", OK), ("collinear", OK),
]
EXPECTED_STATUS = dict(CATEGORIES)


def _rows(a):
    return [[float(x) for x in r] for r in np.asarray(a, dtype=np.float64).reshape(len(a), -1)]


def make_planners(D):
    """The 67 listed planners of joint count D: label, first waypoints (W0 = 2..7, P = 4..19), the
    restated fit (knots, points) and limits. Planner b's label is CATEGORIES[b % 20]; the
    "negative_t_all_kept" planners get the largest P (they fill the work area and, with keep in
    the last span, use the most points), "nonzero_first_knot" has every knot moved by KNOT_SHIFT."""
    rng = np.random.default_rng(20261018 + D)
    planners = []
    for b in range(NUM_LISTED):
        label = CATEGORIES[b % len(CATEGORIES)][0]
        W0 = 2 + (b * 5 + b // 6) % 6
        if label in ("on_knot", "past_knot", "before_knot"):
            W0 = max(W0, 3)
        if label == "negative_t_all_kept":
            W0 = W0MAX
        wps = _rows(rng.uniform(-2.0, 2.0, size=(W0, D)))
        st, knots, points = fit_spline_to_waypoints(wps)
        assert st == OK
        if label == "nonzero_first_knot":
            knots = [k + KNOT_SHIFT for k in knots]
        planners.append(dict(label=label, waypoints=wps, knots=knots, points=points,
                             vmax=rng.uniform(1.0, 2.0, size=D).tolist(), amax=rng.uniform(2.0, 4.0, size=D).tolist(),
                             delta=float(rng.uniform(0.01, 0.03))))
    return planners


def _switch_position(knots, points, keep):
    s = Spline(knots, points, 10 ** 6)
    assert truncate_spline_at(s, keep) == OK
    st, at = eval_curve(s, keep)
    assert st == OK
    return at


def make_case(label, rng, knots, points):
    """One switch of category `label` on the spline (knots, points): dict(label, keep, waypoints,
    status, num_new) with the expected status and, for a success, the expected number of new
    waypoints (None where the geometry decides)."""
    D, nk = len(points[0]), len(knots)
    umin, umax = knots[0], knots[-1]
    W = int(rng.integers(2, 5))
    keep = umin + float(rng.uniform(0.05, 0.95)) * (umax - umin)
    interior = int(rng.integers(3, max(4, nk - 3)))          # an interior knot where there is one
    num_new = None
    if label == "on_knot":
        keep = knots[interior]
    elif label == "past_knot":
        keep = knots[interior] + 1e-9
    elif label == "before_knot":
        keep = knots[interior] - 1e-9
    elif label == "first_span":
        keep = knots[2] + float(rng.uniform(0.1, 0.9)) * (knots[3] - knots[2])
    elif label in ("last_span", "negative_t_all_kept"):
        keep = knots[nk - 4] + float(rng.uniform(0.1, 0.9)) * (knots[nk - 3] - knots[nk - 4])
    elif label == "at_umin":
        keep = umin
    elif label == "below_umin":
        keep = umin - 0.1
    elif label == "at_umax":
        keep = umax
    elif label == "past_umax":
        keep = umax + 0.05
    if label == "no_waypoints":
        W = 0
    elif label in ("one_waypoint", "only_waypoint_is_switch_position"):
        W = 1
    elif label in ("wmax", "negative_t_all_kept"):
        W = WMAX
    wps = _rows(rng.uniform(-2.0, 2.0, size=(W, D))) if W else []
    status = EXPECTED_STATUS.get(label, OK)
    if status == OK or label == "only_waypoint_is_switch_position":
        at = _switch_position(knots, points, min(keep, umax))
        if label == "one_waypoint":
            num_new = 1                                       # the projected point, which is the waypoint
        elif label == "only_waypoint_is_switch_position":
            wps = [list(at)]
        elif label == "near_projection":                      # the first segment passes within 1e-3: no projected point
            e = [1.0 + 0.05 * d for d in range(D)]
            off = [(2e-4 if d & 1 else -2e-4) / math.sqrt(D) * float(rng.uniform(0.2, 1.0)) for d in range(D)]
            wps[0] = [a - 3e-4 * x / _norm(e) + o for a, x, o in zip(at, e, off)]       # the switch position lies ahead: t > 0
            wps[1:] = [[w + 0.8 * i * x + (0.1 if (i + d) & 1 else 0.0) for d, (w, x) in enumerate(zip(wps[0], e))]
                       for i in range(1, W)]
            num_new = W - 1
        elif label == "negative_t_all_kept":                  # the first segment points away from the switch position
            wps[0] = [a + 1.0 + 0.1 * d for d, a in enumerate(at)]
            wps[1] = [x + 2.0 for x in wps[0]]
            for i in range(2, W):
                wps[i] = [x + 5.0 * i for x in wps[1]]
            num_new = W + 1 if D > 1 else W                   # one joint: every projection is the point itself
        elif label == "last_segment":                         # the last segment passes the switch position closely
            direction = [1.0 if d % 2 == 0 else -0.5 for d in range(D)]
            for i in range(W - 2):
                wps[i] = [a + 10.0 + 3.0 * i + 0.3 * d for d, a in enumerate(at)]
            wps[W - 2] = [a - 0.75 * v + 0.05 for a, v in zip(at, direction)]
            wps[W - 1] = [a + 1.25 * v + 0.05 for a, v in zip(at, direction)]
            num_new = 2 if D > 1 else None                    # one joint: an earlier segment passes through the point
        elif label == "repeated_waypoint":
            wps[1] = list(wps[0])
            if W > 3:
                wps[3] = list(wps[2])
        elif label == "collinear":
            wps = [[a + 0.5 + (0.7 * i + 0.1) * (1.0 + 0.05 * d) for d, a in enumerate(at)] for i in range(W)]
    return dict(label=label, keep=float(keep), waypoints=wps, status=status, num_new=num_new)


def make_rounds(D, rounds=3):
    """Three switches in a row on each of the 67 planners, by the restatement: round 0 is planner
    b's category, rounds 1 and 2 switch the result again (a failed planner switches its unchanged
    spline) with stops inside a span, next to a knot and in the last span in turn. Returns
    (planners, [round][b] -> dict(case, before=(knots, points), result))."""
    planners = make_planners(D)
    rng = np.random.default_rng(977 * D + 5)
    state = [(p["knots"], p["points"]) for p in planners]
    out = []
    for r in range(rounds):
        row = []
        for b, p in enumerate(planners):
            knots, points = state[b]
            label = p["label"] if r == 0 else ("inside", "past_knot", "last_span", "before_knot")[(b + r) % 4]
            if label in ("past_knot", "before_knot") and len(knots) < 7:
                label = "inside"
            case = make_case(label, rng, knots, points)
            res = switch_to_waypoint_path(knots, points, case["keep"], case["waypoints"])
            row.append(dict(case=case, before=(knots, points), result=res))
            if res["status"] == OK:
                state[b] = (res["knots"], res["points"])
        out.append(row)
    return planners, out


def reached(case, result, num_points_before, num_points_after):
    """The category `case` was reached by an implementation that returned `result` status and the
    point counts: the expected status, and for a success the expected count of added points."""
    if result != case["status"]:
        return False
    if result == OK and case["num_new"] is not None:
        kept = num_points_after - max(3 * case["num_new"] - 2, 4)
        return 3 <= kept <= num_points_before
    return result == OK or num_points_after == num_points_before


FIT_ROUNDINGS = (0.0, 0.2, 50.0)


def make_fit_cases(D):
    """Waypoint lists for the fit: W = 1, 2, 40, repeated and collinear waypoints, a polygon
    shorter than 0.1, and a few random ones; each with rounding 0, 0.2 and larger than every
    segment. One empty list (W = 0: INVALID_ARGUMENT, the planner keeps its state)."""
    rng = np.random.default_rng(31 * D + 7)
    lists = [("W1", rng.uniform(-2, 2, size=(1, D))), ("W2", rng.uniform(-2, 2, size=(2, D))),
             ("W40", rng.uniform(-2, 2, size=(40, D)))]
    rep = rng.uniform(-2, 2, size=(5, D))
    rep[2] = rep[1]
    rep[4] = rep[3]
    lists.append(("repeated", rep))
    lists.append(("collinear", np.outer(np.array([0.0, 0.3, 0.9, 1.0, 2.5]), rng.uniform(-1, 1, size=D)) + 0.25))
    lists.append(("short", 0.5 + rng.uniform(-0.004, 0.004, size=(4, D)) / np.sqrt(D)))
    for W in (3, 6, 7):
        lists.append(("W%d" % W, rng.uniform(-2, 2, size=(W, D))))
    cases = [dict(label="%s/r%g" % (name, r), waypoints=_rows(w), rounding=r) for name, w in lists for r in FIT_ROUNDINGS]
    cases.append(dict(label="W0", waypoints=[], rounding=0.2))
    return cases


def make_velocity_cases(D):
    """Trajectories and query times for GetVelocityAtTime: on a sample, between samples, the
    first and the last sample, before and after the trajectory, no samples, one sample."""
    rng = np.random.default_rng(59 * D + 3)
    cases = []
    for n in (0, 1, 2, 5, 33):
        t = (np.round((2.0 + np.cumsum(rng.uniform(0.001, 0.01, size=n))) * 1e9) / 1e9).tolist()
        v = _rows(rng.uniform(-1.5, 1.5, size=(n, D))) if n else []
        if n == 0:
            queries = [("no_samples", 1.0)]
        else:
            i = int(rng.integers(0, n))
            queries = [("on_sample", t[i]), ("first", t[0]), ("last", t[-1]), ("before", t[0] - 1e-6), ("after", t[-1] + 1e-6)]
            if n > 1:
                j = int(rng.integers(0, n - 1))
                queries += [("between", 0.5 * (t[j] + t[j + 1])), ("inside", t[0] + float(rng.uniform(0, 1)) * (t[-1] - t[0]))]
        cases += [dict(label=k, time=t, velocity=v, query=float(q)) for k, q in queries]
    return cases

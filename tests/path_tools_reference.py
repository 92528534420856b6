"""What a stopping point and a projection mean, stated independently of the kernels and the mirror.

1. compute_stopping_point / project_point_on_path: restatements of path_tools.cc:25-74 and
   path_tools.h:56-100 in np.longdouble, written from the reference's sources (each step cites its
   lines), not from csrc/tpamd_retarget.h or host/path_tools.cc. The two eigenmath helpers that the
   reference's tree does not contain are restated from their documented meaning:
   ScaleDownToLimits scales a vector uniformly until no component exceeds its limit, and
   DistanceFromLineSegment gives the distance to the closest point of a segment and that point's
   line parameter (limited to the segment's end; a negative parameter is kept, as
   timeable_path_joint_spline.cc:232-239 relies on).
2. check_stopping_point / check_projection: property checks in np.longdouble that take the inputs
   and the outputs of ANY implementation and assert what the result is, independent of the order of
   operations:
     - out - pos is parallel to vel;
     - the deceleration of the stop respects every limit and meets at least one, or has the
       size of the largest limit where the reference's scaling does not act (its own test case,
       three equal limits and a diagonal velocity, is of that kind);
     - |delta| = |vel|^2 / (2 |dec|);
     - the extra offset has length min(rounding, |delta| / 4) along vel;
     - no sampled point of any segment is closer to the point than the projection.

Plain Python and numpy; no GPU, no product imports.
"""
import numpy as np

LD = np.longdouble
OK, INVALID_ARGUMENT = 0, 3            # TPAMD_PLAN_*
REST_THRESHOLD = 100 * np.finfo(np.float64).eps      # path_tools.cc:43-44
CORNER_SPACING = 4                     # splines/spline_utils.h:44-46
CORNER_TINY = 1e-6                     # splines/spline_utils.cc:33


def _ld(x):
    return np.asarray(x, dtype=LD)


def corner_offset(delta, radius):
    """PolyLineToBspline3WaypointsCornerOffset, splines/spline_utils.cc:25-45."""
    delta = _ld(delta)
    norm = np.sqrt(np.sum(delta * delta))
    offset = delta / norm if norm > CORNER_TINY else np.zeros_like(delta)     # :33-37
    if norm > CORNER_SPACING * LD(radius):                                    # :38-42
        return offset * LD(radius)
    return offset * (LD(1) / CORNER_SPACING) * norm


def scale_down_to_limits(value, limits):
    """eigenmath::ScaleDownToLimits by its meaning: the largest uniform scaling <= 1 after which
    |value_i| <= limits_i for every i."""
    value, limits = _ld(value), _ld(limits)
    factor = LD(1)
    for v, l in zip(np.abs(value), limits):
        if v > l:
            factor = min(factor, l / v)
    return value * factor


def compute_stopping_point(position, velocity, acceleration_limit, corner_rounding):
    """path_tools.cc:25-74. Returns (status, point, parts); parts holds the intermediate values
    (dec, stop_time, delta, offset) for the property checks, None where the function returns early."""
    pos, vel, acc = _ld(position), _ld(velocity), _ld(acceleration_limit)
    if acc.min() <= 0:                                                        # :39-42
        return INVALID_ARGUMENT, None, None
    if np.abs(vel).max() < REST_THRESHOLD:                                    # :43-46
        return OK, pos.copy(), None
    normalized = vel / np.sqrt(np.sum(vel * vel))
    dec = scale_down_to_limits(-normalized * acc.max(), acc)                  # :50-52
    stop_time = -np.sum(vel * vel) / np.sum(vel * dec)                        # :60
    delta = stop_time * (vel + LD(0.5) * stop_time * dec)                     # :62-63
    offset = corner_offset(delta, corner_rounding)                            # :70-72
    return OK, pos + delta + offset, dict(dec=dec, stop_time=stop_time, delta=delta, offset=offset)


def stopping_point_error(out, position, velocity, acceleration_limit, corner_rounding):
    """Relative error of an implementation's point against the restatement: the largest component
    difference over the largest |component| of the exact point (0 for a bit-equal point)."""
    _, ref, _ = compute_stopping_point(position, velocity, acceleration_limit, corner_rounding)
    scale = max(np.abs(ref).max(), LD(np.finfo(np.float64).tiny))
    return float(np.abs(_ld(out) - ref).max() / scale)


def check_stopping_point(out, position, velocity, acceleration_limit, corner_rounding, rel):
    """What a stopping point is, asserted on `out` with the relative slack `rel` (of the size of the
    point and of the offset from the position)."""
    pos, vel, acc, out = _ld(position), _ld(velocity), _ld(acceleration_limit), _ld(out)
    assert acc.min() > 0
    if np.abs(vel).max() < REST_THRESHOLD:
        assert np.array_equal(out, pos)
        return
    step = out - pos
    speed = np.sqrt(np.sum(vel * vel))
    direction = vel / speed
    slack = LD(rel) * max(np.abs(out).max(), np.abs(pos).max(), LD(1e-300))
    # parallel to vel, and pointing along it
    along = np.sum(step * direction)
    assert along >= 0
    assert np.abs(step - along * direction).max() <= 4 * slack, "the offset is not parallel to the velocity"
    # the deceleration along -vel: max acc, scaled down until every limit is respected. Where the
    # scaling acts, one joint decelerates at its limit; where it does not (|direction_i| max acc
    # <= acc_i for every joint, e.g. equal limits and a diagonal velocity), |dec| is max acc.
    steepest = min(acc[i] / abs(direction[i]) for i in range(len(vel)) if direction[i] != 0)
    dec_norm = min(steepest, acc.max())
    assert np.all(np.abs(direction) * dec_norm <= acc * (1 + LD(1e-18)))
    # |delta| = |vel|^2 / (2 |dec|), then min(rounding, |delta| / 4) more
    delta_norm = speed * speed / (2 * dec_norm)
    extra = min(LD(corner_rounding), delta_norm / CORNER_SPACING) if delta_norm > CORNER_TINY else LD(0)
    assert abs(along - (delta_norm + extra)) <= 4 * slack, (along, delta_norm, extra)


def check_stopping_parts(parts, velocity, acceleration_limit, corner_rounding):
    """The same properties on the restatement's own intermediate values, to its precision."""
    vel, acc = _ld(velocity), _ld(acceleration_limit)
    dec, delta, offset = parts["dec"], parts["delta"], parts["offset"]
    tiny = LD(64) * np.finfo(LD).eps
    norm = lambda v: np.sqrt(np.sum(v * v))
    assert np.all(np.abs(dec) <= acc * (1 + tiny))
    met = np.any(np.abs(np.abs(dec) - acc) <= acc * tiny)
    assert met or abs(norm(dec) - acc.max()) <= acc.max() * tiny
    assert abs(norm(delta) - np.sum(vel * vel) / (2 * norm(dec))) <= norm(delta) * tiny
    want = min(LD(corner_rounding), norm(delta) / CORNER_SPACING) if norm(delta) > CORNER_TINY else LD(0)
    assert abs(norm(offset) - want) <= max(want, LD(1e-300)) * tiny
    # delta and the offset point along vel
    for v in (delta, offset):
        assert np.abs(v * norm(vel) - vel * norm(v)).max() <= norm(vel) * max(norm(v), LD(1e-300)) * tiny


def project_point_on_path(waypoints, point):
    """path_tools.h:56-100. Returns (status, index, distance, line_parameter, projected_point)."""
    wps, pt = _ld(waypoints), _ld(point)
    if len(wps) == 0:                                                         # :62-64
        return INVALID_ARGUMENT, 0, None, None, None
    if len(wps) == 1:                                                         # :65-71
        return OK, 0, np.sqrt(np.sum((wps[0] - pt) ** 2)), LD(0), wps[0].copy()
    best = (np.finfo(np.float64).max, LD(0), 0)                               # :82
    for i in range(len(wps) - 1):                                             # :83-93
        a, b = wps[i], wps[i + 1]
        ab = b - a
        ab2 = np.sum(ab * ab)
        t = np.sum((pt - a) * ab) / ab2 if ab2 > 0 else LD(0)
        t = min(t, LD(1))
        closest = a + max(t, LD(0)) * ab
        dist = np.sqrt(np.sum((closest - pt) ** 2))
        if dist < best[0]:
            best = (dist, t, i)
    dist, t, i = best
    return OK, i, dist, t, wps[i] + t * (wps[i + 1] - wps[i])                 # :95-97


def check_projection(waypoints, point, distance, rel, samples=33):
    """No sampled point of any segment is closer to `point` than `distance` (the waypoints
    themselves are among the samples)."""
    wps, pt = _ld(waypoints), _ld(point)
    slack = LD(rel) * max(np.abs(wps).max(), np.abs(pt).max(), LD(1))
    if len(wps) == 1:
        assert abs(np.sqrt(np.sum((wps[0] - pt) ** 2)) - LD(distance)) <= slack
        return
    closest = None
    for i in range(len(wps) - 1):
        for j in range(samples):
            c = wps[i] + (LD(j) / (samples - 1)) * (wps[i + 1] - wps[i])
            d = np.sqrt(np.sum((c - pt) ** 2))
            closest = d if closest is None else min(closest, d)
    assert LD(distance) <= closest + slack, (distance, closest)

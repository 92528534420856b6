"""What a stop means, stated twice and independently of the kernels.

1. A restatement of the backward stop in Python floats (IEEE doubles), every operation in the
   reference's order: RescaleTrajectoryBackwardToStop (rescale_to_stop.cc) under
   TrajectoryBuffer::StopAtIndex / StopBeforeTime and InsertSegment's kept count
   (trajectory_buffer.cc). Each function cites the lines it follows. It is written from those
   sources, not from csrc/tpamd_rescale.h or host/*.cc, so that a shared misreading of the
   reference in kernel and mirror does not pass. The forward stop (GetPathStopParameter) already
   has such a restatement: fastest_stop_at_time in tests/test_fastest_stop_cpu.py.
2. Property checkers in np.longdouble (check_stop_segment, check_fastest_stop) that take the
   inputs and the outputs of ANY implementation and assert what a stop is: one common scaling
   rate per row, the rate recurrence, the limits, that the deceleration is the steepest
   admissible one (a brute-force pass over the 2 D candidates), the rescaled time steps, the
   time shift and the kept count. They do not depend on the order of operations.
3. Closed forms for a constant velocity, and the case generators the CPU and GPU tests share.

Two documented deviations from the reference, both TPAMD_PLAN_INTERNAL with nothing changed:
sample `index` at rest before the end (the reference aborts on an empty rescaling), and a rest
sample without an admissible deceleration (the first rescaled step is 2 dt / 0 and the reference
goes on to insert a segment whose times are NaN).

Plain Python and numpy; no GPU, no product imports.
"""
import math

import numpy as np

from test_fastest_stop_cpu import fastest_stop_at_time, synthetic_row

OK, OUT_OF_RANGE, INVALID_ARGUMENT, INTERNAL, NOT_FOUND = 0, 2, 3, 4, 6   # TPAMD_PLAN_*
FAILED_PRECONDITION = 1
STATUS_NAMES = {OK: "ok", OUT_OF_RANGE: "out_of_range", INVALID_ARGUMENT: "invalid_argument",
                INTERNAL: "internal", NOT_FOUND: "not_found"}
BACKWARD_SLACK = 1e-8      # rescale_to_stop.cc:93 kTiny, the validity slack and the velocity cut
FORWARD_SLACK = 1e-10      # path_timing_trajectory.cc ComputeFastestStop's validity slack
FORWARD_CUT = 1e-6         # ... and its velocity cut
TIMESTEP_TOLERANCE = 1e-6  # trajectory_buffer.h TrajectoryBufferOptions::timestep_tolerance


def stop_group_lanes(D):
    """Lanes of the group that serves one trajectory in the lane-group kernels: next_pow2(2 D)."""
    l = 2
    while l < 2 * D:
        l *= 2
    return l


# ------------------------------------------------------------------ A1: the restatement
def inputs_valid(times):
    """AreInputsValidForSampledTrajectory, sampled_trajectory.cc:24-45 (the sizes agree by
    construction here): at least two samples, times strictly increasing."""
    if len(times) < 2:                                     # :29-31
        return False
    for i in range(len(times) - 1):                        # :37-42
        if times[i + 1] <= times[i]:
            return False
    return True


def rescale_backward_to_stop(amax, times, qd, qdd, trace=None):
    """RescaleTrajectoryBackwardToStop, rescale_to_stop.cc:33-162, on times[n], qd / qdd [n][D]
    (lists of Python floats). Returns ("invalid", None), ("empty", None) or ("ok", (t, v, a)) with
    the rescaled rows in forward order; they pair with input rows [n - len(t), n - 1].
    `trace`, if a list, receives one dict per backward step (what the step met; for the outcome
    counters only, nothing of it flows into the result)."""
    if not inputs_valid(times):                            # :54-58
        return "invalid", None
    if max(abs(x) for x in qd[-1]) < 1e-8:                 # :62-65
        return "empty", None
    D, n = len(amax), len(times)                           # :69-70
    r_t, r_v, r_a = [0.0], [[0.0] * D], [[0.0] * D]        # :76-78
    rate2 = 0.0                                            # :80
    for i in range(n - 1, 1, -1):                          # :82
        bias = [a * rate2 for a in qdd[i]]                 # :90
        v = qd[i]                                          # :91
        d = 0.0                                            # :92
        seen = []
        for joint in range(D):                             # :99
            if abs(v[joint]) < 1e-8:                       # :100-102
                continue
            for sign in (-1.0, 1.0):                       # :103
                dj = -2.0 * (bias[joint] + sign * amax[joint]) / v[joint]          # :104-106
                scaled = [bias[j] + 0.5 * v[j] * dj for j in range(D)]             # :107-108
                valid = (min(amax[j] - scaled[j] for j in range(D)) >= -1e-8 and   # :109-111
                         max(-amax[j] - scaled[j] for j in range(D)) <= 1e-8)
                if trace is not None:
                    margin = min(min(amax[j] - scaled[j], scaled[j] + amax[j]) for j in range(D))
                    seen.append((dj, valid, margin))
                if valid and dj < d:                       # :112-114
                    d = dj
        udt = times[i] - times[i - 1]                      # :117
        nxt = rate2 - d * udt                              # :118-119
        clamped = 1.0 if 1.0 < nxt else nxt                # :122 std::min(next, 1.0)
        den = math.sqrt(rate2) + math.sqrt(clamped)        # :124-126
        new_dt = 2.0 * udt / den if den != 0.0 else math.inf   # IEEE x / 0 (udt > 0 here)
        r_t.append(r_t[-1] - new_dt)                       # :127
        root = math.sqrt(clamped)
        r_v.append([root * x for x in v])                  # :128
        r_a.append([bias[j] + 0.5 * v[j] * d for j in range(D)])   # :129-130
        if trace is not None:
            trace.append(dict(i=i, d=d, rate2=rate2, next=nxt, cands=seen,
                              under_cut=sum(1 for x in v if abs(x) < 1e-8)))
        if nxt >= 1.0:                                     # :132-134
            break
        rate2 = nxt                                        # :135
    r_t.reverse()                                          # :139-141
    r_v.reverse()
    r_a.reverse()
    switch_index = n - len(r_t)                            # :144
    time_offset = times[switch_index] - r_t[0]             # :149-150
    r_t = [t + time_offset for t in r_t]                   # :152-154
    return "ok", (r_t, r_v, r_a)


def offset_bracket(times, time_sec):
    """GetOffsetBracket, trajectory_buffer.cc:233-251: (status, lower, upper)."""
    n = len(times)
    if n == 0:                                             # :235-237
        return FAILED_PRECONDITION, 0, 0
    if time_sec < times[0] or time_sec > times[-1]:        # :238-242
        return OUT_OF_RANGE, 0, 0
    u = 0                                                  # :244 upper_bound
    while u < n and not (time_sec < times[u]):
        u += 1
    if u == n:                                             # :245-247
        return OK, n - 1, n - 1
    return OK, u - 1, u                                    # :248-250


def velocity_at_time(times, qd, time_sec):
    """GetVelocityAtTime, trajectory_buffer.cc:269-278: (status, velocity). The linear
    interpolation is written a + f (b - a), f = (t - t_l) / (t_u - t_l); it only feeds the 1e-2
    match below. On the last sample (l == u) the reference interpolates between two equal times,
    whose value its sources here do not pin; it is taken as that sample (reached by a stop at
    index 1 of two samples)."""
    st, l, u = offset_bracket(times, time_sec)
    if st != OK:
        return st, None
    if l == u:
        return OK, list(qd[l])
    f = (time_sec - times[l]) / (times[u] - times[l])
    return OK, [a + f * (b - a) for a, b in zip(qd[l], qd[u])]


def insert_segment_kept(times, front, tolerance=TIMESTEP_TOLERANCE):
    """InsertSegment's kept count for a non-empty segment that starts at `front`,
    trajectory_buffer.cc:102-120: (samples_to_keep, replaced), replaced: the segment replaces
    the whole buffer and the sequence number goes back to 0 (:106-113)."""
    n = len(times)
    it = 0                                                 # :103-105 upper_bound with a <= b
    while it < n and not (front <= times[it]):
        it += 1
    if n == 0 or it == 0:                                  # :106
        return 0, True
    if front - times[it - 1] < tolerance:                  # :117-119
        it -= 1
    return it, False                                       # :120


def _result(status, n, keep=None, first=None, last=None, t=(), v=(), a=(), replaced=False, inserted=False):
    """A stop as tpamd_stop_trajectories_* reports it (include/tpamd.h): a failed stop has
    keep = count and an empty segment first = count, last = count - 1."""
    if keep is None:
        keep, first, last = n, n, n - 1
    return dict(status=status, keep=keep, first=first, last=last, time=list(t), qd=[list(r) for r in v],
                qdd=[list(r) for r in a], replaced=replaced, inserted=inserted)


def stop_at_index(time, qd, qdd, amax, time_step, index, tolerance=TIMESTEP_TOLERANCE, trace=None):
    """TrajectoryBuffer::StopAtIndex, trajectory_buffer.cc:296-362, on a buffer holding the rows
    time[n], qd / qdd [n][D]. Returns status, keep, first, last and rows [first, last] of time,
    qd, qdd; `inserted`: InsertSegment ran (the sequence number moves), `replaced`: it replaced
    the whole buffer."""
    n = len(time)
    if index <= 0 or index > n - 1:                        # :299-303
        return _result(OUT_OF_RANGE, n)
    if min(amax) <= 0.0:                                   # :305-309
        return _result(INVALID_ARGUMENT, n)
    if time_step <= 0.0:                                   # :311-314
        return _result(INVALID_ARGUMENT, n)
    D = len(amax)
    if index == n - 1 and max(abs(x) for x in qd[-1]) < 1e-4:      # :316-322
        return _result(OK, n, n - 1, n - 1, n - 1, [time[-1]], [[0.0] * D], [[0.0] * D])
    m1 = index + 1                                         # :324-336
    what, seg = rescale_backward_to_stop(amax, time[:m1], qd[:m1], qdd[:m1], trace)
    if what == "invalid":                                  # :337-339
        return _result(INVALID_ARGUMENT, n)
    if what == "empty":                                    # :342 CHECK: the reference aborts
        return _result(INTERNAL, n)
    seg_t, seg_v, seg_a = seg
    if not math.isfinite(seg_t[0]):                        # the second deviation (module docstring)
        return _result(INTERNAL, n)
    if len(seg_t) == index:                                # :346
        st, vel = velocity_at_time(time, qd, seg_t[0])     # :347-351
        if st != OK:
            return _result(st, n)
        if max(abs(a - b) for a, b in zip(vel, seg_v[0])) > 1e-2:   # :353-358
            return _result(NOT_FOUND, n)
    keep, replaced = insert_segment_kept(time, seg_t[0], tolerance)    # :360-361
    return _result(OK, n, keep, index + 1 - len(seg_t), index, seg_t, seg_v, seg_a, replaced, True)


def stop_before_time(time, qd, qdd, amax, time_step, time_sec, tolerance=TIMESTEP_TOLERANCE, trace=None):
    """TrajectoryBuffer::StopBeforeTime, trajectory_buffer.cc:370-385. No samples: OK, keep 0 and
    an empty segment (first 0, last -1)."""
    n = len(time)
    if n == 0:                                             # :373-375
        return _result(OK, 0, 0, 0, -1)
    if time_sec < time[0]:                                 # :376-378
        return _result(OUT_OF_RANGE, n)
    lower = 0                                              # :381 lower_bound
    while lower < n and time[lower] < time_sec:
        lower += 1
    index = min(lower + 1, n - 1)                          # :382-383
    return stop_at_index(time, qd, qdd, amax, time_step, index, tolerance, trace)   # :384


def stopped_buffer(time, q, qd, qdd, res):
    """The buffer after the stop: input[0, keep) ++ segment (positions of the segment are the
    input's rows [first, last], rescale_to_stop.cc:147-148)."""
    k, f, l = res["keep"], res["first"], res["last"]
    return (list(time[:k]) + list(res["time"]), [list(r) for r in q[:k]] + [list(r) for r in q[f:l + 1]],
            [list(r) for r in qd[:k]] + res["qd"], [list(r) for r in qdd[:k]] + res["qdd"])


# ------------------------------------------------------------------ A2: the property checkers
LD = np.longdouble

# The largest residual of each identity below on the restatements' own fp64 outputs, evaluated in
# long double over make_batch(D), D = 1..16 (rounded up to two digits; DESIGN.md section 2;
# tests/test_stop_reference_cpu.py measures them again and asserts these figures). The checkers'
# rounding tolerances are 16 x these.
MEASURED_RESIDUALS = {
    "rho": 2.1e-16,        # joints' rates against each other, relative; a rate smaller than the row behind it
    "rate": 4.9e-16,       # next - rate2 + d dt, relative to max(1, |d dt|, |2 bias / v| dt)
    "d": 9.7e-15,          # recovered d against the brute-force minimum, relative to max(1, |d|, |2 bias / v|)
    "limit": 4.3e-16,      # beyond amax + slack, and the limiting joint off its limit, relative to max(1, amax)
    "dt": 2.2e-16,         # rescaled time step, relative to the largest |time| of the segment
    "start": 2.0e-16,      # the segment's first time against time_in[first], same scale
    "fs_next": 6.8e-17,    # forward: next - max(0, rate2 + dt d), absolute (rate2 <= 1)
    "fs_d": 1.2e-14,       # forward: d against the brute-force minimum, relative to max(1, |d|)
    "fs_time": 7.2e-16,    # forward: profile time and duration, relative to max(|t0|, duration)
}
TOLERANCES = {k: 16 * v for k, v in MEASURED_RESIDUALS.items()}
AMBIGUITY_MARGIN = 1e-12        # a validity test this close to its threshold is not judged


class StopCheckError(AssertionError):
    pass


def _need(cond, what, *info):
    if not cond:
        raise StopCheckError("%s %s" % (what, info if info else ""))


def _resid(residuals, key, value, tol):
    value = float(value)
    if residuals is not None:
        residuals[key] = max(residuals.get(key, 0.0), value)
    _need(value <= tol[key], "residual of '%s' above its tolerance" % key, value, tol[key])


def steepest_admissible(v, acc, amax, rate2, cut, slack):
    """Brute force over the 2 D candidates in long double: (d, ambiguous). d = min(0, smallest
    valid candidate); ambiguous if some candidate's validity lies within AMBIGUITY_MARGIN of the
    slack, or a candidate within the margin of 0 decides."""
    v, acc, amax = (np.asarray(x, dtype=LD) for x in (v, acc, amax))
    bias = acc * LD(rate2)
    moving = np.abs(v) >= LD(cut)
    if not moving.any():
        return LD(0), False
    vm, bm, am = v[moving], bias[moving], amax[moving]
    dc = np.concatenate([LD(2) * (-bm - am) / vm, LD(2) * (-bm + am) / vm])
    s = bias[None, :] + LD(0.5) * v[None, :] * dc[:, None]
    margin = np.minimum(amax[None, :] - s, s + amax[None, :]).min(axis=1) + LD(slack)
    ambiguous = bool((np.abs(margin) < AMBIGUITY_MARGIN).any())
    ok = (margin >= 0) & (dc < 0)
    return (dc[ok].min() if ok.any() else LD(0)), ambiguous


def _lacks_room(t_in, v_in, a_in, am, index):
    """The backward integration from `index` in long double, for a stop reported NOT_FOUND: True
    if the rate stays below 1 down to sample 2 and the velocity there misses the trajectory's by
    more than 1e-2, False if not, None if a step is ambiguous or a bound is met within 1e-9."""
    rate2, vf = LD(0), np.zeros_like(v_in[index])
    for i in range(index, 1, -1):
        d, ambiguous = steepest_admissible(v_in[i], a_in[i], am, rate2, BACKWARD_SLACK, BACKWARD_SLACK)
        nxt = rate2 - d * (t_in[i] - t_in[i - 1])
        if ambiguous or abs(nxt - 1) < 1e-9:
            return None
        if nxt >= 1 and i > 2:
            return False                           # reaches 1 with samples to spare: no match is asked
        vf = np.sqrt(min(nxt, LD(1))) * v_in[i]
        rate2 = nxt
    err = float(np.abs(v_in[1] - vf).max())    # the segment starts at sample 1, up to rounding
    return None if abs(err - 1e-2) < 1e-9 else err > 1e-2


def check_stop_segment(time, qd, qdd, amax, time_step, res, index=None, stop_time=None,
                       tolerance=TIMESTEP_TOLERANCE, tol=TOLERANCES, residuals=None, stats=None):
    """Asserts that `res` (status, keep, first, last, time / qd / qdd rows [first, last], from any
    implementation) is the stop of the trajectory time[n], qd / qdd [n][D] at sample `index`, or
    before `stop_time`. Raises StopCheckError. stats (dict) counts steps and ambiguous steps."""
    n, D = len(time), len(amax)
    t_in = np.asarray(time, dtype=LD)
    v_in = np.asarray(qd, dtype=LD).reshape(n, D)
    a_in = np.asarray(qdd, dtype=LD).reshape(n, D)
    am = np.asarray(amax, dtype=LD)
    st, keep, first, last = res["status"], res["keep"], res["first"], res["last"]
    if index is None:
        if n == 0:
            _need((st, keep, first, last) == (OK, 0, 0, -1), "an empty trajectory stops OK with nothing")
            return
        if stop_time < time[0]:
            _need(st == OUT_OF_RANGE, "a stop before the first sample is out of range")
            index = None
        else:
            index = min(int(np.searchsorted(np.asarray(time, dtype=np.float64), stop_time, side="left")) + 1, n - 1)
    if st != OK:
        _need((keep, first, last) == (n, n, n - 1), "a failed stop keeps everything", keep, first, last)
        if index is None:
            return
        if index <= 0 or index > n - 1:
            _need(st == OUT_OF_RANGE, "index outside [1, n - 1] is out of range", st)
        elif min(amax) <= 0.0 or time_step <= 0.0:
            _need(st == INVALID_ARGUMENT, "bad limits or time step are invalid arguments", st)
        elif not bool((np.diff(t_in[:index + 1]) > 0).all()):
            _need(st == INVALID_ARGUMENT, "times must increase up to the stop sample", st)
        elif float(np.abs(v_in[index]).max()) < 1e-8:
            _need(st == INTERNAL, "a rest sample before the end has no stop", st)
        else:
            _need(st in (NOT_FOUND, INTERNAL), "a well-posed stop fails only for lack of room", st)
            if st == INTERNAL:
                d0, _ = steepest_admissible(v_in[index], a_in[index], am, 0, BACKWARD_SLACK, BACKWARD_SLACK)
                _need(d0 == 0, "INTERNAL needs a rest sample without an admissible deceleration")
            else:
                _need(_lacks_room(t_in, v_in, a_in, am, index) is not False,
                      "NOT_FOUND needs a stop that uses every sample and misses the velocity there")
        return
    _need(index is not None and 1 <= index <= n - 1 and min(amax) > 0.0 and time_step > 0.0,
          "OK needs a valid index and arguments", index)
    _need(last == index, "the segment ends on the stop sample", last, index)
    o_t = np.asarray(res["time"], dtype=LD)
    o_v = np.asarray(res["qd"], dtype=LD).reshape(-1, D)
    o_a = np.asarray(res["qdd"], dtype=LD).reshape(-1, D)
    m = last - first + 1
    _need(m >= 1 and len(o_t) == m and o_v.shape[0] == m and o_a.shape[0] == m, "rows [first, last]", first, last)
    _need(not o_v[-1].any() and not o_a[-1].any(), "the rest row has qd = qdd = 0 exactly")
    if index == n - 1 and float(np.abs(v_in[-1]).max()) < 1e-4:
        _need(m == 1 and keep == n - 1 and o_t[0] == t_in[-1], "rest on the last sample changes that sample only")
        return
    _need(first >= 1 and (m >= 2 or index == 1), "a stop never uses sample 0 and, but at index 1, has a scaled row",
          first, last)
    _need(bool((np.diff(t_in[:index + 1]) > 0).all()), "OK needs increasing times")
    scale_t = max(float(np.abs(o_t).max()), float(o_t[-1] - o_t[0]), 1e-300)
    _need(bool((np.diff(o_t) > 0).all()), "segment times increase strictly")
    _need(bool(np.isfinite(o_t.astype(np.float64)).all()), "segment times are finite")
    # rows, backward from the rest row: step i uses sample i and writes row r = i - 1 - first. One
    # rate rho per row, taken from the joint that moves most; a sample that does not move at all
    # has no candidate, so d = 0 and the rate stays.
    rho = np.zeros(m, dtype=LD)
    for i in range(index, first, -1):
        r = i - 1 - first
        src, acc = v_in[i], a_in[i]
        rate2 = rho[r + 1] ** 2
        j = int(np.argmax(np.abs(src)))
        nz = src != 0
        _need(not o_v[r][~nz].any(), "a joint at rest stays at rest")
        if nz.any():
            rho[r] = o_v[r, j] / src[j]
            _resid(residuals, "rho", np.abs(o_v[r][nz] / src[nz] - rho[r]).max() / max(float(rho[r]), 1e-300), tol)
            d = LD(2) * (o_a[r, j] - acc[j] * rate2) / src[j]
            d_scale = max(1.0, float(abs(2 * acc[j] * rate2 / src[j])))
        else:
            rho[r], d, d_scale = rho[r + 1], LD(0), 1.0
        _need(0 < rho[r] <= 1, "0 < rate <= 1", float(rho[r]))
        _resid(residuals, "rho", max(0.0, float(rho[r + 1] - rho[r])), tol)     # never smaller towards the front
        _resid(residuals, "d", max(0.0, float(d)) / d_scale, tol)               # d <= 0
        dt = t_in[i] - t_in[i - 1]
        nxt = rate2 - d * dt
        if r == 0 and rho[0] == 1:
            _need(nxt >= 1 - tol["rate"] * max(1.0, float(abs(d * dt))), "the first row is where the rate reaches 1")
        else:
            _resid(residuals, "rate", abs(nxt - rho[r] ** 2) / max(1.0, float(abs(d * dt)), d_scale * float(dt)), tol)
        s = acc * rate2 + LD(0.5) * src * d
        _resid(residuals, "d", float(np.abs(o_a[r] - s).max() / max(1.0, float(np.abs(s).max()))), tol)
        want, ambiguous = steepest_admissible(src, acc, am, rate2, BACKWARD_SLACK, BACKWARD_SLACK)
        if stats is not None:
            stats["steps"] = stats.get("steps", 0) + 1
            stats["ambiguous"] = stats.get("ambiguous", 0) + int(ambiguous)
        if not ambiguous:
            _resid(residuals, "d", float(abs(d - want)) / max(d_scale, float(abs(want))), tol)
            if want != 0:
                # a valid candidate was chosen: every joint within its limit, a moving one on it.
                # (With d = 0 the accelerations are the input's own, scaled by rate2; the reference
                # does not bound them, and neither does this check.)
                _resid(residuals, "limit", max(0.0, float(((np.abs(o_a[r]) - am - LD(BACKWARD_SLACK)) / np.maximum(am, 1)).max())), tol)
                moving = np.abs(src) >= LD(BACKWARD_SLACK)
                _resid(residuals, "limit", float((np.abs(np.abs(o_a[r]) - am) / np.maximum(am, 1))[moving].min()), tol)
        _resid(residuals, "dt", float(abs((o_t[r + 1] - o_t[r]) - LD(2) * dt / (rho[r + 1] + rho[r])) / scale_t), tol)
    if first > 1:
        _need(rho[0] == 1, "the segment starts at the trajectory's own velocity", float(rho[0]))
    front = o_t[0]
    _resid(residuals, "start", float(abs(front - t_in[first]) / scale_t), tol)
    # InsertSegment's kept count, either branch of trajectory_buffer.cc:117-119
    _need(0 <= keep <= n, "keep in range", keep)
    plain = ((keep == 0 or (t_in[keep - 1] < front and front - t_in[keep - 1] >= LD(tolerance))) and
             (keep == n or t_in[keep] >= front))
    replaced = keep < n and t_in[keep] < front and front - t_in[keep] < LD(tolerance) and \
        (keep + 1 == n or t_in[keep + 1] >= front)
    _need(plain or replaced, "keep is InsertSegment's kept count", keep, float(front))
    if first == 1:
        _, l, u = offset_bracket([float(x) for x in time], float(front))
        f = (front - t_in[l]) / (t_in[u] - t_in[l]) if l != u else LD(0)
        _need(float(np.abs(v_in[l] + f * (v_in[u] - v_in[l]) - o_v[0]).max()) <= 1e-2,
              "a stop that uses every sample matches the velocity there")


def check_fastest_stop(time, s, qd, qdd, amax, query, res, tol=TOLERANCES, residuals=None, stats=None):
    """Asserts that `res` (status, stop_parameter, stop_index, duration and the profile lists
    time, rate2, drate2, from any implementation) is GetPathStopParameter(query) on the row."""
    n, D = len(time), len(amax)
    st, sp, idx, dur = res["status"], res["stop_parameter"], res["stop_index"], res["duration"]
    lo = int(np.searchsorted(np.asarray(time, dtype=np.float64), query, side="left")) if n else 0
    if lo >= n:
        _need((st, sp, idx, dur) == (INVALID_ARGUMENT, 0.0, -1, 0.0), "no sample at or after the query", st, idx)
        return
    _need(st == OK, "a query within the row is OK", st)
    pt, pr, pd = (np.asarray(res[k], dtype=LD) for k in ("time", "rate2", "drate2"))
    m = len(pr)
    _need(m >= 1 and len(pt) == m and len(pd) == m and idx == lo + m - 1 and idx <= n - 1, "profile length", m, idx)
    _need(sp == s[idx], "the stop parameter is s at the stop sample")
    _need(pr[0] == 1 and bool((np.diff(pr) <= 0).all()) and bool((pr[:-1] > 0).all()) and bool((pr >= 0).all()),
          "rate2 goes from 1, never increases and is positive before the stop sample")
    _need(pr[-1] == 0 or idx == n - 1, "the stop is where rate2 reached 0, or the last sample")
    _need(bool((pd <= 0).all()) and pd[-1] == (pd[-2] if m > 1 else 0), "d <= 0; the last entry repeats")
    t_in = np.asarray(time, dtype=LD)
    am = np.asarray(amax, dtype=LD)
    elapsed = LD(0)
    scale = max(abs(float(t_in[lo])), float(dur), 1e-300)
    for k in range(m - 1):
        i = lo + k
        dt = t_in[i + 1] - t_in[i]
        _resid(residuals, "fs_time", float(abs(pt[k] - (t_in[lo] + elapsed)) / scale), tol)
        x = pr[k] + dt * pd[k]
        _resid(residuals, "fs_next", float(abs(pr[k + 1] - (x if x > 0 else LD(0)))), tol)
        want, ambiguous = steepest_admissible(qd[i], qdd[i], am, pr[k], FORWARD_CUT, FORWARD_SLACK)
        if stats is not None:
            stats["steps"] = stats.get("steps", 0) + 1
            stats["ambiguous"] = stats.get("ambiguous", 0) + int(ambiguous)
        if not ambiguous:
            _resid(residuals, "fs_d", float(abs(pd[k] - want) / max(1.0, float(abs(want)))), tol)
        elapsed += LD(2) * dt / (np.sqrt(pr[k]) + np.sqrt(pr[k + 1]))
    _resid(residuals, "fs_time", float(abs(pt[m - 1] - (t_in[lo] + elapsed)) / scale), tol)
    _resid(residuals, "fs_time", float(abs(LD(dur) - elapsed) / scale), tol)


def fastest_stop_result(time, s, qd, qdd, amax, query):
    """fastest_stop_at_time as the dict check_fastest_stop takes."""
    st, sp, idx, dur, pt, pr, pd = fastest_stop_at_time(time, s, qd, qdd, amax, query)
    return dict(status=st, stop_parameter=sp, stop_index=idx, duration=dur, time=pt, rate2=pr, drate2=pd)


# ------------------------------------------------------------------ A3: closed forms
def constant_velocity_case(D, K=64, v=1.0, a=2.0, extra=9, sign=1.0):
    """Constant velocity sign * v c_j, zero acceleration, limits a c_j (c_j powers of two, so the
    D joints give the same candidates exactly), uniform dt with eps = 2 a dt / v = 1 / K. With
    K a power of two every rate k eps is exact. Returns the row and (K, dt, v / a)."""
    dt = v / (2.0 * a * K)
    n = K + 1 + extra
    c = [2.0 ** (j % 4 - 1) for j in range(D)]
    time = [0.5 + i * dt for i in range(n)]
    row = dict(time=time, s=[i * dt * v for i in range(n)], q=[[sign * v * cj * i * dt for cj in c] for i in range(n)],
               qd=[[sign * v * cj for cj in c] for _ in range(n)], qdd=[[0.0] * D for _ in range(n)],
               amax=[a * cj for cj in c], label="closed_form")
    return row, (K, dt, v / a)


def check_closed_forms(row, K, dt, duration, backward, forward, tol=TOLERANCES):
    """The backward stop at the last sample has K + 1 rows, qdd_out = -a sign(v) on every joint
    (all are limiting), rates sqrt(k eps) and lasts v / a; the forward stop from the first sample
    ends K samples on after v / a. This pins the factor 2 in d and the pairing of rows. The bounds
    are the checkers' tolerances as they stand: the trapezoid steps telescope to v / a."""
    n, D = len(row["time"]), len(row["amax"])
    _need(backward["status"] == OK and backward["last"] == n - 1 and backward["first"] == n - 1 - K,
          "the backward stop has K + 1 rows", backward["first"], backward["last"])
    eps = LD(1) / K
    for r in range(K + 1):
        k = K - r                                  # steps from the rest row
        for j in range(D):
            vj, aj = LD(row["qd"][0][j]), LD(row["amax"][j])
            _need(abs(LD(backward["qd"][r][j]) - np.sqrt(k * eps) * vj) <= tol["rho"] * abs(vj), "rates sqrt(k eps)", r, j)
            want = -aj * np.sign(vj) if r < K else LD(0)
            _need(abs(LD(backward["qdd"][r][j]) - want) <= tol["d"] * aj, "qdd_out = -a sign(v)", r, j)
    span = LD(backward["time"][-1]) - LD(backward["time"][0])
    _need(abs(span - LD(duration)) <= tol["dt"] * max(abs(backward["time"][-1]), duration), "the stop lasts v / a")
    _need(forward["status"] == OK and forward["stop_index"] == K, "the forward stop ends K samples on", forward["stop_index"])
    _need(abs(LD(forward["duration"]) - LD(duration)) <= tol["fs_time"] * max(row["time"][0], duration),
          "the forward stop lasts v / a")
    _need(forward["rate2"][-1] == 0.0 and abs(forward["rate2"][K // 2] - 0.5) <= tol["fs_next"], "rate2 falls by eps a sample")


# ------------------------------------------------------------------ A4: case generators
BATCH = 67       # rows of a batch: not a multiple of the 2, 4, 8, 16 or 32 groups of a wave
STRIDE = 160     # samples a row has room for
FAMILIES = ("random", "solver", "under_cut", "all_invalid", "tie", "slack", "first_step", "rest_last",
            "rest_mid", "not_increasing", "no_deceleration", "tight_times", "late_clock", "tiny")


def _rows(arr):
    return [[float(x) for x in r] for r in arr]


def make_row(family, rng, D, n, variant=0):
    """One trajectory of `n` samples: dict time, s, q, qd, qdd, amax, label,
    and optionally index / query: the stop the family is about. No non-finite values."""
    dt = 1e-3 * (0.5 + rng.random(n))
    t0 = rng.random()
    row = dict(label=family)
    pick = None
    if family in ("random", "tiny", "rest_last", "rest_mid", "not_increasing", "tight_times", "late_clock"):
        time, s, qd, qdd, amax = synthetic_row(rng, n, D)
        qd, qdd = 0.3 * np.array(qd).reshape(n, D), np.array(qdd).reshape(n, D)    # brakes within ~40 samples
        time = np.array(time)
        if family == "rest_last":
            qd[-1] = (rng.random(D) - 0.5) * 1e-4          # |v| < 1e-4 on the last sample
            row["index"] = n - 1
            row["query"] = float(time[-1])
        elif family == "rest_mid":
            k = int(rng.integers(n // 2, n - 2))
            qd[k] = (rng.random(D) - 0.5) * 1e-8           # at rest before the end
            row["index"] = k
            row["query"] = float(time[k - 1])
        elif family == "not_increasing":
            k = int(rng.integers(40, n - 8))               # seen by a lane's second or later stride
            time[k + 1] = time[k]
            row["index"] = int(rng.integers(k + 1, n))
            row["query"] = float(time[row["index"]]) - 1e-5
        elif family == "tight_times":
            gaps = np.where(np.arange(n) % 2 == 0, 1e-3 * (0.5 + rng.random(n)), 4e-7 * (0.5 + rng.random(n)))
            time = t0 + np.cumsum(gaps)
            qd *= 0.3
            pick = "keep_below_first"                      # a sample within the tolerance before the segment
        elif family == "late_clock":
            # The row ends just before 2^34 s, where one ulp of a time stamp grows from 1.9e-6 to
            # 3.8e-6: the segment's time shift t[first] - rt is rounded on the coarse side, and
            # rt + shift can land an ulp (more than the tolerance) behind t[first]. Then the sample
            # at `first` is kept and keep = first + 1.
            time = 2.0 ** 34 - (time[-1] - time) - 1e-3 * rng.random()
            pick = "keep_above_first"
        s = np.array(s)
    elif family == "solver":
        # smooth and feasible: a sum of two sinusoids per joint, limits above the peak acceleration
        time = t0 + np.cumsum(dt)
        w, ph, amp = 2.0 + 6.0 * rng.random((2, D)), 6.28 * rng.random((2, D)), 0.2 + rng.random((2, D))
        arg = time[:, None, None] * w[None] + ph[None]
        qd = (amp[None] * np.cos(arg)).sum(axis=1)
        qdd = (-amp[None] * w[None] * np.sin(arg)).sum(axis=1)
        amax = 1.5 * (amp * w).sum(axis=0) + 1.0
        s = np.cumsum(np.abs(qd).max(axis=1) * dt)
    else:
        time = t0 + np.cumsum(dt)
        s = np.cumsum(rng.random(n) * 1e-3)
        amax = 1.0 + 3.0 * rng.random(D)
        qd = (rng.random((n, D)) - 0.5) * 2.0
        qd = np.where(np.abs(qd) < 0.05, 0.05, qd)
        qdd = (rng.random((n, D)) - 0.5) * 3.0
        if family == "under_cut":
            # all joints but one under the backward (1e-8) or the forward (1e-6) cut, or on it
            cut = np.array([5e-9, 1e-8, 5e-7, 1e-6, 0.0, -5e-9, -5e-7])
            for j in range(D):
                if j != D // 2 or D == 1:
                    qd[:, j] = cut[rng.integers(0, len(cut), size=n)]
            if D == 1:
                qd[::2, 0] = 0.3                           # every other sample moves
                qd[-1, 0] = 0.3
        elif family == "all_invalid":
            # one joint stands still and accelerates far beyond its limit: once rate2 > 0 no
            # candidate is valid, d = 0, the loop runs to sample 2 and the velocity match fails
            j = int(rng.integers(0, D))
            if D > 1:                                      # one joint alone always has a valid candidate
                qd[:, j] = 0.0
                qdd[:, j] = 2e6 * amax[j]
        elif family == "tie":
            c = 2.0 ** rng.integers(-2, 3, size=D)
            base = np.where(rng.random(n) < 0.5, -1.0, 1.0) * (0.2 + rng.random(n))
            qd = base[:, None] * c[None, :]
            qdd = ((rng.random(n) - 0.5) * 2.0)[:, None] * c[None, :]
            amax = (1.0 + 3.0 * rng.random()) * c
        elif family == "slack":
            # Constant velocity, no acceleration: at every rate joint 0's braking candidate asks
            # amax[0] |v_j / v_0| of joint j. Every odd joint's limit lies `under` below that, the
            # even ones' 0.3 above. variant 0: under = 5e-9, valid through the backward slack 1e-8
            # only; 1: 5e-11, valid through the forward slack 1e-10 too, and far beyond rounding;
            # 2: 5e-8, valid through neither, so another joint's candidate decides. A slack of
            # another size in a kernel changes which candidate wins, by about 1e-7 of d.
            qd = np.tile(qd[0], (n, 1))
            qdd = np.zeros((n, D))
            under = (5e-9, 5e-11, 5e-8)[variant % 3]
            for j in range(1, D):
                amax[j] = amax[0] * abs(qd[0, j] / qd[0, 0]) - (under if j % 2 else -0.3)
            k = int(rng.integers(n // 2, n))
            row.update(index=k, query=float(time[k - 1]), fs_query=float(time[int(rng.integers(0, n // 4))]))
        elif family == "first_step":
            qd *= 1e-4                                     # d dt >= 1 at once: two rows, one forward step
            if rng.random() < 0.5:
                row["index"] = 2                           # uses every sample, and matches: |v| < 1e-2
        elif family == "no_deceleration":
            # the rest sample's only moving joint asks more of a joint under the cut than that
            # joint's limit allows: no candidate is valid at rate2 = 0 (needs D >= 2)
            k = int(rng.integers(n // 2, n - 2))
            if D > 1:
                qd[k] = 9e-9
                qd[k, 0] = 1e-8
                amax[0], amax[1:] = 10.0, 1.0
            row["index"] = k
            row["query"] = float(time[k - 1])
    q = np.cumsum(np.asarray(qd).reshape(n, D) * 1e-3, axis=0) if n else np.zeros((0, D))
    row.update(time=[float(x) for x in time], s=[float(x) for x in s], q=_rows(q), qd=_rows(qd), qdd=_rows(qdd),
               amax=[float(x) for x in amax])
    if pick:
        # the stop sample is chosen so that the family shows what it is for: the first index from
        # a random start whose stop (by the restatement) has the wanted kept count
        start = int(rng.integers(n // 2, n))
        for index in list(range(start, n)) + list(range(n // 2, start)):
            r = stop_at_index(row["time"], row["qd"], row["qdd"], row["amax"], 1e-3, index)
            if r["status"] == OK and (r["keep"] < r["first"] if pick == "keep_below_first" else r["keep"] > r["first"]):
                row["index"] = index
                row["query"] = row["time"][index - 1]
                break
    return row


def make_batch(D, seed=20261017):
    """The batch both the CPU and the GPU tests use for D joints: BATCH rows over FAMILIES with
    ragged counts (0, 1 and 2 among them), and per row a stop time, a stop index and a fastest-stop
    query: before the first sample, on a sample, between samples, on the last sample, after the
    end; index 0, 1, n - 1, n and inside. Rows whose family is about one stop carry that stop."""
    rng = np.random.default_rng(seed + 1000 * D)
    rows = []
    for b in range(BATCH):
        family = FAMILIES[b % len(FAMILIES)]
        turn = b // len(FAMILIES)
        n = turn % 3 if family == "tiny" else int(rng.integers(72, STRIDE + 1))
        row = make_row(family, rng, D, n, variant=turn)
        kind = (turn + b % len(FAMILIES)) % 5
        t = row["time"]
        if n == 0:
            query, index = 0.25, (0, 1, -1, 0, 2)[kind]
        else:
            i = int(rng.integers(0, max(n - 1, 1)))
            query = (t[0] - 0.25, t[i], 0.5 * (t[i] + t[min(i + 1, n - 1)]), t[-1], t[-1] + 1e-3)[kind]
            index = (0, 1, n - 1, n, int(rng.integers(n // 2, n)) if n > 2 else 1)[kind]
        row.setdefault("fs_query", float(query))
        row.setdefault("query", float(query))
        row.setdefault("index", int(index))
        rows.append(row)
    return rows


def pack_batch(rows, D, stride=STRIDE):
    """The rows as padded numpy arrays: time, s [B][stride], q, qd, qdd [B][stride][D] (padding
    -7), amax [B][D], count, index int32 [B], query, fs_query [B]."""
    B = len(rows)
    out = dict(time=np.full((B, stride), -7.0), s=np.full((B, stride), -7.0), q=np.full((B, stride, D), -7.0),
               qd=np.full((B, stride, D), -7.0), qdd=np.full((B, stride, D), -7.0), amax=np.zeros((B, D)),
               count=np.zeros(B, dtype=np.int32), index=np.zeros(B, dtype=np.int32), query=np.zeros(B),
               fs_query=np.zeros(B))
    for b, r in enumerate(rows):
        n = len(r["time"])
        out["count"][b] = n
        out["time"][b, :n], out["s"][b, :n] = r["time"], r["s"]
        for k in ("q", "qd", "qdd"):
            out[k][b, :n] = np.asarray(r[k], dtype=np.float64).reshape(n, D)
        out["amax"][b] = r["amax"]
        out["index"][b], out["query"][b], out["fs_query"][b] = r["index"], r["query"], r["fs_query"]
    return out


# ------------------------------------------------------------------ outcome counters
BACKWARD_OUTCOMES = ("ok", "out_of_range", "invalid_argument", "internal", "not_found", "n0", "n1", "n2",
                     "under_cut", "all_invalid", "tie", "slack", "off_slack", "first_step", "rest_last", "used_all",
                     "not_increasing_far", "no_deceleration", "keep_below_first", "keep_above_first")
FORWARD_OUTCOMES = ("ok", "invalid_argument", "n0", "n1", "n2", "on_last", "ran_to_end", "stopped_inside",
                    "under_cut", "all_invalid", "tie", "slack", "off_slack", "first_step")
# One joint alone always has a valid candidate (its own limit, met to rounding), and no second joint
# to tie with or to be asked too much, or a little too much, of.
UNREACHABLE = {1: {"all_invalid", "tie", "no_deceleration", "slack", "off_slack"}}
BEYOND_ROUNDING = 1e-12


def _slack_outcomes(cands, slack, seen):
    """"slack": a candidate (d, valid, margin) that is valid only through the slack, by far more
    than rounding (-slack <= margin < -1e-12); "off_slack": one that is invalid by less than 1000
    slacks. Both come from limits built for them (family "slack"), not from rounding."""
    if any(c[1] and -slack <= c[2] < -BEYOND_ROUNDING for c in cands):
        seen.add("slack")
    if any(not c[1] and -1000.0 * slack <= c[2] < -slack for c in cands):
        seen.add("off_slack")


def backward_outcomes(row, res, by_index):
    """What the stop `res` (asserted equal to the restatement by the caller) met on the way."""
    n = len(row["time"])
    seen = {STATUS_NAMES[res["status"]], "n%d" % n if n <= 2 else "n>2"}
    trace = []
    if by_index:
        stop_at_index(row["time"], row["qd"], row["qdd"], row["amax"], 1e-3, row["index"], trace=trace)
    else:
        stop_before_time(row["time"], row["qd"], row["qdd"], row["amax"], 1e-3, row["query"], trace=trace)
    for k, step in enumerate(trace):
        valid = [c for c in step["cands"] if c[1]]
        if step["under_cut"]:
            seen.add("under_cut")
        if step["cands"] and not valid and step["rate2"] > 0.0:
            seen.add("all_invalid")
        if step["cands"] and not any(c[1] and c[0] < 0.0 for c in step["cands"]) and step["rate2"] == 0.0:
            seen.add("no_deceleration")
        if step["d"] < 0.0 and sum(1 for c in valid if c[0] == step["d"]) >= 2:
            seen.add("tie")
        _slack_outcomes(step["cands"], BACKWARD_SLACK, seen)
        if k == 0 and step["next"] >= 1.0:
            seen.add("first_step")
    if res["status"] == OK and n > 0:
        if res["last"] == n - 1 and max(abs(x) for x in row["qd"][-1]) < 1e-4:
            seen.add("rest_last")
        elif res["first"] == 1 or res["last"] == 1:
            seen.add("used_all")
        if res["keep"] < res["first"]:
            seen.add("keep_below_first")
        if res["keep"] > res["first"]:
            seen.add("keep_above_first")
    if res["status"] == INVALID_ARGUMENT and row["label"] == "not_increasing":
        seen.add("not_increasing_far")
    return seen


def forward_outcomes(row, res):
    n = len(row["time"])
    seen = {STATUS_NAMES[res["status"]], "n%d" % n if n <= 2 else "n>2"}
    if res["status"] != OK:
        return seen
    m = len(res["rate2"])
    lo = res["stop_index"] - m + 1
    seen.add("on_last" if m == 1 else "ran_to_end" if res["rate2"][-1] > 0.0 else "stopped_inside")
    amax, D = row["amax"], len(row["amax"])
    for k in range(m - 1):
        v, a, rate2 = row["qd"][lo + k], row["qdd"][lo + k], res["rate2"][k]
        cands = []
        for c in range(D):
            if abs(v[c]) < FORWARD_CUT:
                continue
            for sg in (-1.0, 1.0):
                d = 2.0 * (-a[c] * rate2 + sg * amax[c]) / v[c]
                margin = min(min(amax[j] - (a[j] * rate2 + 0.5 * v[j] * d), (a[j] * rate2 + 0.5 * v[j] * d) + amax[j])
                             for j in range(D))
                cands.append((d, margin >= -FORWARD_SLACK, margin))
        valid = [c for c in cands if c[1]]
        if any(abs(x) < FORWARD_CUT for x in v):
            seen.add("under_cut")
        if cands and not valid:
            seen.add("all_invalid")
        if res["drate2"][k] < 0.0 and sum(1 for c in valid if c[0] == res["drate2"][k]) >= 2:
            seen.add("tie")
        _slack_outcomes(cands, FORWARD_SLACK, seen)
        if k == 0 and res["rate2"][1] == 0.0:
            seen.add("first_step")
    return seen


def outcome_table(title, names, counts_by_d):
    """The printed table: one line per D, one column per outcome."""
    lines = [title, "  D   L " + " ".join("%4s" % x[:4] for x in names)]
    for D in sorted(counts_by_d):
        lines.append("%3d %3d " % (D, stop_group_lanes(D)) + " ".join("%4d" % counts_by_d[D].get(x, 0) for x in names))
    lines.append("  columns: " + ", ".join(names))
    return "\n".join(lines)

"""What the buffer-set row operations and the bulk readouts mean, stated independently of the
kernels.

1. A restatement of TrajectoryBuffer (trajectory_buffer.{h,cc} of the reference) in plain Python
   lists and floats: every arithmetic operation is one IEEE double operation in the reference's
   order, and each function cites the lines it follows. It is written from those sources, not from
   csrc/tpamd_buffer.h, csrc/tpamd_readout.h or host/trajectory_buffer.cc, so that a misreading
   those three share does not pass. On top of it: the control-tick readout (sample_at_ticks), the
   packed download (pack) and a set of buffers with the capacity rule of include/tpamd.h
   (ReferenceSet: a result of more than `capacity` rows is TPAMD_PLAN_MORE and changes nothing).
2. Exact checkers in fractions.Fraction (check_setpoint, check_buffer_invariants) that take the
   inputs and the outputs of ANY implementation. They do not share the order of operations.
3. Seeded case generators shared by the CPU and the GPU tests (layout_program, operation_program,
   tolerance_program, tick_requests, id_list), a packer for the C-ABI layout, the
   comparison both tests run (run_program, compare_ticks, compare_pack) against any backend, and
   the outcome names every joint count must show (OUTCOMES).

Plain Python; numpy only packs arrays and draws random numbers. No GPU, no product imports.
"""
import collections
import functools
import struct
from fractions import Fraction

import numpy as np

from stop_reference import offset_bracket, insert_segment_kept

OK, FAILED_PRECONDITION, OUT_OF_RANGE, INVALID_ARGUMENT, MORE = 0, 1, 2, 3, 100   # TPAMD_PLAN_*
TIMESTEP_TOLERANCE = 1e-6      # trajectory_buffer.h TrajectoryBufferOptions::timestep_tolerance
INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
SENTINEL = -9.25
ARRAYS = ("q", "qd", "qdd")


def time_to_sec(ns):
    """TimeToSec, time.h:26-29: the nanoseconds as a double, divided by 1e9."""
    return float(ns) / 1e9


def time_from_sec(sec):
    """TimeFromSec, time.h:22-24, as nanoseconds: seconds * 1e9 truncated towards zero."""
    return int(sec * 1e9)


# ------------------------------------------------------------------ 1: the restatement
class Buffer:
    """TrajectoryBuffer: t [n] and q, qd, qdd [n][D] as lists of Python floats, and the sequence
    number. Every method returns what the reference returns; `last` holds what the last
    InsertSegment / DiscardSegmentBefore met (for the outcome counters only)."""

    def __init__(self, tolerance=TIMESTEP_TOLERANCE):
        self.tol = tolerance
        self.seq = 0
        self.t, self.q, self.qd, self.qdd = [], [], [], []
        self.last = None

    def copy(self):
        b = type(self)(self.tol)
        b.seq, b.t = self.seq, list(self.t)
        b.q, b.qd, b.qdd = ([list(r) for r in a] for a in (self.q, self.qd, self.qdd))
        return b

    def snapshot(self):
        return dict(t=list(self.t), q=[list(r) for r in self.q], qd=[list(r) for r in self.qd],
                    qdd=[list(r) for r in self.qdd], seq=self.seq)

    def clear(self):                                           # :64-70
        self.seq = 0
        self.t, self.q, self.qd, self.qdd = [], [], [], []

    def num_samples(self):
        return len(self.q)

    def sequence_number(self):
        return self.seq

    def start_time_ns(self):                                   # :50-55
        return time_from_sec(0) if not self.t else time_from_sec(self.t[0])

    def end_time_ns(self):                                     # :57-62 (absl::Time() is 0 ns)
        return 0 if not self.t else time_from_sec(self.t[-1])

    def insert_segment(self, t, q, qd, qdd):                   # :79-133
        self.seq += 1                                          # :96
        if not q:                                              # :98-100
            self.last = "empty_segment"
            return OK
        keep, replaced = insert_segment_kept(self.t, t[0], self.tol)       # :102-120
        if replaced:                                           # :106-113
            self.t = list(t)
            self.q, self.qd, self.qdd = ([list(r) for r in a] for a in (q, qd, qdd))
            self.seq = 0
            self.last = "replaced"
            return OK
        self.t = self.t[:keep] + list(t)                       # :121-130
        self.q = self.q[:keep] + [list(r) for r in q]
        self.qd = self.qd[:keep] + [list(r) for r in qd]
        self.qdd = self.qdd[:keep] + [list(r) for r in qdd]
        self.last = "kept"
        return OK

    def append_sample(self, t, q, qd, qdd):                    # :135-149
        if self.t and self.t[-1] >= t:                         # :139-141
            return INVALID_ARGUMENT
        self.t.append(t)
        self.q.append(list(q))
        self.qd.append(list(qd))
        self.qdd.append(list(qdd))
        return OK

    def discard_segment_before_ns(self, ns):                   # :151-153
        self.discard_segment_before(time_to_sec(ns))

    def discard_segment_before(self, time_sec):                # :155-208
        if not self.t:                                         # :156-158
            self.last = "empty"
            return
        if time_sec <= self.t[0]:                              # :159-161
            self.last = "before_front"
            return
        if time_sec > self.t[-1]:                              # :162-165
            self.clear()
            self.last = "cleared"
            return
        offset = 0                                             # :168-170 upper_bound with a <= b
        while offset < len(self.t) and not (time_sec <= self.t[offset]):
            offset += 1
        if offset <= 0:                                        # :173-175
            self.last = "before_front"
            return
        close = time_sec - self.t[offset - 1] <= self.tol              # :179-180
        interpolate = abs(self.t[offset] - time_sec) > self.tol        # :181-182
        if close or interpolate:                               # :184-186
            offset -= 1
        if interpolate:                                        # :189-201
            _, a = self.position_at_time(time_sec)
            _, b = self.velocity_at_time(time_sec)
            _, c = self.acceleration_at_time(time_sec)
            self.t[offset] = time_sec
            self.q[offset], self.qd[offset], self.qdd[offset] = a, b, c
        del self.t[:offset], self.q[:offset], self.qd[:offset], self.qdd[:offset]      # :204-207
        self.last = "interpolated" if interpolate else "close_before" if close else "on_sample"

    def positions_up_to_time_ns(self, ns):                     # :210-226, as a count
        if not self.t:                                         # :214-216
            return 0
        time_sec = time_to_sec(ns)                             # :217
        if time_sec < self.t[0] or time_sec > self.t[-1]:      # :218-220
            return 0
        it = 0                                                 # :223 upper_bound
        while it < len(self.t) and not (time_sec < self.t[it]):
            it += 1
        return it - 1                                          # :224

    def offset_bracket(self, time_sec):                        # :233-251
        return offset_bracket(self.t, time_sec)

    def _value_at_time(self, values, time_sec):
        """InterpolateLinear between the bracket's rows, a + t (b - a) with
        t = (x - t_l) / (t_u - t_l); with l == u the sample itself."""
        st, l, u = self.offset_bracket(time_sec)
        if st != OK:
            return st, None
        if l == u:
            return OK, list(values[l])
        f = (time_sec - self.t[l]) / (self.t[u] - self.t[l])
        return OK, [a + f * (b - a) for a, b in zip(values[l], values[u])]

    def position_at_time(self, time_sec):                      # :253-262
        return self._value_at_time(self.q, time_sec)

    def velocity_at_time(self, time_sec):                      # :269-278
        return self._value_at_time(self.qd, time_sec)

    def acceleration_at_time(self, time_sec):                  # :285-294
        return self._value_at_time(self.qdd, time_sec)

    def add_offset_to_timestamps_ns(self, ns):                 # :387-389 offset / Seconds(1)
        self.add_offset_to_timestamps(float(ns) / 1e9)

    def add_offset_to_timestamps(self, offset):                # :390-393
        self.t = [x + offset for x in self.t]


def tick_time(start_ns, step_ns, j):
    """start_ns + j step_ns in int64, or None if the product or the sum leaves int64."""
    off = j * step_ns
    if not INT64_MIN <= off <= INT64_MAX:
        return None
    ns = start_ns + off
    return ns if INT64_MIN <= ns <= INT64_MAX else None


def sample_at_ticks(buffer, start_ns, step_ns, T):
    """Get{Position,Velocity,Acceleration}AtTime at the ticks start_ns + j step_ns, j < T, of one
    buffer (None: an id outside the set): (status [T], rows [T] of (q, qd, qdd) or None)."""
    status, rows = [], []
    for j in range(T):
        if buffer is None:
            status.append(INVALID_ARGUMENT)
            rows.append(None)
            continue
        ns = tick_time(start_ns, step_ns, j)
        if ns is None:
            status.append(OUT_OF_RANGE)
            rows.append(None)
            continue
        x = time_to_sec(ns)
        st, a = buffer.position_at_time(x)
        status.append(st)
        rows.append(None if st != OK else (a, buffer.velocity_at_time(x)[1], buffer.acceleration_at_time(x)[1]))
    return status, rows


def pack(buffers, ids):
    """The packed download of the listed buffers: (offsets [len(ids) + 1], t, q, qd, qdd); an id
    outside the set counts 0 rows."""
    offsets, t, q, qd, qdd = [0], [], [], [], []
    for b in ids:
        if 0 <= b < len(buffers):
            t += buffers[b].t
            q += buffers[b].q
            qd += buffers[b].qd
            qdd += buffers[b].qdd
        offsets.append(len(t))
    return offsets, t, q, qd, qdd


class ReferenceSet:
    """B Buffers behind the calls of a buffer set (include/tpamd.h tpamd_buffer_set_*). With a
    capacity, an insert or append whose result has more rows is MORE and changes nothing, the
    sequence number included. `buffer_class` lets the mutation test put a wrong Buffer here."""

    def __init__(self, B, D, tolerance=TIMESTEP_TOLERANCE, capacity=None, buffer_class=Buffer):
        self.B, self.D, self.capacity = B, D, capacity
        self.buffers = [buffer_class(tolerance) for _ in range(B)]

    def _buffer(self, b):
        return self.buffers[b] if 0 <= b < self.B else None

    def apply(self, rnd):
        """One round (dict kind, ids, entries, unit): the statuses of its entries."""
        ids = rnd["ids"] if rnd["ids"] is not None else range(len(rnd["entries"]))
        out = []
        for b, e in zip(ids, rnd["entries"]):
            buf = self._buffer(b)
            if buf is None:
                out.append(INVALID_ARGUMENT)
                continue
            kind = rnd["kind"]
            if kind in ("insert", "append"):
                trial = buf.copy()
                st = trial.insert_segment(e["t"], e["q"], e["qd"], e["qdd"]) if kind == "insert" else \
                    trial.append_sample(e["t"], e["q"], e["qd"], e["qdd"])
                if st == OK and self.capacity is not None and trial.num_samples() > self.capacity:
                    st = MORE
                elif st == OK:
                    self.buffers[b] = trial
                out.append(st)
                continue
            if kind == "discard":
                buf.discard_segment_before_ns(e["ns"]) if rnd["unit"] == "ns" else buf.discard_segment_before(e["sec"])
            elif kind == "add_offset":
                buf.add_offset_to_timestamps_ns(e["ns"]) if rnd["unit"] == "ns" else buf.add_offset_to_timestamps(e["sec"])
            elif kind == "clear":
                buf.clear()
            else:
                raise ValueError(kind)
            out.append(OK)
        return out

    def download(self, ids=None, capacity=None):
        """dict offsets, t and q, qd, qdd (flat lists); rows None if they exceed `capacity`."""
        offsets, t, q, qd, qdd = pack(self.buffers, range(self.B) if ids is None else ids)
        if capacity is not None and offsets[-1] > capacity:
            return dict(offsets=offsets, t=None, q=None, qd=None, qdd=None)
        return dict(offsets=offsets, t=t, q=_flat(q), qd=_flat(qd), qdd=_flat(qdd))

    def info(self, ids, time_ns):
        out = dict(count=[], seq=[], start_ns=[], end_ns=[], up_to=[])
        for b, ns in zip(range(self.B) if ids is None else ids, time_ns):
            buf = self._buffer(b)
            out["count"].append(buf.num_samples() if buf else 0)
            out["seq"].append(buf.sequence_number() if buf else 0)
            out["start_ns"].append(buf.start_time_ns() if buf else 0)
            out["end_ns"].append(buf.end_time_ns() if buf else 0)
            out["up_to"].append(buf.positions_up_to_time_ns(ns) if buf else 0)
        return out

    def ticks(self, ids, start_ns, step_ns, T, want=(True, True, True)):
        """dict status [count * T] and q, qd, qdd [count * T * D] flat lists (None if not wanted)
        that hold SENTINEL wherever a tick is not OK."""
        D = self.D
        n = len(start_ns)
        out = dict(status=[])
        for k, w in zip(ARRAYS, want):
            out[k] = [SENTINEL] * (n * T * D) if w else None
        for e, (b, s0) in enumerate(zip(range(n) if ids is None else ids, start_ns)):
            status, rows = sample_at_ticks(self._buffer(b), s0, step_ns, T)
            out["status"] += status
            for j, row in enumerate(rows):
                if row is None:
                    continue
                for k, vals in zip(ARRAYS, row):
                    if out[k] is not None:
                        o = (e * T + j) * D
                        out[k][o:o + D] = vals
        return out


# ------------------------------------------------------------------ 2: the exact checkers
class BufferCheckError(AssertionError):
    pass


def _need(cond, what, *info):
    if not cond:
        raise BufferCheckError("%s %s" % (what, info if info else ""))


def _flat(rows):
    return [x for r in rows for x in r]


def bits(values):
    """The bytes of the doubles (the bit-for-bit comparison)."""
    if isinstance(values, np.ndarray):
        return np.ascontiguousarray(values, dtype=np.float64).tobytes()
    values = list(values)
    return struct.pack("<%dd" % len(values), *values)


def _all_sentinel(values):
    return bool((np.asarray(values, dtype=np.float64) == SENTINEL).all())


SETPOINT_BOUND_ULPS = 7


def check_setpoint(times, values, x, got):
    """Asserts that `got` [D] is the linear interpolation of the rows values [n][D] with stamps
    times [n] at time x (which lies within the stamps), from any implementation.

    The bracket is found by exact comparison: the last sample if x equals the last stamp, else the
    l with times[l] <= x < times[l + 1]. Let t = (x - t_l) / (t_u - t_l) in exact rationals,
    0 <= t < 1, and u = 2^-53. An implementation that computes a + t (b - a) in doubles rounds
    x - t_l, t_u - t_l and their quotient (three factors 1 + e_i, |e_i| <= u) to get t', then

        b - a     one rounding:   (b - a)(1 + e4)
        t' (b-a)  one rounding:   t (b - a)(1 + th),  |th| <= 5u / (1 - 5u)      (five factors)
        a + ...   one rounding:   (a + t (b - a)(1 + th))(1 + e6)

    so |got - exact| <= u |a + t (b - a)| + (1 + u) |th| t |b - a|. With 0 <= t < 1 both
    |a + t (b - a)| <= max(|a|, |b|) and t |b - a| <= |a| + |b|, which gives
    |got - exact| <= (u + 5u (1 + 6u)) (|a| + |b|) < 7 * 2^-53 (|a| + |b|), the bound used
    (no underflow: the test values are normal numbers or zero). At t = 0 every factor multiplies
    an exact zero and the result is a itself."""
    n = len(times)
    X = Fraction(x)
    _need(n > 0 and Fraction(times[0]) <= X <= Fraction(times[-1]), "the time lies within the stamps", x)
    if X == Fraction(times[-1]):
        for d, g in enumerate(got):
            _need(Fraction(g) == Fraction(values[-1][d]), "on the last stamp the last sample is returned", d, g)
        return
    l = max(i for i in range(n) if Fraction(times[i]) <= X)
    u = l + 1
    _need(Fraction(times[l]) <= X < Fraction(times[u]), "the bracket holds the time", l, u)
    t = (X - Fraction(times[l])) / (Fraction(times[u]) - Fraction(times[l]))
    for d, g in enumerate(got):
        a, b = Fraction(values[l][d]), Fraction(values[u][d])
        exact = a + t * (b - a)
        if t == 0:
            _need(Fraction(g) == a, "on a stamp the sample itself is returned", d, g)
        bound = SETPOINT_BOUND_ULPS * Fraction(1, 2 ** 53) * (abs(a) + abs(b))
        _need(abs(Fraction(g) - exact) <= bound, "the setpoint is the exact lerp within 7 * 2^-53 (|a| + |b|)", d, g,
              float(exact))


def _row(s, i):
    return bits([s["t"][i]] + s["q"][i] + s["qd"][i] + s["qdd"][i])


def _rows(s, lo, hi):
    return b"".join(_row(s, i) for i in range(lo, hi))


def _tolerance_truths(a, b, tolerance, op):
    """The admissible values of `a - b op tolerance`: that of the exact difference and that of the
    rounded one (they differ only when the rounding crosses the tolerance)."""
    exact, rounded = Fraction(a) - Fraction(b), Fraction(a - b)
    tol = Fraction(tolerance)
    if op == "<":
        return {exact < tol, rounded < tol}
    if op == "<=":
        return {exact <= tol, rounded <= tol}
    return {abs(exact) > tol, abs(rounded) > tol}


def check_buffer_invariants(before, kind, entry, unit, status, after, tolerance=TIMESTEP_TOLERANCE, capacity=None):
    """Asserts that the snapshot `after` (dict t, q, qd, qdd, seq from any implementation) is what
    the operation makes of the snapshot `before`: the kept rows are bit-copies of rows of `before`,
    inserted rows bit-copies of the segment, count, sequence number and first stamp follow the
    reference's rules (by exact comparison), and only the one interpolated row of a discard holds
    new values (judged by check_setpoint). Stamps must not decrease."""
    n = len(before["t"])
    m = len(after["t"])
    _need(all(len(after[k]) == m for k in ARRAYS), "one row of q, qd, qdd per stamp")
    unchanged = lambda: _need(m == n and _rows(after, 0, m) == _rows(before, 0, n) and after["seq"] == before["seq"],
                              "the buffer is unchanged", kind)
    if status == MORE:
        _need(capacity is not None and kind in ("insert", "append"), "MORE only from a set without room")
        unchanged()
        return
    if kind == "insert":
        _need(status == OK, "InsertSegment is OK", status)
        seg = dict(t=entry["t"], q=entry["q"], qd=entry["qd"], qdd=entry["qdd"])
        k = len(seg["t"])
        if k == 0:
            _need(m == n and _rows(after, 0, m) == _rows(before, 0, n) and after["seq"] == before["seq"] + 1,
                  "an empty segment only raises the sequence number")
            return
        front = Fraction(seg["t"][0])
        below = sum(1 for x in before["t"] if Fraction(x) < front)     # stamps do not decrease
        if n == 0 or below == 0:
            _need(m == k and after["seq"] == 0 and _rows(after, 0, m) == _rows(seg, 0, k), "the segment replaces the buffer")
            return
        less = _tolerance_truths(seg["t"][0], before["t"][below - 1], tolerance, "<")
        keep = m - k
        _need((keep == below and False in less) or (keep == below - 1 and True in less),
              "the kept count is InsertSegment's", keep, below)
        _need(capacity is None or m <= capacity, "the result fits the capacity")
        _need(after["seq"] == before["seq"] + 1, "the sequence number goes up", after["seq"])
        _need(_rows(after, 0, keep) == _rows(before, 0, keep), "kept rows are bit-copies")
        _need(_rows(after, keep, m) == _rows(seg, 0, k), "inserted rows are bit-copies of the segment")
        return
    if kind == "append":
        if n and Fraction(before["t"][-1]) >= Fraction(entry["t"]):
            _need(status == INVALID_ARGUMENT, "a sample not after the last is an invalid argument", status)
            unchanged()
            return
        _need(status == OK and m == n + 1 and after["seq"] == before["seq"], "AppendSample adds one row")
        row = dict(t=[entry["t"]], q=[entry["q"]], qd=[entry["qd"]], qdd=[entry["qdd"]])
        _need(_rows(after, 0, n) == _rows(before, 0, n) and _row(after, n) == _row(row, 0), "rows are bit-copies")
        return
    _need(status == OK, "the operation is OK", kind, status)
    if kind == "clear":
        _need(m == 0 and after["seq"] == 0, "Clear leaves no samples and sequence number 0")
        return
    if kind == "add_offset":
        off = float(entry["ns"]) / 1e9 if unit == "ns" else entry["sec"]
        _need(m == n and after["seq"] == before["seq"], "AddOffsetToTimestamps keeps count and sequence number")
        for i in range(n):
            _need(bits([after["t"][i]]) == bits([before["t"][i] + off]), "stamp + offset", i)
        _need(all(bits(_flat(after[k])) == bits(_flat(before[k])) for k in ARRAYS), "the values stay")
        return
    _need(kind == "discard", "a known operation", kind)
    x = time_to_sec(entry["ns"]) if unit == "ns" else entry["sec"]
    X = Fraction(x)
    if n == 0 or X <= Fraction(before["t"][0]):
        unchanged()
        return
    if X > Fraction(before["t"][-1]):
        _need(m == 0 and after["seq"] == 0, "a discard behind the last sample clears the buffer")
        return
    offset = sum(1 for v in before["t"] if Fraction(v) < X)            # the first stamp at or after x
    close = _tolerance_truths(x, before["t"][offset - 1], tolerance, "<=")
    interpolate = _tolerance_truths(before["t"][offset], x, tolerance, ">")
    _need(after["seq"] == before["seq"], "a discard keeps the sequence number")
    drop = n - m
    if drop == offset:
        _need(False in close and False in interpolate, "the sample at or just behind the time becomes the first", offset)
        _need(_rows(after, 0, m) == _rows(before, drop, n), "kept rows are bit-copies")
        return
    _need(drop == offset - 1, "at most one sample before the time is kept", drop, offset)
    _need(_rows(after, 1, m) == _rows(before, drop + 1, n), "kept rows are bit-copies")
    if _row(after, 0) == _row(before, drop):
        _need(True in close and False in interpolate, "an unchanged first sample is one close before the time")
        return
    _need(True in interpolate, "a new first sample needs a next sample beyond the tolerance")
    _need(bits([after["t"][0]]) == bits([x]), "the interpolated sample is stamped with the time")
    for k in ARRAYS:
        check_setpoint(before["t"], before[k], x, after[k][0])


# ------------------------------------------------------------------ 3: outcomes
INSERT_OUTCOMES = ("insert_replaced_whole", "insert_kept_all", "insert_kept_some", "insert_kept_one_less",
                   "insert_kept_0_no_replace", "insert_empty_segment", "insert_more")
APPEND_OUTCOMES = ("append_ok", "append_not_after_last", "append_more")
DISCARD_OUTCOMES = ("discard_empty", "discard_before_front", "discard_cleared", "discard_on_sample",
                    "discard_close_before", "discard_interpolated")
TICK_OUTCOMES = ("tick_ok_interior", "tick_on_first_stamp", "tick_on_last_stamp", "tick_before", "tick_after",
                 "tick_empty_buffer", "tick_bad_id", "tick_overflow")
OUTCOMES = INSERT_OUTCOMES + APPEND_OUTCOMES + DISCARD_OUTCOMES + TICK_OUTCOMES
LAYOUT_OUTCOMES = ("insert_more", "append_more", "insert_replaced_whole", "insert_kept_all", "append_ok",
                   "discard_on_sample")
PROGRAM_OUTCOMES = tuple(x for x in INSERT_OUTCOMES + APPEND_OUTCOMES + DISCARD_OUTCOMES
                         if x not in ("insert_more", "append_more"))


def classify(before, kind, entry, unit, status, after):
    """The outcome names of one operation, from the states around it (an implementation's own:
    the caller has asserted them)."""
    n, m = len(before["t"]), len(after["t"])
    if kind == "insert":
        k = len(entry["t"])
        if status == MORE:
            return {"insert_more"}
        if k == 0:
            return {"insert_empty_segment"}
        if after["seq"] == 0:
            return {"insert_replaced_whole"}
        keep, below = m - k, sum(1 for x in before["t"] if x < entry["t"][0])
        seen = {"insert_kept_all" if keep == n else "insert_kept_some"} if keep else set()
        if keep < below:
            seen.add("insert_kept_one_less")
        if keep == 0:
            seen.add("insert_kept_0_no_replace")
        return seen
    if kind == "append":
        return {"append_more" if status == MORE else "append_ok" if status == OK else "append_not_after_last"}
    if kind == "discard":
        x = time_to_sec(entry["ns"]) if unit == "ns" else entry["sec"]
        if n == 0:
            return {"discard_empty"}
        if x <= before["t"][0]:
            return {"discard_before_front"}
        if m == 0:
            return {"discard_cleared"}
        offset = sum(1 for v in before["t"] if v < x)
        if n - m == offset:
            return {"discard_on_sample"}
        return {"discard_close_before" if _row(after, 0) == _row(before, n - m) else "discard_interpolated"}
    return set()


def classify_tick(buffer_t, in_set, start_ns, step_ns, j, status):
    ns = tick_time(start_ns, step_ns, j)
    if not in_set:
        return "tick_bad_id"
    if ns is None:
        return "tick_overflow"
    if not buffer_t:
        return "tick_empty_buffer"
    x = time_to_sec(ns)
    if x < buffer_t[0]:
        return "tick_before"
    if x > buffer_t[-1]:
        return "tick_after"
    return "tick_on_last_stamp" if x == buffer_t[-1] else "tick_on_first_stamp" if x == buffer_t[0] else \
        "tick_ok_interior"


def outcome_table(title, names, counts_by_d):
    lines = [title, "  D " + " ".join("%4s" % "".join(w[0] for w in x.split("_"))[:4] for x in names)]
    for D in sorted(counts_by_d):
        lines.append("%3d " % D + " ".join("%4d" % counts_by_d[D].get(x, 0) for x in names))
    lines.append("  columns: " + ", ".join(names))
    return "\n".join(lines)


# ------------------------------------------------------------------ 3: case generators
BUFFERS = 48
ROUNDS = 30
GRID_NS = 1_000_000            # segment stamps of the generators fall on whole nanoseconds


def _values(rng, n, D):
    """Rows of values between 1e-3 and 2 in size, both signs. The second factor fills the low
    mantissa bits: numpy's uniform doubles are multiples of 2^-52 (b - a, 2^-51 apart), for which
    a + 1 (b - a) is b exactly and a lerp that should have been a copy could not be told from one."""
    return [[float(x) for x in r] for r in rng.uniform(-2.0, 2.0, size=(n, D)) * 10.0 ** rng.uniform(-3.0, 0.0, size=(n, D))]


def make_segment(rng, D, n, front, tolerance=TIMESTEP_TOLERANCE, tight=False, repeat=False):
    """A segment of n rows from `front` on: steps of 0.5 .. 1.5 ms; `tight` puts one pair of stamps
    1.2 tolerances apart, `repeat` one pair of equal stamps."""
    t, x = [], front
    special = int(rng.integers(1, n)) if n > 2 and (tight or repeat) else -1
    for i in range(n):
        if i:
            x = x if (i == special and repeat) else x + 1.2 * tolerance if i == special else \
                x + 1e-3 * (0.5 + float(rng.random()))
        t.append(x)
    return dict(t=t, q=_values(rng, n, D), qd=_values(rng, n, D), qdd=_values(rng, n, D))


def grid_segment(rng, D, n, front_ns):
    """A segment whose stamps are whole nanoseconds as TimeToSec gives them, so that control ticks
    can fall exactly on them."""
    ns = front_ns + np.concatenate([[0], np.cumsum(rng.integers(500_000, 1_500_000, size=max(n - 1, 0)))])
    return dict(t=[time_to_sec(int(x)) for x in ns[:n]], q=_values(rng, n, D), qd=_values(rng, n, D), qdd=_values(rng, n, D))


def _pick_ids(rng, B, everyone=False):
    """ids of a round: None (buffers 0 .. B-1) or a shuffled subset."""
    if everyone or rng.random() < 0.25:
        return None, list(range(B))
    ids = [int(x) for x in rng.permutation(B)[:int(rng.integers(1, B + 1))]]
    return ids, ids


def _insert_front(rng, buf, variant, tol):
    """The front stamp of a segment for the buffer, by variant: the branches of InsertSegment."""
    t = buf.t
    if not t:
        return 1.0 + float(rng.random())
    i = int(rng.integers(0, len(t)))
    return (t[-1] + 1e-3, t[i], t[i] + 0.5 * tol, t[0] + 0.5 * tol, t[0] - 1e-3, t[i] + 1.5 * tol,
            t[-1] + 0.5 * tol, t[i] - 0.5 * tol)[variant % 8]


def _discard_time(rng, buf, variant, tol):
    t = buf.t
    if not t:
        return 1.0
    i = int(rng.integers(0, len(t)))
    j = min(i + 1, len(t) - 1)
    tight = [k for k in range(len(t) - 1) if 0.0 < t[k + 1] - t[k] <= 1.5 * tol]
    k = tight[0] if tight else i
    return (0.5 * (t[i] + t[j]), t[i], t[k] + 0.5 * (t[min(k + 1, len(t) - 1)] - t[k]), t[i] - 0.5 * tol, t[0] - 1e-3,
            t[-1] + 1e-3, t[i] + 0.5 * tol, t[-1], 0.25 * t[i] + 0.75 * t[j])[variant % 9]


KINDS = ("insert", "discard", "append", "insert", "discard", "insert", "add_offset", "discard", "insert", "append",
         "discard", "insert", "clear", "insert", "discard")


class ReferenceBackend:
    """The backend interface of run_program / compare_ticks / compare_pack on a ReferenceSet (what
    the CPU test mutates, and what the generators run a program on)."""

    def __init__(self, program, buffer_class=Buffer):
        self.set = ReferenceSet(program["B"], program["D"], program["tolerance"],
                                None if program.get("grows") else program["capacity"], buffer_class)
        self.room = program["capacity"]

    def apply(self, rnd):
        return self.set.apply(rnd)

    def download(self, ids=None, capacity=None):
        """Without a capacity the reference's lists; with one, as a device entry fills the
        caller's arrays: `capacity` rows of SENTINEL, written only if the rows fit."""
        if capacity is None:
            return self.set.download(ids)
        offsets = pack_offsets(self.set.buffers, ids)
        out = dict(offsets=offsets)
        fits = offsets[-1] <= capacity
        for k, w in (("t", 1), ("q", self.set.D), ("qd", self.set.D), ("qdd", self.set.D)):
            out[k] = np.full(capacity * w, SENTINEL)
            if fits:
                rows = np.frombuffer(pack_bytes(self.set.buffers, ids, k), dtype=np.float64)
                out[k][:len(rows)] = rows
        return out

    def info(self, ids, time_ns):
        return self.set.info(ids, time_ns)

    def ticks(self, ids, start_ns, step_ns, T, want=(True, True, True)):
        return self.set.ticks(ids, start_ns, step_ns, T, want)

    def capacity(self):
        return self.room


@functools.lru_cache(maxsize=None)
def operation_program(D, repeat=False):
    """The operation program the tests use for D joints (`repeat`: with repeated stamps): the
    first of the seeded programs on which the reference meets a compaction (by the layout model of
    run_program); a fit that fills the capacity exactly is met by every one of them."""
    for attempt in range(20):
        program = make_operation_program(D, seed=20261020 + 7919 * attempt, repeat=repeat)
        stats = collections.Counter()
        run_program(ReferenceBackend(program), program, stats=stats)
        if stats["compactions"] and stats["tight_fits"]:
            return program
    raise AssertionError("no program with a compaction for D = %d" % D)


def make_operation_program(D, seed=20261020, B=BUFFERS, rounds=ROUNDS, tolerance=TIMESTEP_TOLERANCE, repeat=False):
    """An operation program of D joints: `rounds` rounds on B buffers, each one call (kind, ids,
    one entry per listed buffer, unit "sec" / "ns"). The arguments are chosen on a reference set so
    that every branch of InsertSegment, AppendSample and DiscardSegmentBefore is met; the last
    rounds leave some buffers empty and some with stamps on whole nanoseconds (for the ticks).
    Returns dict B, D, tolerance, rounds, capacity (the largest count the reference reaches)."""
    rng = np.random.default_rng(seed + 1000 * D + (500 if repeat else 0))
    ref = ReferenceSet(B, D, tolerance)
    out, cap, uses = [], 0, {}

    def emit(rnd):
        nonlocal cap
        ref.apply(rnd)
        out.append(rnd)
        cap = max(cap, max(b.num_samples() for b in ref.buffers))

    first = [make_segment(rng, D, int(rng.integers(2, 41)) if b % 6 else 0, 1.0 + 0.01 * b, tolerance, tight=b % 2 == 1,
                          repeat=repeat and b % 3 == 0) for b in range(B)]
    emit(dict(kind="insert", ids=None, unit="sec", entries=first))
    for r in range(rounds):
        kind = KINDS[r % len(KINDS)]
        ids, listed = _pick_ids(rng, B)
        uses[kind] = uses.get(kind, 0) + 1
        unit = "ns" if uses[kind] % 2 == 0 and kind in ("discard", "add_offset") else "sec"
        entries = []
        for e, b in enumerate(listed):
            buf, v = ref.buffers[b], r + e
            if kind == "insert":
                n = 0 if v % 11 == 5 else int(rng.integers(1, 41))
                entries.append(make_segment(rng, D, n, _insert_front(rng, buf, v, tolerance), tolerance, tight=v % 3 == 0,
                                            repeat=repeat and v % 4 == 0))
            elif kind == "append":
                last = buf.t[-1] if buf.t else 1.0
                t = (last + 1e-3, last, last + 1.2 * tolerance, last - 1e-3)[v % 4]
                entries.append(dict(t=t, q=_values(rng, 1, D)[0], qd=_values(rng, 1, D)[0], qdd=_values(rng, 1, D)[0]))
            elif kind == "discard":
                x = _discard_time(rng, buf, v, tolerance)
                entries.append(dict(ns=int(round(x * 1e9))) if unit == "ns" else dict(sec=x))
            elif kind == "add_offset":
                x = float(rng.uniform(-0.25, 0.25))
                entries.append(dict(ns=int(round(x * 1e9))) if unit == "ns" else dict(sec=x))
            else:
                entries.append({})
        emit(dict(kind=kind, ids=ids, unit=unit, entries=entries))
    # the end: every third buffer cleared, and two of three of those refilled on the nanosecond grid
    cleared = [b for b in range(B) if b % 3 == 0]
    emit(dict(kind="clear", ids=cleared, unit="sec", entries=[{} for _ in cleared]))
    refill = [b for b in cleared if b % 9]
    emit(dict(kind="insert", ids=refill, unit="sec",
              entries=[grid_segment(rng, D, int(rng.integers(3, 41)), 2_000_000_000 + 7_000_000 * b) for b in refill]))
    return dict(B=B, D=D, tolerance=tolerance, rounds=out, capacity=cap)


def tolerance_program(D, seed=20261021):
    """Differences exactly equal to the tolerance: timestep_tolerance = 2^-20 and stamps that are
    multiples of 2^-24 in [1, 2), where one ulp is 2^-52 and every difference below is exact.
    Buffer pairs (even, odd) get the argument on the boundary and one ulp beside it:
      insert front at prev + tol (not kept-less: the difference is not < tol) and one ulp below;
      discard at prev + tol (close: <=) and one ulp above (interpolated or on the next sample);
      discard at next - tol (|t[offset] - time| == tol: no interpolation) and one ulp below."""
    tol, ulp, g = 2.0 ** -20, 2.0 ** -52, 2.0 ** -24
    rng = np.random.default_rng(seed + D)
    B = 12
    seg = lambda n, front, step: dict(t=[front + i * step for i in range(n)], q=_values(rng, n, D), qd=_values(rng, n, D),
                                      qdd=_values(rng, n, D))
    rounds = [dict(kind="insert", ids=None, unit="sec", entries=[seg(12, 1.0 + b * g, 64 * g) for b in range(B)])]
    base = [1.0 + b * g for b in range(B)]
    prev = lambda b, i: base[b] + i * 64 * g
    # buffers 0-3: insert fronts around sample 5 + tol
    fronts = [prev(0, 5) + tol, prev(1, 5) + tol - ulp, prev(2, 0) + tol, prev(3, 0) + tol - ulp]
    rounds.append(dict(kind="insert", ids=[0, 1, 2, 3], unit="sec", entries=[seg(4, f, 64 * g) for f in fronts]))
    # buffers 4-7: discard just behind sample 3 (the next sample is far: the time is interpolated unless close),
    # buffers 8-11: discard a tolerance before sample 6
    times = [prev(4, 3) + tol, prev(5, 3) + tol + ulp, prev(6, 3) + tol, prev(7, 3) + tol + ulp,
             prev(8, 6) - tol, prev(9, 6) - tol - ulp, prev(10, 6) - tol, prev(11, 6) - tol - ulp]
    rounds.append(dict(kind="discard", ids=list(range(4, 12)), unit="sec", entries=[dict(sec=x) for x in times]))
    # a pair of stamps 1.5 tol apart (one ulp is 2^-51 there), so that no interpolation hides `close`:
    # a tolerance behind the first (close: it stays), one ulp more (not close: on the next sample),
    # half a tolerance behind it, and far behind both
    tight = [dict(t=[3.0, 3.0 + 1.5 * tol, 3.5, 4.0], q=_values(rng, 4, D), qd=_values(rng, 4, D), qdd=_values(rng, 4, D))
             for _ in range(4)]
    rounds.append(dict(kind="insert", ids=[0, 1, 2, 3], unit="sec", entries=tight))
    rounds.append(dict(kind="discard", ids=[0, 1, 2, 3], unit="sec",
                       entries=[dict(sec=3.0 + tol), dict(sec=3.0 + tol + 2 * ulp), dict(sec=3.0 + 0.5 * tol),
                                dict(sec=3.25)]))
    return dict(B=B, D=D, tolerance=tol, rounds=rounds, capacity=16)


def layout_cases(D):
    """(K, first) of the layout cases of D joints: kept-row counts K with K D just below, at (where
    D divides) and just above 256 and 512 doubles (the copy chunk is 256 doubles), and shifts
    `first` of one row, under one chunk, at least one chunk, and more than K rows (no overlap)."""
    ks = []
    for target in (256, 512):
        ks += [(target - 1) // D, target // D + 1] + ([target // D] if target % D == 0 else [])
    ks = sorted(set(k for k in ks if k >= 1))
    cases = []
    for K in ks:
        for first in sorted({1, max(1, 200 // D), 256 // D + 1, K + 1}):
            cases.append((K, first))
    return cases


def layout_program(D, seed=20261022, host=False):
    """One buffer per layout case, one call per step: a whole-buffer insert of K + first rows, a
    discard exactly on sample `first` (OnSample: no row is rewritten), then
      device sets: an insert one row too long (MORE, nothing changes), the insert whose result is
        exactly `capacity` rows (possible only through compaction), and on a second half of the
        buffers an insert that fills the tail, an append (compaction) and, for the cases with
        first == 1, a further append (MORE);
      host-entry sets (`host`): the exact fit (compaction), then everything again with the insert one
        row too long, which makes the set grow with first > 0.
    Returns the program and `expect`: per round and entry whether the step must compact."""
    rng = np.random.default_rng(seed + D)
    cases = layout_cases(D)
    C = len(cases)
    cap = max(K + f for K, f in cases) + 3
    B = C if host else 2 * C
    both = cases if host else cases + cases
    whole = lambda: [grid_segment(rng, D, K + f, 1_000_000_000) for K, f in both]
    tail = lambda n, b: make_segment(rng, D, n, 900.0 + b)        # behind every stamp: keeps all
    rounds, expect = [], []

    def emit(rnd, compacts=None):
        rounds.append(rnd)
        expect.append(compacts)

    def prepare():
        segs = whole()
        emit(dict(kind="insert", ids=None, unit="sec", entries=segs))
        emit(dict(kind="discard", ids=None, unit="sec", entries=[dict(sec=s["t"][f]) for s, (K, f) in zip(segs, both)]))

    prepare()
    if host:
        emit(dict(kind="insert", ids=None, unit="sec", entries=[tail(cap - K, b) for b, (K, f) in enumerate(cases)]),
             [True] * C)
        emit(dict(kind="clear", ids=None, unit="sec", entries=[{} for _ in cases]))
        prepare()
        emit(dict(kind="insert", ids=None, unit="sec", entries=[tail(cap - K + 1, b) for b, (K, f) in enumerate(cases)]))
        return dict(B=B, D=D, tolerance=TIMESTEP_TOLERANCE, rounds=rounds, capacity=cap, expect=expect, cases=cases,
                    grows=True)
    ins = list(range(C))
    app = list(range(C, 2 * C))
    emit(dict(kind="insert", ids=ins, unit="sec", entries=[tail(cap - K + 1, b) for b, (K, f) in enumerate(cases)]))
    emit(dict(kind="insert", ids=ins, unit="sec", entries=[tail(cap - K, b) for b, (K, f) in enumerate(cases)]), [True] * C)
    emit(dict(kind="insert", ids=app, unit="sec", entries=[tail(cap - K - f, b) for b, (K, f) in enumerate(cases)]))
    one = lambda b: dict(t=1900.0 + b, q=_values(rng, 1, D)[0], qd=_values(rng, 1, D)[0], qdd=_values(rng, 1, D)[0])
    emit(dict(kind="append", ids=app, unit="sec", entries=[one(b) for b in range(C)]), [True] * C)
    full = [C + b for b, (K, f) in enumerate(cases) if f == 1]
    emit(dict(kind="append", ids=full, unit="sec", entries=[one(100 + b) for b in range(len(full))]))
    return dict(B=B, D=D, tolerance=TIMESTEP_TOLERANCE, rounds=rounds, capacity=cap, expect=expect, cases=cases)


def on_stamp_ns(x):
    """The nanosecond count whose TimeToSec is the stamp x, or None."""
    for ns in (int(round(x * 1e9)) + d for d in (0, -1, 1)):
        if time_to_sec(ns) == x:
            return ns
    return None


def tick_requests(buffers, count, rng, B=None, bad_ids=True):
    """`count` entries (id, start_ns) over the buffers: starts on the first stamp, on the last
    stamp, 1 ns before and after each, far outside and inside; ids with repeats and, if `bad_ids`,
    -1 and B; the last entry starts near INT64_MAX."""
    B = len(buffers) if B is None else B
    ids, starts = [], []
    grid = [b for b in range(B) if buffers[b].t and None not in (on_stamp_ns(buffers[b].t[0]), on_stamp_ns(buffers[b].t[-1]))]
    empty = [b for b in range(B) if not buffers[b].t]
    order = grid[:7] + empty[:2] + [int(x) for x in rng.permutation(B) if x not in grid[:7] + empty[:2]]
    for e in range(count):
        b = order[e % B] if e % 5 else order[(e // 5) % B]       # repeats
        t = buffers[b].t
        if bad_ids and e in (3, 11):
            ids.append(-1 if e == 3 else B)
            starts.append(1_000_000_000)
            continue
        if not t:
            ids.append(b)
            starts.append(1_000_000_000)
            continue
        lo, hi = on_stamp_ns(t[0]), on_stamp_ns(t[-1])
        lo = int(t[0] * 1e9) if lo is None else lo
        hi = int(t[-1] * 1e9) if hi is None else hi
        starts.append((lo, hi, lo - 1, lo + 1, hi - 1, hi + 1, lo - 10 ** 12, hi + 10 ** 12, (lo + hi) // 2)[e % 9])
        ids.append(b)
    starts[-1] = INT64_MAX - 5
    return ids, starts


def repeated_stamp_ticks(buffers):
    """(ids, start_ns) of ticks 1 ns before each pair of equal consecutive stamps (three ticks of
    1 ns then fall before, about on and behind the pair)."""
    ids, starts = [], []
    for b, buf in enumerate(buffers):
        for i in range(len(buf.t) - 1):
            if buf.t[i] == buf.t[i + 1]:
                ids.append(b)
                starts.append(int(round(buf.t[i] * 1e9)) - 1)
    return ids, starts


def id_list(rng, length, B, bad=True):
    """`length` ids over B buffers with repeats and, if `bad`, a few outside [0, B)."""
    ids = [int(x) for x in rng.integers(0, B, size=length)]
    if bad:
        for k in range(5, length, 97):
            ids[k] = -1 if k % 2 else B + k % 3
    return ids


# ------------------------------------------------------------------ 3: the C-ABI layout
def pack_entries(rnd, D):
    """The arrays of one round as the C-ABI takes them (numpy): insert: offsets int64 [n + 1], time
    [rows], q / qd / qdd [rows][D]; append: time [n], q / qd / qdd [n][D]; discard / add_offset: ns
    int64 [n] or sec [n]."""
    e = rnd["entries"]
    f = lambda rows: np.asarray(rows, dtype=np.float64).reshape(-1, D)
    if rnd["kind"] == "insert":
        off = np.concatenate([[0], np.cumsum([len(x["t"]) for x in e])]).astype(np.int64)
        return dict(offsets=off, time=np.asarray([v for x in e for v in x["t"]], dtype=np.float64),
                    **{k: f([r for x in e for r in x[k]]) for k in ARRAYS})
    if rnd["kind"] == "append":
        return dict(time=np.asarray([x["t"] for x in e], dtype=np.float64), **{k: f([x[k] for x in e]) for k in ARRAYS})
    if rnd["kind"] in ("discard", "add_offset"):
        return dict(ns=np.asarray([x["ns"] for x in e], dtype=np.int64)) if rnd["unit"] == "ns" else \
            dict(sec=np.asarray([x["sec"] for x in e], dtype=np.float64))
    return {}


# ------------------------------------------------------------------ 3: the comparison
def _snapshots(down, seq, B, D):
    """Per buffer the snapshot (dict t, q, qd, qdd, seq) of a download of buffers 0 .. B-1."""
    off = down["offsets"]
    out = []
    for b in range(B):
        lo, hi = off[b], off[b + 1]
        rows = lambda k: [list(down[k][i * D:(i + 1) * D]) for i in range(lo, hi)]
        out.append(dict(t=list(down["t"][lo:hi]), q=rows("q"), qd=rows("qd"), qdd=rows("qdd"), seq=seq[b]))
    return out


def compare_download(want, got, where):
    assert list(got["offsets"]) == list(want["offsets"]), where + ("offsets",)
    for k in ("t",) + ARRAYS:
        assert bits(got[k]) == bits(want[k]), where + ("download", k)


def info_times(buffers, r):
    """One query time (ns) per buffer for GetPositionsUpToTime: on, beside and outside the stamps."""
    out = []
    for b, buf in enumerate(buffers):
        if not buf.t:
            out.append(1_000_000_000)
            continue
        lo, hi = int(buf.t[0] * 1e9), int(buf.t[-1] * 1e9)
        mid = int(buf.t[len(buf.t) // 2] * 1e9)
        out.append((lo, lo + 1, hi, hi + 1, lo - 1, mid, mid + 1, hi - 1, hi + 10 ** 9)[(b + r) % 9])
    return out


def run_program(backend, program, seen=None, stats=None):
    """Runs the program on `backend` (apply(rnd) -> statuses, download() -> dict offsets / t / q /
    qd / qdd of buffers 0 .. B-1, info(ids, time_ns) -> dict count / seq / start_ns / end_ns /
    up_to) next to a ReferenceSet and asserts after every round: equal statuses, a bit-equal packed
    download, equal info, and the exact checkers on the backend's own states. `seen` (Counter)
    receives the outcome names of the backend's results; `stats` counts compactions by a model of
    the first row (tpamd_buffer.h: a whole replacement restarts at row 0, a discard advances the
    first row, an insert or append that would end behind row `capacity` compacts), which judges
    nothing. Returns the reference set."""
    B, D, tol, room = program["B"], program["D"], program["tolerance"], program["capacity"]
    cap = None if program.get("grows") else room       # a host-entry set grows where a device set says MORE
    ref = ReferenceSet(B, D, tol, cap)
    first = [0] * B
    before = _snapshots(ref.download(), [0] * B, B, D)
    for r, rnd in enumerate(program["rounds"]):
        where = (D, "round", r, rnd["kind"])
        want = ref.apply(rnd)
        got = backend.apply(rnd)
        assert list(got) == want, where + ("status", list(got), want)
        if backend.capacity() != room:                   # a host-entry set has grown: every buffer restarts at row 0
            room, first = backend.capacity(), [0] * B
        wd, gd = ref.download(), backend.download()
        compare_download(wd, gd, where)
        times = info_times(ref.buffers, r)
        wi, gi = ref.info(None, times), backend.info(None, times)
        for k in wi:
            assert list(gi[k]) == wi[k], where + ("info", k)
        after = _snapshots(gd, list(gi["seq"]), B, D)
        ids = rnd["ids"] if rnd["ids"] is not None else range(len(rnd["entries"]))
        listed = set()
        for e, b in enumerate(ids):
            listed.add(b)
            args = (before[b], rnd["kind"], rnd["entries"][e], rnd["unit"], got[e], after[b])
            check_buffer_invariants(*args, tolerance=tol, capacity=cap)
            if seen is not None:
                seen.update(classify(*args))
            # the layout model (counts compactions only)
            n0, n1 = len(before[b]["t"]), len(after[b]["t"])
            compacted = False
            added = 0 if got[e] != OK else 1 if rnd["kind"] == "append" else len(rnd["entries"][e].get("t", ())) \
                if rnd["kind"] == "insert" else 0
            if added:
                if n1 - added == 0:
                    first[b] = 0
                elif first[b] + n1 > room:
                    first[b], compacted = 0, True
            elif rnd["kind"] in ("discard", "clear"):
                first[b] = 0 if n1 == 0 else first[b] + n0 - n1
            if stats is not None:
                stats["compactions"] += compacted
                stats["tight_fits"] += n1 == room and rnd["kind"] in ("insert", "append") and got[e] == OK
                stats["more"] += got[e] == MORE
                if program.get("expect") and program["expect"][r] is not None:
                    assert compacted == program["expect"][r][e], where + ("planned compaction", e, b)
        for b in range(B):
            if b not in listed:
                assert _rows(after[b], 0, len(after[b]["t"])) == _rows(before[b], 0, len(before[b]["t"])) and \
                    after[b]["seq"] == before[b]["seq"], where + ("a buffer that is not listed stays", b)
        before = after
    return ref


def compare_ticks(ref, backend, ids, start_ns, step_ns, T, want=(True, True, True), seen=None, where=()):
    """sample_at_ticks of `backend` (ticks(ids, start_ns, step_ns, T, want) -> dict status and
    q / qd / qdd flat, pre-filled with SENTINEL) against the reference set: equal statuses, equal
    bits, SENTINEL wherever a tick is not OK, and check_setpoint on the backend's own values."""
    D = ref.D
    w, g = ref.ticks(ids, start_ns, step_ns, T, want), backend.ticks(ids, start_ns, step_ns, T, want)
    assert list(g["status"]) == w["status"], where + ("tick status",)
    listed = range(len(start_ns)) if ids is None else ids
    for k, wanted in zip(ARRAYS, want):
        if not wanted:
            continue
        assert bits(g[k]) == bits(w[k]), where + ("tick values", k)
        for e, b in enumerate(listed):
            buf = ref._buffer(b)
            for j in range(T):
                o = (e * T + j) * D
                row = list(g[k][o:o + D])
                if g["status"][e * T + j] != OK:
                    assert row == [SENTINEL] * D, where + ("a tick that is not OK writes nothing", e, j, k)
                else:
                    check_setpoint(buf.t, getattr(buf, k), time_to_sec(tick_time(start_ns[e], step_ns, j)), row)
    if seen is not None:
        for e, b in enumerate(listed):
            buf = ref._buffer(b)
            for j in range(T):
                seen[classify_tick(buf.t if buf else None, buf is not None, start_ns[e], step_ns, j,
                                   g["status"][e * T + j])] += 1


def pack_offsets(buffers, ids):
    """The running sum of the listed buffers' sample counts; an id outside the set counts 0."""
    offsets = [0]
    for b in ids:
        offsets.append(offsets[-1] + (len(buffers[b].t) if 0 <= b < len(buffers) else 0))
    return offsets


def pack_bytes(buffers, ids, key):
    """The bytes of the packed rows of one array ("t", "q", "qd", "qdd") of the listed buffers."""
    each = [bits(b.t if key == "t" else _flat(getattr(b, key))) for b in buffers]
    return b"".join(each[b] for b in ids if 0 <= b < len(buffers))


def compare_pack(ref, backend, ids, where=()):
    """The packed download of an id list (download(ids, capacity) -> dict offsets and t, q, qd,
    qdd of `capacity` rows pre-filled with SENTINEL): offsets equal the reference's running sum;
    with a capacity equal to the total the rows are bit-equal; with one row more room the row behind
    them keeps the SENTINEL; with one row less the offsets are still complete and no row is written."""
    want = pack_offsets(ref.buffers, ids)
    total = want[-1]
    g = backend.download(ids, total)
    assert list(g["offsets"]) == want, where + ("offsets", len(ids))
    for k in ("t",) + ARRAYS:
        assert bits(g[k]) == pack_bytes(ref.buffers, ids, k), where + ("rows", k, len(ids))
    g = backend.download(ids, total + 1)
    assert list(g["offsets"]) == want, where + ("offsets, a row to spare", len(ids))
    for k, w in (("t", 1), ("q", ref.D), ("qd", ref.D), ("qdd", ref.D)):
        assert bits(g[k][:total * w]) == pack_bytes(ref.buffers, ids, k), where + ("rows, a row to spare", k, len(ids))
        assert _all_sentinel(g[k][total * w:]), where + ("nothing behind the rows is written", k, len(ids))
    if total > 0:
        g = backend.download(ids, total - 1)
        assert list(g["offsets"]) == want, where + ("offsets, one row short", len(ids))
        for k in ("t",) + ARRAYS:
            assert _all_sentinel(g[k]), where + ("one row short: nothing is written", k, len(ids))


# ------------------------------------------------------------------ 3: what both tests run
TICK_STEP_NS = 300_000
PACK_LENGTHS = (0, 1, 1023, 1024, 1025, 2049, 2500)


def run_ticks(ref, backend, rng, seen=None, bad_ids=True, null_arrays=False, where=()):
    """The setpoint ticks on the buffers a program left: 37 x 7 ticks (the last block of 256 partly
    filled) and 32 x 8 (exactly full), starts on and 1 ns beside the first and last stamps and far
    outside, empty buffers, repeated ids and (`bad_ids`) ids -1 and B, a start near INT64_MAX, a
    step of 2^62 ns whose product overflows, and (`null_arrays`) each of q, qd, qdd left out in turn."""
    for count, T in ((37, 7), (32, 8)):
        ids, starts = tick_requests(ref.buffers, count, rng, bad_ids=bad_ids)
        compare_ticks(ref, backend, ids, starts, TICK_STEP_NS, T, seen=seen, where=where + (count, T))
    ids, starts = tick_requests(ref.buffers, 5, rng, bad_ids=False)
    compare_ticks(ref, backend, ids, starts, 2 ** 62, 4, seen=seen, where=where + ("step 2^62",))
    # every buffer whose end stamps are whole nanoseconds, on its last and on its first stamp: one
    # joint alone shows a last sample that was interpolated, not copied, only now and then
    grid = [b for b in range(ref.B) if ref.buffers[b].t and
            None not in (on_stamp_ns(ref.buffers[b].t[0]), on_stamp_ns(ref.buffers[b].t[-1]))]
    starts = [on_stamp_ns(ref.buffers[b].t[-1]) for b in grid] + [on_stamp_ns(ref.buffers[b].t[0]) for b in grid]
    compare_ticks(ref, backend, grid + grid, starts, TICK_STEP_NS, 2, seen=seen, where=where + ("on the end stamps",))
    if null_arrays:
        ids, starts = tick_requests(ref.buffers, 9, rng, bad_ids=bad_ids)
        for skip in range(3):
            compare_ticks(ref, backend, ids, starts, TICK_STEP_NS, 3, want=tuple(a != skip for a in range(3)),
                          where=where + ("without", ARRAYS[skip]))


def run_packs(ref, backend, rng, bad_ids=True, lengths=PACK_LENGTHS, where=()):
    """The packed download over id lists of the lengths around the 1024 threads of the offset scan."""
    for n in lengths:
        compare_pack(ref, backend, id_list(rng, n, ref.B, bad=bad_ids), where=where)

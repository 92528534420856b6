"""What the two resamplers and the s(t) query compute, restated independently of the kernels.

A restatement in Python floats (IEEE doubles), one scalar operation per operation of the
reference and in its order, of

  * TimeAtPathSamplesLowerIndex, InterpolateAtTime, ResampleEquidistantlyInTime and
    ResampleSkippingSamplesCloserThanTimeStep (trajectory_planning/path_timing_trajectory.cc
    :686-695, :709-753, :755-783, :785-836, with GetMinTimeDeltaToKeep :893-900), and
  * GetPathParameterAndDerivatives with SampleIndexFromTime
    (trajectory_planning/time_optimal_path_timing.cc:1549-1627, :1497-1524, with low_idx_ and
    high_idx_ as :468-477 sets them).

Each function cites the lines it follows. It is written from those sources, not from
oracle/tp_oracle.c or csrc/tpamd_kernels.h, so that a misreading shared by oracle and kernels does
not pass. No numpy arithmetic and no fused multiply-add: every `+`, `-`, `*`, `/` below rounds once.

Two things the reference's text cannot pin:

  * eigenmath::InterpolateLinear is not in the reference's tree. It is restated as
    a + t * (b - a): the same choice, with the same caveat, as DESIGN.md records for the oracle and
    the kernels (ulp-level parity of interpolated values unpinned). lerp_exact_bound below states
    how far any reasonable order of operations can be from the exact value.
  * ResampleEquidistantlyInTime with a start more than a time step past the end has no samples
    (`positions_.back()` of an empty vector): resample_uniform then returns the count, which is
    <= 0, and no samples.

ds_, s_start_ and s_end_ of the query come from the s row as include/tpamd.h documents: s[0] is
s_start_, s[N - 1] is s_end_ (.cc:544-547) and (s_end_ - s_start_) / (N - 1) repeats the division
that formed ds_ (.cc:540).

Plain Python; no GPU, no product imports.
"""
import math
import sys
from fractions import Fraction

EPSILON = sys.float_info.epsilon          # std::numeric_limits<double>::epsilon()
UNIT_ROUNDOFF = 2.0 ** -53


def interpolate_linear(t, a, b):
    """eigenmath::InterpolateLinear(t, a, b), restated (see the module docstring): unpinned."""
    return a + t * (b - a)


# ------------------------------------------------------------------ path_timing_trajectory.cc
def lower_index(time, start_index, t):
    """TimeAtPathSamplesLowerIndex, :686-695: the serial scan from start_index."""
    index = start_index
    while index < len(time) - 1:                            # :688-689
        if time[index + 1] > t:                             # :690
            return index                                    # :691
        index += 1
    return len(time) - 1                                    # :694


def interpolate_at_time(time, s, sd, sdd, q, qd, qdd, amax, time_sec, start_index):
    """InterpolateAtTime, :709-753. q, qd, qdd are [N][D] rows, amax [D]. Returns a dict:
    lower_index, upper_index, interpolate_at, position / velocity / acceleration [D],
    path_parameter and its two derivatives; and, for the tests' reach checks only, `half` (the
    bracket was shorter than epsilon) and `clamped` [D] (the acceleration limit acted)."""
    lower = lower_index(time, start_index, time_sec)        # :713
    upper = min(len(time) - 1, lower + 1)                   # :714-715
    half = abs(time[upper] - time[lower]) < EPSILON         # :717-719
    if half:
        at = 0.5                                            # :720
    else:
        at = (time_sec - time[lower]) / (time[upper] - time[lower])     # :721-723
    D = len(amax)
    position = [interpolate_linear(at, q[lower][d], q[upper][d]) for d in range(D)]       # :725-727
    velocity = [interpolate_linear(at, qd[lower][d], qd[upper][d]) for d in range(D)]     # :729-731
    acceleration, clamped = [], []
    for d in range(D):
        a = interpolate_linear(at, qdd[lower][d], qdd[upper][d])        # :736-738
        c = a
        if c < -amax[d]:                                    # :739 cwiseMax(-max acceleration)
            c = -amax[d]
        if c > amax[d]:                                     # :740 cwiseMin(max acceleration)
            c = amax[d]
        acceleration.append(c)
        clamped.append(c != a)
    return dict(lower_index=lower, upper_index=upper, interpolate_at=at, half=half, clamped=clamped,
                position=position, velocity=velocity, acceleration=acceleration,
                path_parameter=interpolate_linear(at, s[lower], s[upper]),                     # :742-744
                path_parameter_derivative=interpolate_linear(at, sd[lower], sd[upper]),        # :745-747
                second_path_parameter_derivative=interpolate_linear(at, sdd[lower], sdd[upper]))  # :748-750


def uniform_count(end_time, start_sec, time_step):
    """:756-757; the conversion to int truncates."""
    duration = end_time - start_sec
    return int(math.ceil(duration / time_step) + 1)


def _push(out, time, r):
    out[0].append(time)
    out[1].append(r["path_parameter"])
    out[2].append(r["path_parameter_derivative"])
    out[3].append(r["second_path_parameter_derivative"])
    out[4].append(r["position"])
    out[5].append(r["velocity"])
    out[6].append(r["acceleration"])


def resample_uniform(time, s, sd, sdd, q, qd, qdd, start_sec, time_step, amax, max_out=None, trace=None):
    """ResampleEquidistantlyInTime, :755-783. Returns (count, samples): count is uniform_samples
    as an int, also when it is <= 0 (then samples are empty); samples = (time, s, sd, sdd, q, qd,
    qdd), lists with min(count, max_out) entries. max_out has the C-ABI's meaning: count reports
    the full number, only the first max_out samples exist, and the end sample (:780-782) is special
    only if it is among them. `trace`, if a list, receives interpolate_at_time's dict per tick."""
    count = uniform_count(time[-1], start_sec, time_step)   # :756-757
    out = ([], [], [], [], [], [], [])
    if count <= 0:
        return count, out
    written = count if max_out is None else min(count, max_out)
    lower = 0                                               # :766
    for i in range(written):                                # :767
        t = start_sec + time_step * i                       # :768
        r = interpolate_at_time(time, s, sd, sdd, q, qd, qdd, amax, t, lower)   # :769
        lower = r["lower_index"]                            # :770
        _push(out, t, r)                                    # :771-778
        if trace is not None:
            trace.append(r)
    if written == count:
        D = len(amax)
        out[4][-1] = [q[-1][d] for d in range(D)]           # :780
        out[5][-1] = [0.0] * D                              # :781
        out[6][-1] = [0.0] * D                              # :782
    return count, out


def resample_skip(time, s, sd, sdd, q, qd, qdd, start_sec, time_step, amax, max_out=None, trace=None):
    """ResampleSkippingSamplesCloserThanTimeStep, :785-836. Returns (count, samples) as
    resample_uniform does. `trace`, if a list, receives the first sample's dict and then the kept
    indices."""
    lower = lower_index(time, 0, start_sec)                 # :787
    min_delta = 0.95 * time_step                            # :805 with :899
    r = interpolate_at_time(time, s, sd, sdd, q, qd, qdd, amax, start_sec, lower)   # :808
    out = ([], [], [], [], [], [], [])
    _push(out, start_sec, r)                                # :809-817
    if trace is not None:
        trace.append(r)
    for i in range(lower + 1, len(time)):                   # :818
        if abs(time[i] - out[0][-1]) < min_delta:           # :820
            continue
        out[0].append(time[i])                              # :823-830
        out[1].append(s[i])
        out[2].append(sd[i])
        out[3].append(sdd[i])
        out[4].append(list(q[i]))
        out[5].append(list(qd[i]))
        out[6].append(list(qdd[i]))
        if trace is not None:
            trace.append(i)
    D = len(amax)
    out[4][-1] = [q[-1][d] for d in range(D)]               # :833
    out[5][-1] = [0.0] * D                                  # :834
    out[6][-1] = [0.0] * D                                  # :835
    count = len(out[0])
    if max_out is not None and max_out < count:             # the C-ABI's cut: the end sample is not among them
        out = tuple(x[:max_out] for x in out)
    return count, out


def lerp_exact_bound(time_lower, time_upper, time_sec, a, b):
    """One interpolated value of InterpolateAtTime from the bracket (time_lower, time_upper) and
    the two sample values a, b, evaluated exactly with fractions.Fraction: the exact
    at = (time_sec - time_lower) / (time_upper - time_lower) (1/2 under the epsilon rule, which is
    decided on the rounded difference as the reference decides it) and the exact a + at (b - a).
    Returns (value, bound), value a Fraction and

        bound = 8 u (|a| + max(1, |at|) |b - a|),   u = 2^-53.

    Derivation (first order in u; every rounding is at most u relative, no underflow at the
    magnitudes used here). The product at (b - a) is reached through five roundings: the two time
    differences, their quotient, the difference b - a and the product, so it carries a relative
    error of at most 5 u. The final sum rounds once more: u (|a| + |at| |b - a|). Together

        |computed - exact| <= u |a| + 6 u |at| |b - a| + O(u^2),

    which any order of the same operations (a (1 - at) + at b, a fused multiply-add) also meets.
    8 u (|a| + max(1, |at|) |b - a|) is that with less than a factor two of slack (8 / 6 on the
    product term), enough for the second-order terms; max(1, |at|) keeps the bound from vanishing
    with at where b - a itself was rounded. The bound is derived, not measured. (The issue that
    asked for this bound lists five roundings -- two differences, the quotient, the product, the
    sum; the count above also has the difference b - a, six in all. The bound is the same.)"""
    if abs(time_upper - time_lower) < EPSILON:
        at = Fraction(1, 2)
    else:
        at = (Fraction(time_sec) - Fraction(time_lower)) / (Fraction(time_upper) - Fraction(time_lower))
    a, b = Fraction(a), Fraction(b)
    value = a + at * (b - a)
    bound = 8 * Fraction(UNIT_ROUNDOFF) * (abs(a) + max(Fraction(1), abs(at)) * abs(b - a))
    return value, bound


# ------------------------------------------------------------------ time_optimal_path_timing.cc
def search_bounds(time):
    """low_idx_ and high_idx_, :468-477, as written (for a row whose times are all equal the
    reference reads time_[-1]; Python's wrap-around index ends that loop just the same, and the
    query never gets to the search on such a row)."""
    n = len(time)
    low = 0                                                 # :468
    while time[low] == time[low + 1] and low < n - 2:       # :469-470
        low += 1                                            # :471
    high = n - 1                                            # :473
    while time[high] == time[high - 1] and high >= low:     # :474-475
        high -= 1                                           # :476
    return low, high


def sample_index_from_time(time, t):
    """SampleIndexFromTime, :1497-1524, the search as the reference writes it."""
    n = len(time)
    if t <= time[0]:                                        # :1499-1501
        return 0
    if t >= time[n - 1]:                                    # :1502-1504
        return n - 2
    low, high = search_bounds(time)                         # :1506-1507
    mid = (low + high) // 2                                 # :1508 (non-negative: C's division)
    trips = 0
    while t < time[mid] or t >= time[mid + 1]:              # :1509
        if t < time[mid]:                                   # :1510-1514
            high = mid
        else:
            low = mid
        mid = (low + high) // 2                             # :1515
        trips += 1
        if trips > 2 * n:
            raise RuntimeError("SampleIndexFromTime does not end on this row (times not sorted?)")
    # :1519-1522; the reference reads time_[mid + 1] before it tests mid, the test comes first here
    while mid < n - 1 and time[mid] == time[mid + 1]:
        mid += 1
    return mid


def query(time, s, sd, sd2, t, trace=None):
    """GetPathParameterAndDerivatives, :1549-1627, on one solved row. Returns (ok, s, sd, sdd);
    where the reference returns false it leaves its outputs alone: (False, None, None, None).
    `trace`, if a dict, receives branch (one of start, end, equal_time, moving, zero_velocity,
    invalid), k, low_idx, high_idx, clamped (`ds > ds_` acted) and saturated (s_[k + 1] was the
    smaller one) -- for the tests' reach checks, nothing of it flows into the result.
    The search leaves its loop only on time[mid] <= t < time[mid + 1], so for a finite t the
    equal-time skip loop and the equal_time branch never act; they are restated all the same.
    A NaN leaves the loop at the first midpoint: times that are not finite are out of scope."""
    n = len(time)
    s_start, s_end = s[0], s[n - 1]
    ds_ = (s_end - s_start) / (n - 1)                       # :540
    inv_ds = 1.0 / ds_                                      # :542
    tr = {} if trace is None else trace
    tr.update(branch=None, k=None, clamped=False, saturated=False)
    tr["low_idx"], tr["high_idx"] = search_bounds(time)
    if t <= time[0]:                                        # :1562-1568
        tr["branch"] = "start"
        return True, s_start, sd[0], 0.5 * inv_ds * (sd2[1] - sd2[0])
    if t >= time[n - 1]:                                    # :1569-1575
        tr["branch"] = "end"
        return True, s_end, sd[n - 1], 0.0
    k = sample_index_from_time(time, t)                     # :1576
    tr["k"] = k
    if time[k] == time[k + 1]:                              # :1578-1584
        tr["branch"] = "equal_time"
        return True, s[k + 1], sd[k + 1], 0.5 * inv_ds * (sd2[k + 1] - sd2[k])
    dt = t - time[k]                                        # :1586
    if k > n - 2:                                           # :1588-1591
        tr["branch"] = "invalid"
        return False, None, None, None
    sda, sdb = sd[k], sd[k + 1]                             # :1596-1597
    sd2a, sd2b = sd2[k], sd2[k + 1]                         # :1598-1599
    if sda > 0 or sdb > 0:                                  # :1600
        ds = sda * dt + dt * dt * 0.25 * inv_ds * (sd2b - sd2a)         # :1601
        if ds > ds_:                                        # :1602-1604
            ds = ds_
            tr["clamped"] = True
        if dt < 0 or ds < 0:                                # :1605-1609
            tr["branch"] = "invalid"
            return False, None, None, None
        cand = s[k] + ds
        tr["saturated"] = s[k + 1] < cand
        rs = min(cand, s[k + 1])                            # :1612
        sqrt_arg = sd2a + ds * inv_ds * (sd2b - sd2a)       # :1613
        tr["branch"] = "moving"
        rsd = math.sqrt(sqrt_arg) if sqrt_arg >= 0 else math.nan        # :1614-1615; C's sqrt does not raise
        return True, rs, rsd, 0.5 * inv_ds * (sd2b - sd2a)              # :1616
    tr["branch"] = "zero_velocity"
    return True, s[k] + (s[k + 1] - s[k]) * dt / (time[k + 1] - time[k]), 0.0, 0.0       # :1619-1621

"""The fastest stop along a timed path (GetPathStopParameter / ComputeFastestStop,
path_timing_trajectory.cc:75-172, :235-287): a pure-Python restatement of the recurrence, checked
bit for bit against the mirror's host function (host/fastest_stop.cc) through a small C++ driver.
The GPU entries are checked against the same restatement in tests/test_gpu_fastest_stop.py."""
import math
import subprocess

import numpy as np
import pytest

from native_driver import build_driver

PLAN_OK, PLAN_INVALID_ARGUMENT = 0, 3


def compute_fastest_stop(time, qd, qdd, amax):
    """ComputeFastestStop on rows time[m], qd[m][D], qdd[m][D] (Python floats, IEEE doubles):
    returns (relative stop index, duration, profile time, rate2, drate2)."""
    m, D = len(time), len(amax)
    duration, rate2, drate2 = 0.0, 1.0, 0.0
    t0 = time[0]
    pt, pr, pd = [], [], []
    i = 0
    while i < m - 1 and rate2 > 0.0:
        v, a = qd[i], qdd[i]
        dmin = 0.0
        for dof in range(D):
            if abs(v[dof]) < 1e-6:
                continue
            bias = a[dof] * rate2
            for cand in (2.0 * (-bias - amax[dof]) / v[dof], 2.0 * (-bias + amax[dof]) / v[dof]):
                valid = True
                for j in range(D):
                    acc = a[j] * rate2 + (0.5 * v[j]) * cand
                    if not (amax[j] - acc >= -1e-10 and -amax[j] - acc <= 1e-10):
                        valid = False
                        break
                if valid and cand < dmin:
                    dmin = cand
        drate2 = 0.0 if 0.0 < dmin else dmin                 # std::min(dmin, 0.0)
        pt.append(t0 + duration)
        pr.append(rate2)
        pd.append(drate2)
        udt = time[i + 1] - time[i]
        x = rate2 + udt * drate2
        nxt = x if 0.0 < x else 0.0                           # std::max(0.0, x)
        duration += 2.0 * udt / (math.sqrt(rate2) + math.sqrt(nxt))
        rate2 = nxt
        i += 1
    pt.append(t0 + duration)
    pr.append(rate2)
    pd.append(drate2)
    return i, duration, pt, pr, pd


def fastest_stop_at_time(time, s, qd, qdd, amax, query):
    """GetPathStopParameter on one row of `count` = len(time) samples: (status, stop_parameter,
    stop_index, duration, profile time, rate2, drate2) as tpamd_fastest_stop_* defines them."""
    n = len(time)
    lo, hi = 0, n
    while lo < hi:                                           # lower_bound
        mid = (lo + hi) // 2
        if time[mid] < query:
            lo = mid + 1
        else:
            hi = mid
    if lo >= n:
        return PLAN_INVALID_ARGUMENT, 0.0, -1, 0.0, [], [], []
    k, dur, pt, pr, pd = compute_fastest_stop(time[lo:], qd[lo:], qdd[lo:], amax)
    return PLAN_OK, s[lo + k], lo + k, dur, pt, pr, pd


def synthetic_row(rng, count, D, still=False):
    """A timed row: increasing times (about 1 ms apart), increasing s, joint velocities and
    accelerations of robot-like size; still=True: every |qd| < 1e-6."""
    dt = 1e-3 * (0.5 + rng.random(count))
    time = list(np.cumsum(dt) + rng.random())
    s = list(np.cumsum(rng.random(count) * 1e-3))
    if still:
        qd = (rng.random((count, D)) - 0.5) * 1e-6
    else:
        qd = (rng.random((count, D)) - 0.5) * 2.0 * (0.5 + rng.random(D))
    qdd = (rng.random((count, D)) - 0.5) * 3.0
    amax = list(1.0 + 3.0 * rng.random(D))
    return time, s, [list(r) for r in qd], [list(r) for r in qdd], amax


def stop_cases(seed=7):
    """(time, s, qd, qdd, amax, query) cases: D in {1, 3, 7, 16}, queries before the first sample,
    on a sample, between samples, on the last sample and after the end, counts 0 and 1, and a
    row that never moves."""
    rng = np.random.default_rng(seed)
    cases = []
    for D in (1, 3, 7, 16):
        for count in (0, 1, 2, 5, 300):
            for still in (False, True):
                if still and count < 5:
                    continue
                time, s, qd, qdd, amax = synthetic_row(rng, count, D, still)
                queries = [-1.0, 0.0, 5.0]
                if count:
                    k = int(rng.integers(0, count))
                    queries += [time[0], time[k], 0.5 * (time[k] + time[min(k + 1, count - 1)]),
                                time[-1], time[-1] + 1e-9, time[0] - 1e-3]
                for q in queries:
                    cases.append((time, s, qd, qdd, amax, q))
    return cases


def test_restatement_edge_cases():
    """The restatement itself: a standing row runs to the end, a query after the last sample is
    out of range, a query on the last sample stops there with duration 0."""
    rng = np.random.default_rng(1)
    time, s, qd, qdd, amax = synthetic_row(rng, 50, 3, still=True)
    st, sp, idx, dur, pt, pr, pd = fastest_stop_at_time(time, s, qd, qdd, amax, time[0])
    assert st == PLAN_OK and idx == 49 and sp == s[49] and len(pt) == 50
    assert all(r == 1.0 for r in pr) and all(d == 0.0 for d in pd)
    assert fastest_stop_at_time(time, s, qd, qdd, amax, time[-1] + 1e-6)[0] == PLAN_INVALID_ARGUMENT
    st, sp, idx, dur, pt, pr, pd = fastest_stop_at_time(time, s, qd, qdd, amax, time[-1])
    assert (st, sp, idx, dur, len(pt)) == (PLAN_OK, s[-1], 49, 0.0, 1)
    assert fastest_stop_at_time([], [], [], [], amax, 0.0)[0] == PLAN_INVALID_ARGUMENT
    # a moving row brakes within the row
    time, s, qd, qdd, amax = synthetic_row(rng, 400, 3)
    st, sp, idx, dur, pt, pr, pd = fastest_stop_at_time(time, s, qd, qdd, amax, time[0])
    assert st == PLAN_OK and 0 < idx < 399 and pr[-1] == 0.0 and dur > 0.0


def test_mirror_matches_restatement_bit_for_bit(tmp_path):
    cases = stop_cases()
    inp = tmp_path / "cases.txt"
    with open(inp, "w") as f:
        f.write("%d\n" % len(cases))
        for time, s, qd, qdd, amax, q in cases:
            D = len(amax)
            f.write("%d %d %s\n" % (len(time), D, float(q).hex()))
            flat = list(time) + list(s) + [x for r in qd for x in r] + [x for r in qdd for x in r] + list(amax)
            f.write(" ".join(float(x).hex() for x in flat) + "\n")
    exe = build_driver("test_fastest_stop.cc", tmp_path, libs=("host", "engine"), opt="-O2")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == len(cases)
    seen = {"invalid": 0, "last": 0, "mid": 0, "end": 0}
    for (time, s, qd, qdd, amax, q), line in zip(cases, lines):
        tok = line.split()
        st, idx, n = int(tok[0]), int(tok[1]), int(tok[4])
        sp, dur = float.fromhex(tok[2]), float.fromhex(tok[3])
        prof = [float.fromhex(x) for x in tok[5:]]
        ref = fastest_stop_at_time(time, s, qd, qdd, amax, q)
        assert st == ref[0] and idx == ref[2], (len(time), len(amax), q)
        assert sp.hex() == float(ref[1]).hex() and dur.hex() == float(ref[3]).hex()
        assert n == len(ref[4])
        assert [x.hex() for x in prof] == [float(x).hex() for x in ref[4] + ref[5] + ref[6]]
        if st != PLAN_OK:
            seen["invalid"] += 1
        elif n == 1:
            seen["last"] += 1
        elif idx == len(time) - 1:
            seen["end"] += 1
        else:
            seen["mid"] += 1
    assert all(v > 0 for v in seen.values()), seen

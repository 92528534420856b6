"""The stops against an independent statement of what a stop is (tests/stop_reference.py), on the
CPU: the restatement of StopBeforeTime / StopAtIndex / RescaleTrajectoryBackwardToStop equals the
mirror (host/trajectory_buffer.cc, host/rescale_to_stop.cc) and the host-compilable code of the
kernels (rs_stop_serial of csrc/tpamd_rescale.h, bs_stop_in_place of csrc/tpamd_buffer.h) bit for
bit for every D = 1..16 on the cases the GPU tests use (tests/cpp/test_stop_reference.cc); the
reference's own test cases hold on it; the long-double property checkers pass on the restatements'
outputs with the recorded residuals, skip at most 1 % of the steps as ambiguous, hold the closed
forms and notice eight mutations; every outcome is reached for every D. No GPU needed."""
import collections
import functools
import subprocess
import time

import numpy as np
import pytest

import native_driver
import stop_reference as sr

ALL_DOFS = list(range(1, 17))
TIME_STEP = 1e-3


@functools.lru_cache(maxsize=None)
def batch_results(D):
    """make_batch(D) with the restatements' results: per row the stop by time, the stop by index
    and the fastest stop."""
    rows = sr.make_batch(D)
    out = []
    for row in rows:
        args = (row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP)
        out.append(dict(row=row, by_time=sr.stop_before_time(*args, row["query"]),
                        by_index=sr.stop_at_index(*args, row["index"]),
                        forward=sr.fastest_stop_result(row["time"], row["s"], row["qd"], row["qdd"], row["amax"],
                                                       row["fs_query"])))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return native_driver.build_driver("test_stop_reference.cc", tmp_path_factory.mktemp("stop_reference"), opt="-O2",
                                      extra_sources=("host/rescale_to_stop.cc", "host/trajectory_buffer.cc"), timeout=600)


def _hex(values):
    return " ".join(float(x).hex() for x in values)


def _flat(rows):
    return [x for r in rows for x in r]


def run_driver(exe, path, cases):
    """cases: (row, by_index). Returns per case the parsed M, S and B lines."""
    with open(path, "w") as f:
        f.write("%d\n" % len(cases))
        for row, by_index in cases:
            n, D = len(row["time"]), len(row["amax"])
            f.write("%d %d %d %d %s %s\n" % (n, D, int(by_index), row["index"], float(row["query"]).hex(),
                                             float(TIME_STEP).hex()))
            f.write(_hex(row["time"] + _flat(row["q"]) + _flat(row["qd"]) + _flat(row["qdd"]) + row["amax"]) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 3 * len(cases)
    parsed = []
    for k in range(len(cases)):
        rec = {}
        for line in lines[3 * k:3 * k + 3]:
            tok = line.split()
            head = 5 if tok[0] == "S" else 4
            rec[tok[0]] = ([int(x) for x in tok[1:head]], [float.fromhex(x) for x in tok[head:]])
        parsed.append(rec)
    return parsed


def _same_bits(a, b):
    return np.asarray(a, dtype=np.float64).tobytes() == np.asarray(b, dtype=np.float64).tobytes()


def compare_with_driver(row, res, rec, where):
    """The restatement's stop `res` of `row` against the driver's three results."""
    n, D = len(row["time"]), len(row["amax"])
    bt, bq, bv, ba = sr.stopped_buffer(row["time"], row["q"], row["qd"], row["qdd"], res)
    sequence = 0 if res["replaced"] or not res["inserted"] else 1
    want = bt + _flat(bq) + _flat(bv) + _flat(ba)
    for who in ("M", "B"):
        (status, seq, count), values = rec[who]
        assert status == res["status"], where + (who, "status", status, res["status"])
        assert count == len(bt) and seq == sequence, where + (who, count, len(bt), seq, sequence)
        assert _same_bits(values, want), where + (who, "buffer")
    (status, keep, first, last), values = rec["S"]
    assert (status, keep, first, last) == (res["status"], res["keep"], res["first"], res["last"]), where + ("S",)
    assert _same_bits(values, res["time"] + _flat(res["qd"]) + _flat(res["qdd"])), where + ("S", "rows")


@pytest.mark.parametrize("D", ALL_DOFS)
def test_restatement_equals_mirror_and_kernel_cores_bit_for_bit(driver, tmp_path, D):
    results = batch_results(D)
    cases = [(r["row"], by_index) for r in results for by_index in (False, True)]
    parsed = run_driver(driver, tmp_path / "cases.txt", cases)
    for k, ((row, by_index), rec) in enumerate(zip(cases, parsed)):
        res = results[k // 2]["by_index" if by_index else "by_time"]
        compare_with_driver(row, res, rec, (D, k // 2, row["label"], by_index))


def test_no_admissible_deceleration_is_internal_and_changes_nothing(driver, tmp_path):
    """Regression for the rest sample without an admissible deceleration: its only joint at or
    above the 1e-8 cut asks more of a joint under the cut than that joint's limit allows, no
    candidate is valid at rate2 = 0, d = 0 and the first rescaled step is 2 dt / 0. The reference
    goes on to a segment with NaN times; the kernels used to take the NaN front time into the
    bracket search of the velocity match (sample -1) and into the kept count (keep 0, while the
    mirror kept every sample and appended the NaN rows). Now mirror, kernels and restatement
    report TPAMD_PLAN_INTERNAL and change nothing."""
    cases = []
    for D in (2, 3, 8, 9, 16):
        rng = np.random.default_rng(D)
        for n in (3, 40, 120):
            row = sr.make_row("no_deceleration", rng, D, max(n, 6))
            if n == 3:          # the segment would use every sample: the velocity match comes next
                row["index"], row["query"] = 2, row["time"][1]
                for k in ("time", "s", "q", "qd", "qdd"):
                    row[k] = row[k][:4]
                row["qd"][2] = [1e-8] + [9e-9] * (D - 1)
            cases.append((row, False))
            cases.append((row, True))
    parsed = run_driver(driver, tmp_path / "cases.txt", cases)
    for (row, by_index), rec in zip(cases, parsed):
        args = (row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP)
        res = sr.stop_at_index(*args, row["index"]) if by_index else sr.stop_before_time(*args, row["query"])
        assert res["status"] == sr.INTERNAL and res["keep"] == len(row["time"])
        compare_with_driver(row, res, rec, (len(row["amax"]), len(row["time"]), by_index))
        sr.check_stop_segment(*args, res, index=row["index"] if by_index else None, stop_time=row["query"])


def test_in_place_stop_keeps_the_sample_its_segment_goes_behind(driver, tmp_path):
    """Regression for bs_stop_in_place (the code of k_bset_stop) with keep = first + 1: time stamps
    just under 2^34 s, where the segment's front time lands one ulp (1.9e-6 s, more than the 1e-6
    tolerance) behind sample `first`, so InsertSegment keeps that sample and the segment goes one
    row up. The in-place stop used to rescale rows [first, index] where they stood and move them
    up afterwards, which left the segment's first row in place of the kept sample `first`. Line B
    of the driver must equal the restatement and the mirror."""
    cases = []
    for D in (1, 3, 7, 16):
        row = sr.make_row("late_clock", np.random.default_rng(100 + D), D, 140)
        cases += [(row, False), (row, True)]
    parsed = run_driver(driver, tmp_path / "cases.txt", cases)
    for (row, by_index), rec in zip(cases, parsed):
        args = (row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP)
        res = sr.stop_at_index(*args, row["index"]) if by_index else sr.stop_before_time(*args, row["query"])
        assert res["status"] == sr.OK and res["keep"] == res["first"] + 1, (len(row["amax"]), res["keep"], res["first"])
        compare_with_driver(row, res, rec, (len(row["amax"]), by_index))
        kept = rec["B"][1][res["first"]]                   # the buffer's time stamp at row `first`
        assert kept == row["time"][res["first"]] and kept < res["time"][0]


# ------------------------------------------------------------------ the reference's own test cases
def _constant(D, x):
    return [x] * D


def _quadratic(n, dt, D):
    """GetQuadraticTestTrajectory of trajectory_buffer_test.cc: q = 0.5 (t - T)^2, v = t - T, a = 1."""
    T = (n - 1) * dt
    time = [dt * i for i in range(n)]
    return (time, [_constant(D, 0.5 * (t - T) * (t - T)) for t in time], [_constant(D, t - T) for t in time],
            [_constant(D, 1.0) for _ in time])


def test_reference_test_cases_on_the_restatement():
    # rescale_to_stop_test.cc SucceedsForConstantVelocity: 200 samples, 8 ms, 4 joints, limit 2
    for velocity in (-1.0, 1.0):
        n, D, dt, amax = 200, 4, 8e-3, 2.0
        time = [i * dt for i in range(n)]
        q = [_constant(D, velocity * t) for t in time]
        what, seg = sr.rescale_backward_to_stop(_constant(D, amax), time, [_constant(D, velocity)] * n,
                                                [_constant(D, 0.0)] * n)
        assert what == "ok"
        st, sv, sa = seg
        assert len(st) > 0 and len(st) == len(sv) == len(sa)
        assert abs((st[-1] - st[0]) - abs(velocity) / amax) <= dt
        assert not any(sv[-1]) and not any(sa[-1])
        travel = velocity * velocity / (2.0 * amax) * (-1.0 if velocity < 0 else 1.0)
        assert abs(q[n - 1][0] - q[n - len(st)][0] - travel) <= abs(velocity * dt)
    # trajectory_buffer_test.cc: the quadratic trajectory, 9 joints, 1001 samples of 1 ms
    D, n, dt = 9, 1001, 1e-3
    time, q, qd, qdd = _quadratic(n, dt, D)

    def within(res, amax):
        return all(abs(x) <= amax + 1e-8 for r in res["qdd"] for x in r)

    r = sr.stop_at_index(time, qd, qdd, _constant(D, 5.0), dt, n // 2)         # StopAtIndexSucceedsIfFeasible
    assert r["status"] == sr.OK and r["keep"] + len(r["time"]) >= n // 2 + 1 and not any(r["qd"][-1]) and within(r, 5.0)
    sr.check_stop_segment(time, qd, qdd, _constant(D, 5.0), dt, r, index=n // 2)
    r = sr.stop_at_index(time, qd, qdd, _constant(D, 1.0), dt, 2)              # StopAtIndexFailsIfInfeasible
    assert r["status"] == sr.NOT_FOUND and r["keep"] == n
    for t in (dt * 2, dt * 3.1415):                                            # StopBeforeTimeFailsIfInfeasible
        assert sr.stop_before_time(time, qd, qdd, _constant(D, 1.0), dt, t)["status"] == sr.NOT_FOUND
    for t in (time[n // 2], 0.5 * (time[n // 2] + time[n // 2 + 1])):          # StopBeforeTimeSucceedsIfFeasible
        r = sr.stop_before_time(time, qd, qdd, _constant(D, 5.0), dt, t)
        assert r["status"] == sr.OK and r["keep"] + len(r["time"]) >= n // 2 + 1 and not any(r["qd"][-1]) and within(r, 5.0)
        sr.check_stop_segment(time, qd, qdd, _constant(D, 5.0), dt, r, stop_time=t)
    # StopBeforeTimeSucceedsIfCutoffTimeBeyondFinalTimestep: 50 samples of 10 ms, velocity 1
    t50 = [i * 0.01 for i in range(50)]
    r = sr.stop_before_time(t50, [_constant(3, 1.0)] * 50, [_constant(3, 0.0)] * 50, _constant(3, 2.0), 0.01, t50[-1] + 12.0)
    assert r["status"] == sr.OK and r["last"] == 49 and not any(r["qd"][-1])
    # DetectsErrors: 5 samples from 1.0 s, v = 10 i, a = 100 i
    t5 = [i * 8e-3 + 1.0 for i in range(5)]
    v5, a5, amax = [_constant(D, 10.0 * i) for i in range(5)], [_constant(D, 100.0 * i) for i in range(5)], _constant(D, 4.0)
    assert sr.stop_at_index([], [], [], amax, 8e-3, -1)["status"] == sr.OUT_OF_RANGE
    assert sr.stop_at_index([], [], [], amax, 8e-3, 0)["status"] == sr.OUT_OF_RANGE
    assert sr.stop_at_index(t5, v5, a5, amax, 8e-3, 5)["status"] == sr.OUT_OF_RANGE
    assert sr.stop_at_index(t5, v5, a5, amax, -0.1, 2)["status"] == sr.INVALID_ARGUMENT
    assert sr.stop_at_index(t5, v5, a5, _constant(D, 0.0), 8e-3, 2)["status"] == sr.INVALID_ARGUMENT
    assert sr.stop_before_time(t5, v5, a5, amax, 8e-3, 0.5)["status"] == sr.OUT_OF_RANGE
    r = sr.stop_before_time([], [], [], amax, 8e-3, 1.0)
    assert (r["status"], r["keep"], r["first"], r["last"]) == (sr.OK, 0, 0, -1)
    # the documented deviation: at rest before the end
    time, q, qd, qdd = _quadratic(20, 1e-2, 2)
    qd[10] = [0.0, 0.0]
    assert sr.stop_at_index(time, qd, qdd, [5.0, 5.0], 1e-2, 10)["status"] == sr.INTERNAL


# ------------------------------------------------------------------ the checkers on the restatements
def test_checkers_pass_residuals_ambiguity_and_outcomes():
    residuals, families = {}, collections.defaultdict(dict)
    back, fwd = {}, {}
    t0 = time.time()
    for D in ALL_DOFS:
        back[D], fwd[D] = collections.Counter(), collections.Counter()
        for k, r in enumerate(batch_results(D)):
            row = r["row"]
            args = (row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP)
            sr.check_stop_segment(*args, r["by_time"], stop_time=row["query"], residuals=residuals,
                                  stats=families["backward " + row["label"]])
            sr.check_stop_segment(*args, r["by_index"], index=row["index"], residuals=residuals,
                                  stats=families["backward " + row["label"]])
            sr.check_fastest_stop(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], row["fs_query"],
                                  r["forward"], residuals=residuals, stats=families["forward " + row["label"]])
            back[D].update(sr.backward_outcomes(row, r["by_time"], False))
            back[D].update(sr.backward_outcomes(row, r["by_index"], True))
            fwd[D].update(sr.forward_outcomes(row, r["forward"]))
    print("restatements and checkers, D = 1..16: %.1f s" % (time.time() - t0))
    print("measured residuals:", {k: "%.3g" % v for k, v in sorted(residuals.items())})
    for k in sr.MEASURED_RESIDUALS:
        # the recorded figure is the measured one, rounded up
        assert residuals[k] <= sr.MEASURED_RESIDUALS[k] <= 1.25 * residuals[k] + 1e-18, (k, residuals[k])
        assert sr.TOLERANCES[k] == 16 * sr.MEASURED_RESIDUALS[k]
    for name, st in sorted(families.items()):
        steps, amb = st.get("steps", 0), st.get("ambiguous", 0)
        print("ambiguous steps, %-26s %6d of %6d" % (name + ":", amb, steps))
        assert amb <= 0.01 * steps, (name, amb, steps)
    print(sr.outcome_table("backward stops (restatement)", sr.BACKWARD_OUTCOMES, back))
    print(sr.outcome_table("forward stops (restatement)", sr.FORWARD_OUTCOMES, fwd))
    for D in ALL_DOFS:
        skip = sr.UNREACHABLE.get(D, set())
        assert [k for k in sr.BACKWARD_OUTCOMES if not back[D][k] and k not in skip] == [], D
        assert [k for k in sr.FORWARD_OUTCOMES if not fwd[D][k] and k not in skip] == [], D


@pytest.mark.parametrize("D", [1, 2, 3, 8, 9, 16])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_closed_forms(D, sign):
    row, (K, dt, duration) = sr.constant_velocity_case(D, sign=sign)
    n = len(row["time"])
    args = (row["time"], row["qd"], row["qdd"], row["amax"], dt)
    backward = sr.stop_at_index(*args, n - 1)
    forward = sr.fastest_stop_result(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], row["time"][0])
    sr.check_closed_forms(row, K, dt, duration, backward, forward)
    sr.check_stop_segment(*args, backward, index=n - 1)
    sr.check_fastest_stop(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], row["time"][0], forward)
    wrong = dict(backward, qdd=[[2.0 * x for x in r] for r in backward["qdd"]])
    with pytest.raises(sr.StopCheckError):
        sr.check_closed_forms(row, K, dt, duration, wrong, forward)


# ------------------------------------------------------------------ the checkers notice errors
def _mutant_stop(row, index, mutation=None):
    """A second, compact backward stop at `index` with one deliberate error. Without a mutation
    it is a correct stop (the checker must pass it)."""
    t, v, a = np.array(row["time"]), np.array(row["qd"]), np.array(row["qdd"])
    amax = np.array(row["amax"])
    D = len(amax)
    rt, rv, ra = [0.0], [np.zeros(D)], [np.zeros(D)]
    rate2 = 0.0
    for i in range(index, 1, -1):
        bias = a[i] * rate2
        cands = []
        for c in range(D):
            if abs(v[i, c]) < 1e-8:
                continue
            for sign in (-1.0, 1.0):
                b = -bias[c] if mutation == "candidate_sign" else bias[c]
                d = -2.0 * (b + sign * amax[c]) / v[i, c]
                s = bias + 0.5 * v[i] * d
                if (amax - s).min() >= -1e-8 and (-amax - s).max() <= 1e-8 and d < 0.0:
                    cands.append(d)
        cands.sort()
        d = cands[0] if cands else 0.0
        if mutation == "non_minimal" and rate2 > 0.0:
            d = cands[1] if len(cands) > 1 else 0.0
        if mutation == "d_halved":
            d *= 0.5
        dt = t[i] - t[i - 1]
        nxt = rate2 - d * dt
        clamped = nxt if mutation == "rate_not_clamped" else min(nxt, 1.0)
        rt.append(rt[-1] - 2.0 * dt / (np.sqrt(rate2) + np.sqrt(clamped)))
        rv.append(np.sqrt(clamped) * v[i])
        ra.append(bias + 0.5 * v[i] * d)
        if nxt >= 1.0:
            break
        rate2 = nxt
    rt, rv, ra = rt[::-1], rv[::-1], ra[::-1]
    first = index + 1 - len(rt)
    offset = 0.0 if mutation == "time_shift_dropped" else t[first] - rt[0]
    rt = [x + offset for x in rt]
    if mutation == "rows_shifted":          # every scaled row carries the values of the row behind it
        rv, ra = rv[1:-1] + rv[-2:], ra[1:-1] + ra[-2:]
    if mutation == "one_joint_rate":
        rv = [x * np.where(np.arange(D) == D - 1, 0.9, 1.0) for x in rv]
    keep, _ = sr.insert_segment_kept(row["time"], t[first] if mutation == "time_shift_dropped" else rt[0])
    if mutation == "keep_off_by_one":
        keep += 1
    return dict(status=sr.OK, keep=keep, first=first, last=index, time=[float(x) for x in rt],
                qd=[[float(x) for x in r] for r in rv], qdd=[[float(x) for x in r] for r in ra])


MUTATIONS = ("d_halved", "rows_shifted", "rate_not_clamped", "candidate_sign", "non_minimal", "keep_off_by_one",
             "time_shift_dropped", "one_joint_rate")


def _mutation_case():
    rng = np.random.default_rng(5)
    row = sr.make_row("solver", rng, 3, 160)
    return row, 150


def test_the_unmutated_stop_passes_the_checker():
    row, index = _mutation_case()
    args = (row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP)
    res = _mutant_stop(row, index)
    assert 1 < res["first"] < index - 8
    sr.check_stop_segment(*args, res, index=index)
    ref = sr.stop_at_index(*args, index)
    assert (ref["status"], ref["keep"], ref["first"]) == (sr.OK, res["keep"], res["first"])


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_checker_notices(mutation):
    row, index = _mutation_case()
    res = _mutant_stop(row, index, mutation)
    with pytest.raises(sr.StopCheckError) as err:
        sr.check_stop_segment(row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP, res, index=index)
    print("%s: %s" % (mutation, err.value))


@pytest.mark.parametrize("mutation", ["d_halved", "rate_not_clamped", "candidate_sign", "stop_one_late", "duration"])
def test_the_forward_checker_notices(mutation):
    row, _ = _mutation_case()
    q = row["time"][3]
    res = sr.fastest_stop_result(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], q)
    sr.check_fastest_stop(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], q, res)
    assert len(res["rate2"]) > 8
    bad = {k: (list(v) if isinstance(v, list) else v) for k, v in res.items()}
    if mutation == "d_halved":
        bad["drate2"] = [0.5 * x for x in bad["drate2"]]
    elif mutation == "rate_not_clamped":
        bad["rate2"][-1] = -1e-3
    elif mutation == "candidate_sign":
        bad["drate2"][2] = -bad["drate2"][2]
    elif mutation == "stop_one_late":
        bad["stop_index"] += 1
        bad["stop_parameter"] = row["s"][bad["stop_index"]]
    else:
        bad["duration"] *= 1.0 + 1e-9
    with pytest.raises(sr.StopCheckError):
        sr.check_fastest_stop(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], q, bad)

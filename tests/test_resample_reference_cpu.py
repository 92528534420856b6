"""tests/resample_reference.py, the independent restatement of the two resamplers and the s(t)
query, held to the oracle bit for bit (tpo.resample_uniform, tpo.resample_skip,
tpo_resample_uniform_count, tpo.Profile.query) on solved joint profiles and on the synthetic rows
of tests/resample_cases.py, with every interpolated value also within lerp_exact_bound of the
exact one; and the conditions on those inputs that tests/test_gpu_resample_query_edges.py relies
on: that they reach the clamp, the sub-epsilon bracket, every branch of the query, the counts 1, 0
and below, and ticks on sample times. These hold on the restatement alone, so the GPU test cannot
pass by missing a branch. No GPU needed."""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import resample_cases as rc
import resample_reference as rr
import scenarios

@pytest.fixture(scope="module")
def tpo():
    from oracle import tpo
    tpo.build()
    return tpo


def _rows(case, i):
    return [case["sol"][k][i].tolist() for k in rc.SOL], case["amax"][i].tolist()


def _ref(fn, case, i, **kw):
    rows, amax = _rows(case, i)
    return fn(*rows, float(case["start"][i]), case["dt"], amax, **kw)


def _assert_equals_oracle(samples, oracle, what):
    for name, got, want in zip(rc.SOL, samples, oracle):
        got = np.array(got, dtype=np.float64).reshape(want.shape)
        np.testing.assert_array_equal(got, want, err_msg="%s %s" % (what, name))


def _assert_within_exact(case, i, r, t, values, what):
    """The values InterpolateAtTime gave at time t from the bracket of trace dict r against the
    exact interpolation; values = (s, sd, sdd, q, qd, qdd) of that tick."""
    sol, amax = case["sol"], case["amax"][i]
    lo, up = r["lower_index"], r["upper_index"]
    tl, tu = float(sol["time"][i, lo]), float(sol["time"][i, up])
    for name, got in zip(rc.SOL[1:], values):
        a, b = sol[name][i, lo], sol[name][i, up]
        for d, (x, y, g) in enumerate(zip(np.atleast_1d(a), np.atleast_1d(b), np.atleast_1d(got))):
            exact, bound = rr.lerp_exact_bound(tl, tu, t, float(x), float(y))
            if name == "qdd":
                am = Fraction(float(amax[d]))
                exact = min(max(exact, -am), am)            # the clamp moves two values no further apart
            assert abs(Fraction(float(g)) - exact) <= bound, (what, name, d, float(g), float(exact), float(bound))


def _check_uniform(tpo, case, what):
    B, N, D = case["sol"]["q"].shape
    counts = []
    for i in range(B):
        trace = []
        count, samples = _ref(rr.resample_uniform, case, i, trace=trace)
        assert isinstance(count, int)
        want = tpo.lib().tpo_resample_uniform_count(float(case["sol"]["time"][i, -1]), float(case["start"][i]), case["dt"])
        assert count == want, (what, i)
        counts.append(count)
        if count <= 0:
            assert all(len(x) == 0 for x in samples)
            continue
        oracle = tpo.resample_uniform(*[case["sol"][k][i] for k in rc.SOL], float(case["start"][i]), case["dt"],
                                      case["amax"][i])
        _assert_equals_oracle(samples, oracle, "%s path %d" % (what, i))
        for j in range(count - 1):                          # the end sample is set, not interpolated
            _assert_within_exact(case, i, trace[j], samples[0][j], [x[j] for x in samples[1:]],
                                 "%s path %d tick %d" % (what, i, j))
        j = count - 1                                       # ... but its s, sd, sdd are
        _assert_within_exact(case, i, trace[j], samples[0][j], [x[j] for x in samples[1:4]], "%s end" % what)
    return counts


def _check_skip(tpo, case, what):
    B, N, D = case["sol"]["q"].shape
    counts = []
    for i in range(B):
        trace = []
        count, samples = _ref(rr.resample_skip, case, i, trace=trace)
        oracle = tpo.resample_skip(*[case["sol"][k][i] for k in rc.SOL], float(case["start"][i]), case["dt"],
                                   case["amax"][i])
        assert count == len(oracle[0]) == len(samples[0]), (what, i)
        _assert_equals_oracle(samples, oracle, "%s path %d" % (what, i))
        n = 7 if count > 1 else 4                           # with one output its q, qd, qdd are the end sample's
        _assert_within_exact(case, i, trace[0], float(case["start"][i]), [x[0] for x in samples[1:n]], what)
        for cap in (70, 1):                                 # the C-ABI's cut: a prefix, the end sample only if it fits
            c2, cut = _ref(rr.resample_skip, case, i, max_out=cap)
            assert c2 == count
            w = min(cap, count)
            for full, part in zip(samples, cut):
                assert part == full[:w]
        counts.append(count)
    return counts


# ------------------------------------------------------------------ the restatement against the oracle
@pytest.mark.parametrize("D", rc.ALL_DOFS)
def test_uniform_every_joint_count(tpo, D):
    counts = _check_uniform(tpo, rc.uniform_dof_case(D), "D=%d" % D)
    assert min(counts) > 60


EDGES = rc.uniform_edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_uniform_edges(tpo, name):
    counts = _check_uniform(tpo, EDGES[name], name)
    if name.startswith("count_"):
        assert counts == [int(name[6:])] * 2


def test_uniform_max_out(tpo):
    """max_out with the C-ABI's meaning, against the oracle's own max_out argument."""
    case = rc.count_case(rc.MAX_OUT_COUNT)
    B, N, D = case["sol"]["q"].shape
    for i in range(B):
        full_count, full = _ref(rr.resample_uniform, case, i)
        assert full_count == rc.MAX_OUT_COUNT
        for cap in rc.max_outs(full_count):
            count, cut = _ref(rr.resample_uniform, case, i, max_out=cap)
            assert count == full_count and len(cut[0]) == min(cap, count)
            out = [np.full((cap,) + ((D,) if k in rc.SOL[4:] else ()), -1.0) for k in rc.SOL]
            M = tpo.lib().tpo_resample_uniform(*[np.ascontiguousarray(case["sol"][k][i]) for k in rc.SOL], N, D,
                                               float(case["start"][i]), case["dt"],
                                               np.ascontiguousarray(case["amax"][i]), cap, *out)
            assert M == full_count
            _assert_equals_oracle(cut, out, "max_out=%d path %d" % (cap, i))
            if cap < count:                                 # the end sample is special only if it is written
                assert cut[4][-1] == full[4][cap - 1] and cut[5][-1] == full[5][cap - 1]


@pytest.mark.parametrize("D", rc.ALL_DOFS)
def test_skip_every_joint_count(tpo, D):
    counts = _check_skip(tpo, rc.skip_dof_case(D), "D=%d" % D)
    # kept samples: a full 64-entry register batch and a partial one; a cut at 70 falls inside the second
    assert 71 <= counts[0] - 1 <= 127 and 71 <= counts[1] - 1 <= 127, counts


def test_skip_edges(tpo):
    """The first output of the skip method on the uniform edge inputs: before, on and past the
    samples, the sub-epsilon bracket, N = 2."""
    for name in ("ticks_on_samples", "past_the_end", "tiny_bracket", "two_samples"):
        _check_skip(tpo, EDGES[name], name)


@functools.lru_cache(maxsize=None)
def _solved(tpo):
    import structured_paths as sp
    b = rc.solved_batch()
    return b, sp.oracle_solve(tpo, b, rc.SOLVED_N, nthreads=1)


def test_solved_profiles_resample(tpo):
    b, ref = _solved(tpo)
    assert (ref["status"] == 0).all()
    sol = {k: ref["t" if k == "time" else k] for k in rc.SOL}
    plateau = 0
    for frac in (-0.01, 0.0, 0.37, 1.0):
        start = sol["time"][:, 0] + frac * (sol["time"][:, -1] - sol["time"][:, 0])
        case = dict(sol=sol, amax=b["amax"], start=start, dt=0.016)
        _check_uniform(tpo, case, "solved, start at %g" % frac)
        _check_skip(tpo, case, "solved, start at %g" % frac)
    for i in range(len(rc.SOLVED_FAMILIES)):
        plateau += int((np.diff(sol["time"][i]) == 0).any())
    assert plateau >= 2, "stop_first and stop_last no longer give time plateaus"


def _check_query(p, times, reached, what):
    time, s, sd, sd2 = (x.tolist() for x in (p.time, p.s, p.sd, p.sd2))
    for t in times:
        tr = {}
        got = rr.query(time, s, sd, sd2, float(t), trace=tr)
        want = p.query(float(t))
        assert got == want, (what, float(t).hex(), got, want, tr)
        reached.add(tr["branch"])
        if tr["k"] is not None and tr["low_idx"] > 0 and tr["k"] == tr["low_idx"]:
            reached.add("plateau_first")
        if tr["k"] is not None and tr["high_idx"] < len(time) - 1 and tr["k"] == tr["high_idx"] - 1:
            reached.add("plateau_last")


def test_query_matches_oracle_on_solved_profiles(tpo):
    reached = set()
    for name, rows, s0, s1, sd0, _ in scenarios.all_cases():
        n, c = rows[0].shape
        p = tpo.Profile(n, c)
        p.set_max_loops(10 * n)
        assert p.setup(*rows, s0, s1, sd0) == 0 and p.optimize() == 0, name
        _check_query(p, rc.query_times(p.time), reached, name)
    b, _ = _solved(tpo)
    for i, name in enumerate(rc.SOLVED_FAMILIES):
        p = rc.oracle_profile(tpo, b, i)
        _check_query(p, rc.query_times(p.time), reached, name)
    assert {"start", "end", "moving", "plateau_first", "plateau_last"} <= reached, reached


# ------------------------------------------------------------------ the inputs reach what they claim
def test_inputs_reach_the_acceleration_clamp_and_the_sub_epsilon_bracket():
    for D in rc.ALL_DOFS:
        case = rc.uniform_dof_case(D)
        clamped = 0
        for i in range(4):
            trace = []
            count, _ = _ref(rr.resample_uniform, case, i, trace=trace)
            clamped += sum(any(r["clamped"]) for r in trace[:count - 1])    # the end sample's is set to zero
        assert clamped > 0, D
        case = rc.skip_dof_case(D)
        trace = []
        _ref(rr.resample_skip, case, 0, trace=trace)
        trace1 = []
        _ref(rr.resample_skip, case, 1, trace=trace1)
        # the skip method interpolates its first output only: 2 D accelerations against limits of
        # 0.1 .. 0.8 (resample_cases.trajectory), too few draws to count on below 3 joints; the
        # uniform side above reaches the clamp at every D
        if D >= 3:
            assert any(trace[0]["clamped"]) or any(trace1[0]["clamped"]), D
    case = rc.tiny_bracket_case()
    time = case["sol"]["time"]
    for i, half in enumerate((True, True, False)):
        trace = []
        _ref(rr.resample_uniform, case, i, trace=trace)
        r = trace[0]
        assert r["half"] == half, i
        if half:
            assert (r["lower_index"], r["upper_index"]) == (0, 1) and time[i, 0] != time[i, 1]
            assert r["interpolate_at"] == 0.5
        assert not any(x["half"] for x in trace[1:-1])
        trace = []
        _ref(rr.resample_skip, case, i, trace=trace)
        assert trace[0]["half"] == half


def test_inputs_reach_the_counts_and_the_ticks():
    case = rc.past_the_end_case()
    counts = [_ref(rr.resample_uniform, case, i)[0] for i in range(4)]
    assert counts[0] == 1 and counts[1] == 1 and counts[2] == 0 and counts[3] < 0, counts
    case = rc.ticks_on_samples_case()
    for i in (0, 1):
        trace = []
        count, samples = _ref(rr.resample_uniform, case, i, trace=trace)
        assert count == 40 - (0, 5)[i]
        stamps = set(case["sol"]["time"][i].tolist())
        assert all(t in stamps for t in samples[0][1:-1]) and samples[0][0] in stamps and samples[0][-1] in stamps
        # on a sample the bracket is the one that begins there: interpolate_at is exactly 0
        assert all(r["interpolate_at"] == 0.0 for r in trace[:-1])
        assert [r["lower_index"] for r in trace[:-1]] == list(range((0, 5)[i], 39))
        # ... and the bracket that ends there (interpolate_at = 1) would not give the same numbers
        q = case["sol"]["q"][i].tolist()
        assert any(rr.interpolate_linear(1.0, a, b) != b for ra, rb in zip(q[:-1], q[1:]) for a, b in zip(ra, rb))
    trace = []
    _ref(rr.resample_uniform, case, 2, trace=trace)
    assert trace[0]["interpolate_at"] == -0.5 and all(r["interpolate_at"] == 0.5 for r in trace[1:-1])
    case = rc.two_samples_case()
    assert [_ref(rr.resample_uniform, case, i)[0] for i in range(3)] == [8, 4, 1]
    case = rc.uniform_dof_case(3)
    starts = []
    for i in range(4):
        trace = []
        _ref(rr.resample_uniform, case, i, trace=trace)
        starts.append((trace[0]["lower_index"], trace[0]["interpolate_at"]))
    assert starts[0][0] == 0 and starts[0][1] < 0                    # before the first sample: extrapolation
    assert 0 < starts[1][0] < 128 and 0 < starts[1][1] < 1
    assert starts[2] == (64, 0.0) and starts[3][0] == 64 and 0 < starts[3][1] < 1e-10


def test_query_inputs_reach_every_branch():
    """Every branch the GPU test's query batches claim is returned by the restatement, in every
    batch shape that has room for it."""
    for N in rc.QUERY_SAMPLES:
        union = set()
        for B, K in rc.QUERY_SHAPES:
            qb = rc.query_batch(N, B, K)
            reached = set()
            for b in range(B):
                rows = [qb[k][b].tolist() for k in ("time", "s", "sd", "sd2")]
                for t in qb["tq"][b].tolist():
                    tr = {}
                    ok, s, sd, sdd = rr.query(*rows, t, trace=tr)
                    reached.add(tr["branch"])
                    assert ok == (tr["branch"] != "invalid")
                    if tr["clamped"] and ok:
                        reached.add("clamped")
                    if tr["saturated"]:
                        reached.add("saturated")
                    if tr["k"] is not None and tr["low_idx"] > 0 and tr["k"] == tr["low_idx"]:
                        reached.add("plateau_first")
                    if tr["k"] is not None and tr["high_idx"] < N - 1 and tr["k"] == tr["high_idx"] - 1:
                        reached.add("plateau_last")
                    if ok:
                        assert all(math.isfinite(x) for x in (s, sd, sdd))
            union |= reached
            assert {"start", "end"} <= reached or B * K < 256, (N, B, K, reached)
            if N >= 65:                     # row kinds by b % 4: see query_batch
                want = {"start", "end", "moving"}
                if B >= 2:
                    want |= {"plateau_first", "plateau_last"}
                if B >= 4:
                    want |= {"clamped", "saturated", "invalid", "zero_velocity"}
                assert want <= reached, (N, B, K, want - reached)
        assert {"start", "end", "moving"} <= union, (N, union)
        assert "equal_time" not in union        # SampleIndexFromTime's bracket is strict: no finite time gets there

"""The solution check on explicit rows on the GPU (tpamd_check_rows_*, Engine.check_rows).

No solve is needed: the rows and the "solution" are made up. Every comparison is bit equality with
tests/check_reference.py (NaN by position); the outputs are filled with sentinels first. Five paths
per (N, C); N * C covers less than a wave (3), one element more than a block (257 x 1), several
trips and C that does not divide the block (14, 33):
  0  random rows with margin, a few violated ones, and a largest excess of exactly 5 that four
     elements share -- a duplicated sample and a duplicated row -- so the tie rule decides
  1  every element on the kTiny edge: upper = v - kTiny (kept), the next double below (violated),
     lower = v + kTiny (kept), the next double above (violated)
  2  as 0 without the tie, with a NaN sdd at sample 1
  3  nothing but NaN: count 0, NaN, -1, -1, -1
  4  as 2, with status 7: the -1 record (and a checked path when no status is given)"""
import importlib

import numpy as np
import pytest

import check_reference as cr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

B = 5
SHAPES = [(n, c) for n in (3, 65, 257, 600) for c in (1, 2, 14, 33, 64)]
PRE, PRE_INT = -7.25, -9


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev="cuda:0")


def _v(a, b, sd2, sdd):
    with np.errstate(invalid="ignore"):
        return a * sdd[:, None] + b * sd2[:, None]


def make_case(N, C):
    rng = np.random.default_rng(1000 * N + C)
    a = rng.uniform(-2.0, 2.0, (B, N, C))
    b = rng.uniform(-2.0, 2.0, (B, N, C))
    sd2 = rng.uniform(0.0, 3.0, (B, N))
    sdd = rng.uniform(-3.0, 3.0, (B, N))
    lo, hi = np.empty((B, N, C)), np.empty((B, N, C))
    j, k = 0, N - 1                              # the duplicated sample
    for p in (0, 2, 4):
        if p == 0:
            a[p, k], b[p, k], sd2[p, k], sdd[p, k] = a[p, j], b[p, j], sd2[p, j], sdd[p, j]
            if C > 1:
                a[p, :, C - 1], b[p, :, C - 1] = a[p, :, 0], b[p, :, 0]
        v = _v(a[p], b[p], sd2[p], sdd[p])
        lo[p] = v - rng.uniform(0.5, 2.0, (N, C))
        hi[p] = v + rng.uniform(0.5, 2.0, (N, C))
        bad = rng.uniform(size=(N, C)) < 0.1      # violated on one side or the other, by less than 5
        up = rng.uniform(size=(N, C)) < 0.5
        hi[p][bad & up] = (v - rng.uniform(0.01, 3.0, (N, C)))[bad & up]
        lo[p][bad & ~up] = (v + rng.uniform(0.01, 3.0, (N, C)))[bad & ~up]
        if p == 0:
            for i in (j, k):
                for c in {0, C - 1}:
                    lo[p, i, c], hi[p, i, c] = v[i, c] - 9.0, v[i, c] - 5.0
    # path 1: the kTiny edge, element by element
    v = _v(a[1], b[1], sd2[1], sdd[1])
    lo[1], hi[1] = v - 1.0, v + 1.0
    kind = (np.arange(N * C) % 5).reshape(N, C)
    hi[1][kind == 1] = (v - cr.KT)[kind == 1]
    hi[1][kind == 2] = np.nextafter(v - cr.KT, -np.inf)[kind == 2]
    lo[1][kind == 3] = (v + cr.KT)[kind == 3]
    lo[1][kind == 4] = np.nextafter(v + cr.KT, np.inf)[kind == 4]
    sdd[2, 1] = np.nan
    sdd[4, 1] = np.nan
    sd2[3], sdd[3] = np.nan, np.nan
    lo[3], hi[3] = -1.0, 1.0
    status = np.array([0, 0, 0, 0, 7], np.int32)
    return dict(N=N, C=C, a=a, b=b, lower=lo, upper=hi, sd2=sd2, sdd=sdd, sd=np.sqrt(sd2), status=status)


def expected(case, counts=None, use_status=True, from_sd=False):
    N = case["N"]
    sd2 = case["sd"] * case["sd"] if from_sd else case["sd2"]
    recs = []
    for p in range(B):
        n = N if counts is None else int(counts[p])
        if (use_status and case["status"][p] != 0) or n < 2 or n > N:
            recs.append(cr.NOT_CHECKED)
        else:
            recs.append(cr.check_rows(case["a"][p, :n], case["b"][p, :n], case["lower"][p, :n], case["upper"][p, :n],
                                      sd2[p, :n], case["sdd"][p, :n]))
    return recs


def run(env, case, host=False, counts=None, use_status=True, from_sd=False, skip=()):
    """One call of Engine.check_rows on sentinel-filled outputs; returns them as numpy arrays."""
    torch = env["torch"]
    conv = (lambda x: np.ascontiguousarray(x)) if host else (lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(env["dev"]))
    inp = {k: conv(case[k]) for k in ("a", "b", "lower", "upper")}
    sol = {"sdd": conv(case["sdd"])}
    sol["sd" if from_sd else "sd2"] = conv(case["sd" if from_sd else "sd2"])
    if use_status:
        sol["status"] = conv(case["status"])
    out = {k: conv(np.full(B, PRE if k == "worst_excess" else PRE_INT, np.float64 if k == "worst_excess" else np.int32))
           for k in cr.KEYS}
    for k in skip:
        out[k] = None
    ns = None if counts is None else conv(np.asarray(counts, np.int32))
    got = env["E"].check_rows(inp, sol, outputs=out, num_samples_per_path=ns, host=host)
    if not host:
        torch.cuda.synchronize()
    return {k: (None if v is None else (v if host else v.cpu().numpy())) for k, v in got.items()}


def assert_records(got, want, what):
    for p in range(B):
        assert cr.same_record(cr.record_of(got, p), want[p]), (what, p, cr.record_of(got, p), want[p])


@pytest.fixture(scope="module")
def cases():
    return {s: make_case(*s) for s in SHAPES}


@pytest.mark.parametrize("shape", SHAPES)
def test_records_match_the_reference(env, cases, shape):
    case = cases[shape]
    N, C = shape
    want = expected(case)
    # what the inputs are there for
    assert want[0][1] == 5.0 and (want[0][2], want[0][3]) == (0, 0)               # the tie
    kinds = (np.arange(N * C) % 5)
    assert want[1][0] == int(((kinds == 2) | (kinds == 4)).sum())                 # the kTiny edge
    assert want[3][0] == 0 and np.isnan(want[3][1]) and want[3][2:] == (-1, -1, -1)
    assert want[4] is cr.NOT_CHECKED
    dev = run(env, case)
    assert_records(dev, want, "device")
    host = run(env, case, host=True)
    assert_records(host, want, "host")
    assert_records(run(env, case, use_status=False), expected(case, use_status=False), "no status")
    assert_records(run(env, case, from_sd=True), expected(case, from_sd=True), "sd in place of sd2")


@pytest.mark.parametrize("shape", SHAPES)
def test_ragged_counts(env, cases, shape):
    case = cases[shape]
    N = shape[0]
    counts = [N, max(2, N // 2), N + 1, 1, 2]
    case = dict(case, status=np.zeros(B, np.int32))
    want = expected(case, counts)
    assert want[2] is cr.NOT_CHECKED and want[3] is cr.NOT_CHECKED and want[4][0] >= 0
    assert_records(run(env, case, counts=counts), want, "device")
    assert_records(run(env, case, counts=counts, host=True), want, "host")


def test_optional_outputs(env, cases):
    case = cases[(65, 14)]
    want = expected(case)
    optional = cr.KEYS[1:]
    for host in (False, True):
        got = run(env, case, host=host, skip=optional)
        assert [int(x) for x in got["violations"]] == [w[0] for w in want]
        assert all(got[k] is None for k in optional)
        for keep in optional:
            got = run(env, case, host=host, skip=[k for k in optional if k != keep])
            i = cr.KEYS.index(keep)
            for p in range(B):
                assert np.float64(got[keep][p]).tobytes() == np.float64(want[p][i]).tobytes(), (host, keep, p)


def test_call_level_errors_write_nothing(env):
    eng, torch = env["eng"], env["torch"]
    case = make_case(3, 65)                       # C = 65 is outside 1..64
    conv = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(env["dev"])
    for host in (False, True):
        cv = (lambda x: np.ascontiguousarray(x)) if host else conv
        out = {k: cv(np.full(B, PRE if k == "worst_excess" else PRE_INT, np.float64 if k == "worst_excess" else np.int32))
               for k in cr.KEYS}
        inp = {k: cv(case[k]) for k in ("a", "b", "lower", "upper")}
        sol = {"sd2": cv(case["sd2"]), "sdd": cv(case["sdd"])}
        with pytest.raises(eng.TpamdError, match="-3"):
            env["E"].check_rows(inp, sol, outputs=out, host=host)
        ok = make_case(3, 2)
        inp = {k: cv(ok[k]) for k in ("a", "b", "lower", "upper")}
        for bad in ({"sd2": cv(ok["sd2"])}, {"sdd": cv(ok["sdd"])}):       # no sdd; neither sd2 nor sd
            with pytest.raises(eng.TpamdError, match="-1"):
                env["E"].check_rows(inp, bad, outputs=out, host=host)
        with pytest.raises(eng.TpamdError, match="-1"):                       # no violations array
            env["E"].check_rows(inp, {"sd2": cv(ok["sd2"]), "sdd": cv(ok["sdd"])},
                                outputs=dict(out, violations=None), host=host)
        with pytest.raises(eng.TpamdError, match="-1"):                       # a missing row array
            env["E"].check_rows(dict(inp, upper=None), {"sd2": cv(ok["sd2"]), "sdd": cv(ok["sdd"])}, outputs=out,
                                host=host)
        if not host:
            torch.cuda.synchronize()
        for k in cr.KEYS:
            v = out[k] if host else out[k].cpu().numpy()
            assert (v == (PRE if k == "worst_excess" else PRE_INT)).all(), (host, k)

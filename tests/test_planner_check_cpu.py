"""The host side of planner-set checking, without a GPU (host/solution_check.h through the stand-alone
driver tests/cpp/test_planner_check_record.cc, built with g++ -ffp-contract=off and once more with
-fsanitize=address,undefined):

  * CheckSolutionRows -- what TimeOptimalPathProfile::GetSolutionCheckRecord returns -- equals
    check_reference.check_rows bit for bit on random rows and on planted edge cases;
  * MergeWindowRecord over 1..5 windows equals a numpy restatement of the cross-window rule;
  * tpamd_planner_check is 48 bytes and its field offsets are those of PLANNER_CHECK_DTYPE."""
import ctypes
import importlib
import os
import subprocess

import numpy as np
import pytest

import check_reference as cr
from conftest import PKG_NAME
from native_driver import build_driver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "test_planner_check_record.cc")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    exe = build_driver(SOURCE, tmp_path_factory.mktemp("planner_check"), flags=flags, name="driver_" + request.param)

    def run(text, tmp=os.path.dirname(exe)):
        path = os.path.join(tmp, "cases.txt")
        with open(path, "w") as f:
            f.write(text)
        out = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
        return [line.split() for line in out.stdout.splitlines()]
    return run


def _hex(values):
    return " ".join(float(v).hex() for v in np.asarray(values, dtype=np.float64).reshape(-1))


def _rows_case(A, B, lo, hi, sd2, sdd):
    N, C = A.shape
    return "rows %d %d\n%s\n" % (N, C, "\n".join(_hex(x) for x in (A, B, lo, hi, sd2, sdd)))


def _rows_record(fields):
    assert fields[0] == "rows"
    return (int(fields[1]), float.fromhex(fields[2]) if "nan" not in fields[2] else float(fields[2]),
            int(fields[3]), int(fields[4]), int(fields[5]))


def planted_cases():
    KT = cr.KT
    one = lambda x: np.array(x, dtype=np.float64)
    A = one([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
    B = one([[0.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    lo = np.full((3, 2), -10.0)
    sd2, sdd = one([2.0, 2.0, 2.0]), one([0.5, 0.5, 0.5])
    cases = {}
    # ties in the excess: every row has the same margin; two violated rows with the same excess
    cases["tie_margin"] = (A, B, lo, np.full((3, 2), 10.0), sd2, sdd)
    cases["tie_violated"] = (A, B, lo, one([[10.0, 1.0], [10.0, 1.0], [10.0, 10.0]]), sd2, sdd)
    # NaN rows among good ones, NaN in the solution, and nothing but NaN
    cases["nan_rows"] = (A * one([[np.nan, 1.0], [1.0, 1.0], [1.0, np.nan]]), B, lo, np.full((3, 2), 1.0), sd2, sdd)
    cases["nan_bounds"] = (A, B, one([[np.nan, -10.0]] * 3), one([[10.0, np.nan]] * 3), sd2, sdd)
    cases["nan_solution"] = (A, B, lo, np.full((3, 2), 1.0), sd2, one([0.5, np.nan, 0.5]))
    cases["all_nan"] = (A, B, lo, np.full((3, 2), 10.0), np.full(3, np.nan), np.full(3, np.nan))
    # an excess of +0 (lower == v) and of -0 (v = -0, upper = +0), alone and tied with each other
    zA, zB = one([[1.0], [1.0]]), one([[0.0], [0.0]])
    cases["plus_zero"] = (zA, zB, one([[0.5], [0.0]]), one([[9.0], [9.0]]), one([1.0, 1.0]), one([0.5, 1.0]))
    # (b = -0 keeps the sum at -0: -0 + +0 would be +0)
    cases["minus_zero"] = (zA, -zB, one([[-1.0], [-1.0]]), one([[0.0], [1.0]]), one([1.0, 1.0]), one([-0.0, 0.0]))
    cases["zero_tie"] = (zA, -zB, one([[-1.0], [0.0]]), one([[0.0], [9.0]]), one([1.0, 1.0]), one([-0.0, 0.0]))
    # the kTiny edge: v - kTiny == upper is kept, one ulp further is violated; the same below
    hi = one([[0.5 - KT, 10.0], [np.nextafter(0.5 - KT, -np.inf), 10.0], [10.0, 10.0]])
    cases["ktiny_upper"] = (A, B, lo, hi, sd2, sdd)
    low = one([[0.5 + KT, -10.0], [np.nextafter(0.5 + KT, np.inf), -10.0], [-10.0, -10.0]])
    cases["ktiny_lower"] = (A, B, low, np.full((3, 2), 10.0), sd2, sdd)
    return cases


def random_cases():
    rng = np.random.default_rng(2024)
    cases = {}
    for C in (1, 2, 14, 34):
        for N in (3, 64, 257):
            A, B = rng.normal(size=(N, C)), rng.normal(size=(N, C)) ** 2
            sd2, sdd = rng.uniform(0.0, 2.0, N), rng.normal(size=N)
            v = A * sdd[:, None] + B * sd2[:, None]
            # bounds around v: most rows with margin, some violated on either side, some at the bound
            lo = v - rng.uniform(0.0, 1.0, (N, C)) * (rng.uniform(size=(N, C)) > 0.05)
            hi = v + rng.uniform(0.0, 1.0, (N, C)) * (rng.uniform(size=(N, C)) > 0.05)
            flip = rng.uniform(size=(N, C)) < 0.03
            hi = np.where(flip, v - rng.uniform(0.0, 0.5, (N, C)), hi)
            cases["random_%d_%d" % (C, N)] = (A, B, lo, hi, sd2, sdd)
    return cases


def test_record_equals_check_rows(driver):
    cases = {**planted_cases(), **random_cases()}
    got = driver("".join(_rows_case(*c) for c in cases.values()))
    assert len(got) == len(cases)
    violated = 0
    for (name, c), fields in zip(cases.items(), got):
        want = cr.check_rows(*c)
        assert cr.same_record(_rows_record(fields), want), (name, fields, want)
        violated += want[0] > 0
    assert violated >= 12          # the random cases hold both outcomes
    want = {name: cr.check_rows(*c) for name, c in planted_cases().items()}
    assert want["tie_margin"] == (0, -8.0, 0, 1, -1)
    assert want["tie_violated"][0] == 2 and want["tie_violated"][2:] == (0, 1, 0)
    assert cr.same_record(want["all_nan"], (0, np.nan, -1, -1, -1))
    assert cr.same_record(want["plus_zero"], (0, 0.0, 0, 0, -1))
    assert cr.same_record(want["minus_zero"], (0, -0.0, 0, 0, -1))
    assert cr.same_record(want["zero_tie"], (0, -0.0, 0, 0, -1))
    assert want["ktiny_upper"][0] == 1 and want["ktiny_upper"][4] == 1
    assert want["ktiny_lower"][0] == 1 and want["ktiny_lower"][4] == 1


def merge_reference(windows):
    """The cross-window rule of include/tpamd.h on (violations, excess, sample, row, first, s) per window."""
    rec = dict(windows=0, violations=-1, last=-1, worst=(-1, -1, -1), first=(-1, -1), excess=np.nan, s=np.nan)
    best = None
    for w, (count, excess, sample, row, first, s) in enumerate(windows):
        rec["windows"] += 1
        rec["violations"] = max(rec["violations"], 0) + count
        rec["last"] = count
        if sample >= 0:
            key = (-excess, w, sample, row)          # the larger excess, then the smaller (window, sample, row)
            if best is None or key < best:
                best = key
                rec["worst"], rec["excess"], rec["s"] = (w, sample, row), excess, s
        if first >= 0 and rec["first"] == (-1, -1):
            rec["first"] = (w, first)
    return (rec["windows"], rec["violations"], rec["last"]) + rec["worst"] + rec["first"] + (rec["excess"], rec["s"])


def test_merge_equals_the_cross_window_rule(driver):
    nan = np.nan
    clean = lambda e, i, s: (0, e, i, 0, -1, s)
    cases = [
        [(3, 2.5, 4, 1, 2, 0.25)],
        [clean(-0.5, 7, 0.1), (2, 1.5, 3, 2, 3, 0.2), clean(-0.25, 0, 0.3), (1, 0.75, 9, 0, 9, 0.4)],   # a clean first window
        [(1, 1.5, 8, 3, 8, 0.1), (1, 1.5, 2, 0, 2, 0.2)],                      # equal excesses: the earlier window
        [(2, 1.0, 1, 1, 1, 0.1), clean(-1.0, 0, 0.2), (4, 3.0, 5, 6, 0, 0.3), clean(-2.0, 3, 0.4), (1, 3.0, 0, 0, 0, 0.5)],
        [(0, nan, -1, -1, -1, nan), clean(-0.125, 6, 0.7)],                    # a window without any excess
        [(0, nan, -1, -1, -1, nan)],
        [clean(-0.0, 1, 0.1), clean(0.0, 0, 0.2)],                             # -0 == +0: the earlier window stays
    ]
    rng = np.random.default_rng(5)
    for W in range(1, 6):
        for _ in range(8):
            case = []
            for _ in range(W):
                count = int(rng.integers(0, 3))
                case.append((count, float(rng.integers(-3, 3)) / 2, int(rng.integers(0, 5)), int(rng.integers(0, 4)),
                             int(rng.integers(0, 5)) if count else -1, float(rng.uniform())))
            cases.append(case)
    text = ""
    for case in cases:
        text += "merge %d\n" % len(case)
        for count, excess, sample, row, first, s in case:
            text += "%d %s %d %d %d %s\n" % (count, float(excess).hex(), sample, row, first, float(s).hex())
    got = driver(text)
    assert len(got) == len(cases)
    for case, fields in zip(cases, got):
        want = merge_reference(case)
        assert fields[0] == "merge"
        assert tuple(int(x) for x in fields[1:9]) == tuple(want[:8]), (case, fields, want)
        for text_value, value in zip(fields[9:], want[8:]):
            value_got = float(text_value) if "nan" in text_value else float.fromhex(text_value)
            assert np.float64(value_got).tobytes() == np.float64(value).tobytes(), (case, fields, want)
    assert merge_reference(cases[2])[3:6] == (0, 8, 3)
    assert merge_reference(cases[1])[6:8] == (1, 3)


def test_struct_layout(driver):
    eng = importlib.import_module(PKG_NAME + ".engine")
    dt = eng.PLANNER_CHECK_DTYPE
    assert dt.itemsize == 48 and ctypes.sizeof(eng._PlannerCheck) == 48
    offsets = [dt.fields[n][1] for n in dt.names]
    assert offsets == [getattr(eng._PlannerCheck, n).offset for n in dt.names]
    (fields,) = driver("layout\n")
    assert [int(x) for x in fields[1:]] == [48] + offsets
    for name in ("tpamd_planner_set_set_checking", "tpamd_planner_set_checking", "tpamd_planner_set_check_results",
                 "tpamd_planner_set_check_results_device"):
        assert name in eng.ABI_SYMBOLS

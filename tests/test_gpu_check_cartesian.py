"""The solution check for Cartesian batches on the GPU (tpamd_check_cartesian_paths_*,
Engine.check_cartesian_paths).

The engine solves the synthetic Cartesian batches of tests/check_reference.py (asking for sd2), then
checks its own solution and the same solution 1 % too fast. Every comparison is bit equality (NaN by
position) on sentinel-filled outputs:
  * against tests/check_reference.py on the ORACLE's rows (tpo.cartesian_path_derivatives +
    tpo.cartesian_constraint_setup, J q' summed over the joints in index order);
  * violations against the oracle's constraint_violations() of its own solve;
  * strided uniform, strided ragged (counts from 1 to N + 1, the two ends refused) and packed row
    tables through first_row with reordered and overlapping ranges, each against the uniform check
    of every path alone; _host against _device."""
import importlib

import numpy as np
import pytest

import check_reference as cr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

PRE, PRE_INT = -7.25, -9
NAMES = dict(ik_positions="ik_positions", jacobians="jacobians", vmax="max_velocity", amax="max_acceleration",
             vtrans="max_translational_velocity", vrot="max_rotational_velocity", path_start="path_start",
             delta="delta", sd_start="sd_start", time_start="time_start")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    from oracle import tpo
    tpo.build()
    return dict(torch=torch, eng=eng, syn=syn, tpo=tpo, E=eng.Engine(0), dev="cuda:0")


def _up(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _sentinels(B):
    return {k: np.full(B, PRE if k == "worst_excess" else PRE_INT, np.float64 if k == "worst_excess" else np.int32)
            for k in cr.KEYS}


def _inputs(batch):
    return {NAMES[k]: batch[k] for k in NAMES}


def solve(env, batch, B, N, counts=None, first=None):
    torch = env["torch"]
    out = {k: torch.full((B, N), PRE, dtype=torch.float64, device=env["dev"]) for k in ("time", "s", "sd", "sdd", "sd2")}
    out["status"] = torch.full((B,), PRE_INT, dtype=torch.int32, device=env["dev"])
    env["E"].time_cartesian_paths({k: _up(env, v) for k, v in _inputs(batch).items()}, out, safety=batch["safety"],
                                  num_samples_per_path=_up(env, counts), first_row=_up(env, first))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(env, batch, B, sol, counts=None, first=None, host=False, with_status=True):
    conv = (lambda a: None if a is None else np.ascontiguousarray(a)) if host else (lambda a: _up(env, a))
    solution = {k: conv(sol[k]) for k in ("sd2", "sdd")}
    if with_status:
        solution["status"] = conv(sol["status"])
    got = env["E"].check_cartesian_paths({k: conv(v) for k, v in _inputs(batch).items()}, solution,
                                         safety=batch["safety"], num_samples_per_path=conv(counts),
                                         first_row=conv(first), outputs={k: conv(v) for k, v in _sentinels(B).items()},
                                         host=host)
    if host:
        return got
    env["torch"].cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def path_rows(batch, b, n, first=None):
    """q [n][D], J [n][6][D] of path b: strided, or rows first[b] .. of the packed tables."""
    if first is None:
        return batch["ik_positions"][b, :n], batch["jacobians"][b, :n]
    r = int(first[b])
    return batch["ik_positions"][r:r + n], batch["jacobians"][r:r + n]


def expected(env, batch, B, N, sol, counts=None, first=None, with_status=True):
    recs = []
    for b in range(B):
        n = N if counts is None else int(counts[b])
        if (with_status and sol["status"][b] != 0) or n < 2 or n > N:
            recs.append(cr.NOT_CHECKED)
            continue
        q, J = path_rows(batch, b, n, first)
        rows = cr.cartesian_rows(env["tpo"], q, J, batch["vmax"][b], batch["amax"][b], batch["vtrans"][b],
                                 batch["vrot"][b], batch["delta"][b], batch["safety"])
        recs.append(cr.check_rows(*rows, sol["sd2"][b, :n], sol["sdd"][b, :n]))
    return recs


def alone(env, batch, B, N, sol, counts=None, first=None, with_status=True):
    """The uniform check of every path alone (None where the batch call must not check the path)."""
    recs = []
    for b in range(B):
        n = N if counts is None else int(counts[b])
        if n < 3 or n > N:                      # (a uniform call needs 3 samples; 2 is covered by `expected`)
            recs.append(None)
            continue
        q, J = path_rows(batch, b, n, first)
        one = {k: np.ascontiguousarray(batch[k][b:b + 1]) for k in NAMES if k not in ("ik_positions", "jacobians")}
        one.update(ik_positions=np.ascontiguousarray(q[None]), jacobians=np.ascontiguousarray(J[None]),
                   safety=batch["safety"])
        s1 = {k: np.ascontiguousarray(sol[k][b:b + 1, :n]) for k in ("sd2", "sdd")}
        s1["status"] = sol["status"][b:b + 1]
        recs.append(cr.record_of(check(env, one, 1, s1, with_status=with_status), 0))
    return recs


def assert_records(got, want, what):
    for b, w in enumerate(want):
        if w is not None:
            assert cr.same_record(cr.record_of(got, b), w), (what, b, cr.record_of(got, b), w)


def variants(sol):
    fast = dict(sol, sd2=sol["sd2"] * 1.01)
    return (("own", sol, True), ("1.01", fast, True), ("1.01, no status", fast, False))


@pytest.mark.parametrize("shape", cr.CARTESIAN_SHAPES)
def test_uniform_strided(env, shape):
    D, N, W = shape
    B = cr.cartesian_paths(shape)
    batch = env["syn"].make_cartesian_batch(B, D, N, W)
    sol = solve(env, batch, B, N)
    assert (sol["status"] == 0).all()
    got = check(env, batch, B, sol)
    for b, (rc, viol, _, _) in enumerate(cr.oracle_counts(env["tpo"], batch, cartesian=True)):
        assert rc == 0 and got["violations"][b] == viol, (b, got["violations"][b], viol)
    for name, s, with_status in variants(sol):
        want = expected(env, batch, B, N, s, with_status=with_status)
        # (the three-sample shape has one free sample, which the solver leaves far inside its rows: no
        # factor violates one there; its worst excess and indices still tell a kernel's answer apart)
        if name != "own" and N > 3:
            assert any(w[0] > 0 for w in want), "the expectation must hold violated rows"
        assert_records(check(env, batch, B, s, with_status=with_status), want, (name, "device"))
        assert_records(check(env, batch, B, s, with_status=with_status, host=True), want, (name, "host"))
    assert_records(got, alone(env, batch, B, N, sol), "each path alone")


@pytest.mark.parametrize("shape", cr.CARTESIAN_SHAPES)
def test_ragged_strided_and_packed(env, shape):
    D, N, W = shape
    B = cr.cartesian_paths(shape)
    batch = env["syn"].make_cartesian_batch(B, D, N, W)
    cycle = [N, max(2, N // 2), max(2, N - 1), 3, 2, N + 1, 1, max(2, N // 3)]
    counts = np.array([cycle[b % len(cycle)] for b in range(B)], np.int32)
    # strided
    sol = solve(env, batch, B, N, counts)
    for name, s, with_status in variants(sol):
        want = expected(env, batch, B, N, s, counts, with_status=with_status)
        assert want[5] is cr.NOT_CHECKED and want[6] is cr.NOT_CHECKED
        got = check(env, batch, B, s, counts, with_status=with_status)
        assert_records(got, want, (name, "strided"))
        assert_records(check(env, batch, B, s, counts, with_status=with_status, host=True), want, (name, "strided host"))
        assert_records(got, alone(env, batch, B, N, s, counts, with_status=with_status), (name, "strided, alone"))
    # packed: the usable paths' rows in a shuffled order; every fourth path reads from the middle of
    # its predecessor's range instead (an overlap), and two rows of NaN end the table
    usable = [b for b in range(B) if 2 <= counts[b] <= N]
    order = np.random.default_rng(7 + D).permutation(usable)
    first = np.zeros(B, np.int32)
    tq, tj, r = [], [], 0
    for b in order:
        n = int(counts[b])
        first[b] = r
        tq.append(batch["ik_positions"][b, :n])
        tj.append(batch["jacobians"][b, :n])
        r += n
    tq = np.concatenate(tq + [np.full((2, D), np.nan)])
    tj = np.concatenate(tj + [np.full((2, 6, D), np.nan)])
    for b in usable[3::4]:
        prev = usable[usable.index(b) - 1]
        n = min(int(counts[b]), int(counts[prev]))
        counts[b] = max(2, n - 1)
        first[b] = first[prev] + (n - counts[b])
    packed = dict(batch, ik_positions=tq, jacobians=tj)
    sol = solve(env, packed, B, N, counts, first)
    checked = 0
    for name, s, with_status in variants(sol):
        want = expected(env, packed, B, N, s, counts, first, with_status=with_status)
        checked += sum(w is not cr.NOT_CHECKED for w in want)
        got = check(env, packed, B, s, counts, first, with_status=with_status)
        assert_records(got, want, (name, "packed"))
        assert_records(check(env, packed, B, s, counts, first, with_status=with_status, host=True), want,
                       (name, "packed host"))
        assert_records(got, alone(env, packed, B, N, s, counts, first, with_status=with_status), (name, "packed, alone"))
    assert checked >= B // 2

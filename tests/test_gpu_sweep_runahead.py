"""The loop queue of the joint sweep (csrc/tpamd_sweep_joint.h, "loop queue"): the forward wave posts the
switching-point loops and runs ahead, the backward wave takes them in order. Every output bit for
bit against the CPU oracle -- status, last_extremal_index, time, s, sd, sdd, q, qd, qdd on solved
paths -- on inputs with many loops on few samples (runahead_cases.py), under solver loop limits, in
every pipelining mode, ragged, Cartesian, without qd/qdd and on long paths; one batch solved a
hundred times gives the same bytes; and no path anywhere reports TPAMD_PATH_SWEEP_POLL_EXPIRED (12),
the exit of a bounded wait between the two waves.

Statuses: inputs on which the oracle ends with "no connection" (7), "non-zero end" (9) or "critical
index zero" (10) without a loop limit were searched for on the CPU with tools/search_failing_statuses.py
-- joint-spline and Cartesian paths from every generator the tests have, 3..257 samples, limits scaled
over five to seven decades, start velocities, overshooting horizons, scaled control points: 4000
cases, 106 672 paths (profiles/sweep_runahead_status_search.json) -- and none exists there: the oracle
solves them all. What the joint sweep can be made to fail with is a loop limit, status 8 (NaN in
sd2), compared per path below at limits 1, 2 and 3. The generic rows kernel, which does reach 7, 9
and 10 (tests/test_gpu_parity.py), has no loop queue. Which code of the queue is therefore covered by
reasoning only is listed in profiles/sweep_runahead_ab.md."""
import importlib

import numpy as np
import pytest

import cartesian_paths as cp
import runahead_cases as rc
import structured_paths as sp
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

KEYS = ("time", "s", "sd", "sdd", "q", "qd", "qdd")
POLL_EXPIRED = 12


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    from oracle import tpo
    return dict(torch=torch, eng=eng, syn=syn, tpo=tpo, E=eng.Engine(0), dev="cuda:0")


def _solve(env, E, b, N, max_loops=0, **alloc):
    eng, torch = env["eng"], env["torch"]
    B, _, D = b["control_points"].shape
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"], **alloc)
    E.time_joint_paths(inp, out, N, max_solver_loops=max_loops)
    E.fence()
    torch.cuda.synchronize()
    return inp, out


def _assert_bit_parity(out, ref, what, keys=KEYS):
    st = out["status"].cpu().numpy()
    assert not (st == POLL_EXPIRED).any(), "%s: a bounded wait of the sweep ran out" % what
    np.testing.assert_array_equal(st, ref["status"], err_msg=what)
    ok = st == 0
    np.testing.assert_array_equal(out["last_extremal_index"].cpu().numpy()[ok],
                                  ref["last_extremal_index"][ok], err_msg=what)
    for k in keys:
        g = out[k].cpu().numpy()
        r = ref["t" if k == "time" else k]
        np.testing.assert_array_equal(g[ok], r[ok], err_msg="%s %s" % (what, k))
    return ok


@pytest.fixture(scope="module")
def long_batch(env):
    """64 paths x 7 joints x 2000 samples with tightened limits and the oracle's solution, once."""
    b = rc.tight_batch(7, 2000, B=64, first=500)
    ref = sp.oracle_solve(env["tpo"], b, 2000, nthreads=16)
    assert (ref["status"] == 0).all()
    return b, ref


@pytest.mark.parametrize("D", rc.DOFS)
@pytest.mark.parametrize("N", rc.SAMPLES)
def test_many_loops_on_few_samples(env, D, N):
    """Tightened limits: 9..27 loops per path, switching points a few samples apart. All 32 paths
    are solved, by the oracle and here."""
    b = rc.tight_batch(D, N)
    ref = sp.oracle_solve(env["tpo"], b, N)
    assert (ref["status"] == 0).all()
    _, out = _solve(env, env["E"], b, N)
    assert _assert_bit_parity(out, ref, "D=%d N=%d" % (D, N)).all()


@pytest.mark.parametrize("shape", rc.FAMILY_SHAPES, ids=lambda s: "D%d-N%d" % s)
@pytest.mark.parametrize("family", rc.FAMILIES)
def test_structured_families(env, family, shape):
    """Stationary stretches (runs of equal limit-curve values, switching points next to each
    other) and paths that never touch the limit curve (no loop: the first pair in order, an end
    entry as the only post)."""
    D, N = shape
    b = rc.family_batch(family, D, N)
    ref = sp.oracle_solve(env["tpo"], b, N)
    assert (ref["status"] == 0).all()
    _, out = _solve(env, env["E"], b, N)
    assert _assert_bit_parity(out, ref, "%s D=%d N=%d" % (family, D, N)).all()


@pytest.mark.parametrize("limit", [1, 2, 3])
def test_solver_loop_limits_status_per_path(env, limit):
    """At most `limit` entries are posted, then the end entry; the oracle's solver takes the same
    limit. Status per path; the arrays of the paths that limit still solves."""
    D, N, B = 7, 257, 16
    b = sp.concat([rc.family_batch("tie_mirror", D, N, B=8), rc.family_batch("stop_interior", D, N, B=4),
                   rc.family_batch("velocity_bound", D, N, B=4)])
    want = [rc.oracle_with_loop_limit(env["tpo"], b, i, N, limit) for i in range(B)]
    _, out = _solve(env, env["E"], b, N, max_loops=limit)
    st = out["status"].cpu().numpy()
    assert not (st == POLL_EXPIRED).any()
    np.testing.assert_array_equal(st, np.array([w[0] for w in want]))
    assert (st != 0).any() and (st == 0).any()         # the limit bites, and not everywhere
    for i, (s, r) in enumerate(want):
        if s != 0:
            continue
        for k in ("time", "s", "sd", "sdd"):
            np.testing.assert_array_equal(out[k][i].cpu().numpy(), r["t" if k == "time" else k],
                                          err_msg="limit %d path %d %s" % (limit, i, k))


def test_one_batch_a_hundred_times_the_same_bytes(env):
    """Which wave reaches a switching point first differs from run to run; the bytes do not."""
    torch = env["torch"]
    b = rc.tight_batch(7, 300, B=64, first=900)
    ref = sp.oracle_solve(env["tpo"], b, 300)
    inp, first = _solve(env, env["E"], b, 300)
    assert _assert_bit_parity(first, ref, "first solve").all()
    names = KEYS + ("status", "last_extremal_index", "max_time_increment")
    names = tuple(k for k in names if k in first)
    keep = {k: first[k].clone() for k in names}
    out = env["eng"].alloc_joint_outputs(64, 300, 7, env["dev"])
    differing = 0
    for _ in range(99):
        for k in names:
            out[k].zero_()
        env["E"].time_joint_paths(inp, out, 300)
        env["E"].fence()
        for k in names:
            a, c = out[k], keep[k]
            same = torch.equal(a.view(torch.int64), c.view(torch.int64)) if a.dtype == torch.float64 \
                else torch.equal(a, c)
            differing += 0 if same else 1
    torch.cuda.synchronize()
    assert differing == 0


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_long_paths_through_every_pipelining_mode(env, long_batch, mode):
    b, ref = long_batch
    E = env["eng"].Engine(0)
    E.set_pipelining(mode)
    try:
        _, out = _solve(env, E, b, 2000)
        assert _assert_bit_parity(out, ref, "pipelining mode %d" % mode).all()
    finally:
        E.close()


def test_without_qd_and_qdd(env, long_batch):
    """No emission: the backward wave goes from one entry straight to the wait for the next."""
    b, ref = long_batch
    _, out = _solve(env, env["E"], b, 2000, with_derivs=False)
    assert "qd" not in out and "qdd" not in out
    assert _assert_bit_parity(out, ref, "no derivatives", keys=("time", "s", "sd", "sdd")).all()


def test_cartesian_batch_with_extra_rows(env):
    """D = 6 with the two Cartesian rows (E = 2) at N = 129."""
    torch, eng, syn, tpo = env["torch"], env["eng"], env["syn"], env["tpo"]
    N = 129
    b = cp.concat([cp.with_starts(cp.make_family(f, 8, 6, N, seed=6), seed=k)
                   for k, f in enumerate(("singular", "idle"))])
    ref = cp.oracle_solve(tpo, b)
    out = eng.alloc_joint_outputs(16, N, 6, env["dev"])
    env["E"].time_cartesian_paths(syn.upload_cartesian_batch(b, env["dev"]), out)
    torch.cuda.synchronize()
    ok = _assert_bit_parity(out, ref, "cartesian D=6 N=%d" % N)
    assert ok.all(), ref["status"]


def test_ragged_sample_counts_nothing_past_the_end(env):
    torch, eng, tpo, E = (env[k] for k in ("torch", "eng", "tpo", "E"))
    D, stride = 7, 600
    counts = np.array([130, 257, 600, 599, 131, 64, 65, 33, 300, 511, 512, 513, 200, 77, 450, 258],
                      dtype=np.int32)
    B = len(counts)
    b = rc.tight_batch(D, stride, B=B, first=300)
    b["delta"] = np.ascontiguousarray(b["knots"][:, -1] / (counts - 1))
    inp = eng.upload_joint_batch(b, env["dev"])
    inp["num_samples_per_path"] = torch.from_numpy(counts).to(env["dev"])
    out = eng.alloc_joint_outputs(B, stride, D, env["dev"])
    for k in KEYS:
        out[k].fill_(-7.0)
    E.time_joint_paths(inp, out, stride)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in KEYS}
    st = out["status"].cpu().numpy()
    lei = out["last_extremal_index"].cpu().numpy()
    for i, n in enumerate(counts):
        one = {k: b[k][i:i + 1] for k in ("knots", "control_points", "vmax", "amax", "path_start",
                                          "delta", "sd_start", "time_start")}
        one["safety"] = b["safety"]
        ref = sp.oracle_solve(tpo, one, int(n), nthreads=1)
        assert st[i] == ref["status"][0] == 0, (i, n)
        assert lei[i] == ref["last_extremal_index"][0], (i, n)
        for k in KEYS:
            np.testing.assert_array_equal(got[k][i, :n], ref["t" if k == "time" else k][0],
                                          err_msg="%s path %d n %d" % (k, i, n))
            assert (got[k][i, n:] == -7.0).all(), "wrote past n[b]"

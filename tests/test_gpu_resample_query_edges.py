"""The uniform resampler (k_resample), the skip resampler (k_resample_skip) and the s(t) query
(k_query) at every joint count and at their edges, bit for bit against the independent restatement
tests/resample_reference.py and, where it has the call, against the oracle. The inputs come from
tests/resample_cases.py; tests/test_resample_reference_cpu.py holds the restatement to the oracle
on them and asserts that they reach the branches named here.

Every output array is filled with a sentinel before the call and carries a guard of 256 slots
behind its last row; every slot the call must not write still holds the sentinel afterwards, and
count / ok start at -5. A row cut by max_out is compared below max_out only: the end sample is
special only if it is among the written slots."""
import ctypes as C
import functools
import importlib

import numpy as np
import pytest

import resample_cases as rc
import resample_reference as rr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
OUT = ("out_time", "out_s", "out_sd", "out_sdd", "out_q", "out_qd", "out_qdd")
GUARD = 256             # slots behind the last row: a 256-lane block that ignored max_out would land here


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(eng=eng, tpo=tpo, torch=torch, E=eng.Engine(0), dev=torch.device("cuda", 0))


def _up(env, a):
    return None if a is None else env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"])


def _guarded(env, shape, value, dtype=np.float64):
    """A device array of `shape` filled with value, with GUARD more rows of shape[1:] behind it.
    Returns (view of the array, the guard)."""
    rows = int(np.prod(shape[1:], dtype=np.int64)) if len(shape) > 1 else 1
    width = 1 if len(shape) < 3 else shape[2]
    flat = _up(env, np.full(shape[0] * rows + GUARD * width, value, dtype=dtype))
    return flat[:shape[0] * rows].view(*shape), flat[shape[0] * rows:]


# ---------------------------------------------------------------------------- resamplers
def _resample(env, case, max_out, skip=False, host=False):
    """tpamd_resample_{uniform,skip}_device (through Engine.resample_uniform) or _host into
    sentinel-filled outputs; returns them as numpy arrays."""
    torch, eng, E = env["torch"], env["eng"], env["E"]
    sol, amax = case["sol"], case["amax"]
    B, N, D = sol["q"].shape
    shape = lambda k: (B, max_out) + ((D,) if k in OUT[4:] else ())
    status = case.get("status")
    if host:
        out = {k: np.full(shape(k), SENTINEL) for k in OUT}
        out["count"] = np.full(B, -5, dtype=np.int32)
        start = np.ascontiguousarray(case["start"])
        args = eng._ResampleArgs(B, N, D, max_out, *[eng._ptr(np.ascontiguousarray(sol[k])) for k in rc.SOL],
                                 eng._ptr(amax), eng._ptr(start), float(case["dt"]), eng._ptr(status),
                                 *[eng._ptr(out[k]) for k in OUT + ("count",)])
        fn = E._lib.tpamd_resample_skip_host if skip else E._lib.tpamd_resample_uniform_host
        rc_ = fn(E._h, C.byref(args))
        assert rc_ == 0, E._lib.tpamd_error_string(rc_)
        return out
    dsol = {k: _up(env, sol[k]) for k in rc.SOL}
    dsol["status"] = _up(env, status)
    dout, guards = {}, {}
    for k in OUT:
        dout[k], guards[k] = _guarded(env, shape(k), SENTINEL)
    dout["count"], guards["count"] = _guarded(env, (B,), -5, np.int32)
    E.resample_uniform(dsol, _up(env, amax), _up(env, case["start"]), case["dt"], dout, skip=skip)
    torch.cuda.synchronize()
    for k in OUT:
        assert bool((guards[k] == SENTINEL).all()), (k, "written behind the last row")
    assert bool((guards["count"] == -5).all())
    return {k: v.cpu().numpy() for k, v in dout.items()}


def _reference(case, i, max_out, skip):
    rows = [case["sol"][k][i].tolist() for k in rc.SOL]
    fn = rr.resample_skip if skip else rr.resample_uniform
    return fn(*rows, float(case["start"][i]), case["dt"], case["amax"][i].tolist(), max_out=max_out)


def _check(env, case, max_out, skip=False, what=""):
    """One device call for the batch; every path against the restatement and the oracle. Returns
    the counts."""
    tpo = env["tpo"]
    B, N, D = case["sol"]["q"].shape
    got = _resample(env, case, max_out, skip=skip)
    status = case.get("status")
    counts = []
    for i in range(B):
        if status is not None and status[i] != 0:
            count, ref, full = 0, None, None
        else:
            count, ref = _reference(case, i, max_out, skip)
            full = None
            if count > 0:
                call = tpo.resample_skip if skip else tpo.resample_uniform
                full = call(*[case["sol"][k][i] for k in rc.SOL], float(case["start"][i]), case["dt"], case["amax"][i])
                assert len(full[0]) == count
        assert got["count"][i] == count, (what, i, got["count"][i], count)
        w = max(0, min(count, max_out))
        for j, k in enumerate(OUT):
            if w:
                want = np.array(ref[j], dtype=np.float64).reshape(got[k][i, :w].shape)
                np.testing.assert_array_equal(got[k][i, :w], want, err_msg="%s path %d %s" % (what, i, k))
                np.testing.assert_array_equal(got[k][i, :w], full[j][:w], err_msg="%s path %d %s (oracle)" % (what, i, k))
            assert (got[k][i, w:] == SENTINEL).all(), (what, i, k, "written at or above min(count, max_out)")
        counts.append(count)
    return counts, got


@functools.lru_cache(maxsize=None)
def _uniform_counts(name):
    case = EDGES[name]
    return [rr.uniform_count(float(case["sol"]["time"][i, -1]), float(case["start"][i]), case["dt"])
            for i in range(len(case["start"]))]


@pytest.mark.parametrize("D", rc.ALL_DOFS)
def test_uniform_every_joint_count(env, D):
    """D = 1 .. 16, 17, 63, 64, 65; N = 130, B = 4, 4 ms; starts before the first sample
    (extrapolation), inside, on sample 64 and nextafter above it."""
    case = rc.uniform_dof_case(D)
    most = max(rr.uniform_count(float(case["sol"]["time"][i, -1]), float(case["start"][i]), case["dt"]) for i in range(4))
    counts, _ = _check(env, case, most + 3, what="D=%d" % D)
    assert min(counts) > 60


EDGES = rc.uniform_edge_cases()


@pytest.mark.parametrize("name", sorted(EDGES))
def test_uniform_edges(env, name):
    """D = 3. ticks_on_samples: every tick a sample time. past_the_end: starts at the last time
    stamp and 0.5, 1.5, 10 steps past it -- counts 1, 1, 0 and negative, and nothing but count is
    written for the last two. tiny_bracket: two distinct samples closer than epsilon. count_M:
    counts on each side of one and two 256-lane blocks. status: a skipped path. two_samples: N = 2."""
    case = EDGES[name]
    counts, got = _check(env, case, max(max(_uniform_counts(name)), 1) + 3, what=name)
    if name == "past_the_end":
        assert counts[:3] == [1, 1, 0] and counts[3] < 0
        for i in (0, 1):                # the one sample is the end sample: end position, zero qd, qdd
            np.testing.assert_array_equal(got["out_q"][i, 0], case["sol"]["q"][i, -1])
            assert (got["out_qd"][i, 0] == 0).all() and (got["out_qdd"][i, 0] == 0).all()
            assert got["out_time"][i, 0] == case["start"][i] and got["out_s"][i, 0] == case["sol"]["s"][i, -1]
    if name == "status":
        assert counts[1] == 0 and counts[0] > 1 and counts[2] > 1
    if name.startswith("count_"):
        assert counts == [int(name[6:])] * 2


@pytest.mark.parametrize("which", range(5))
def test_uniform_max_out(env, which):
    """A count of 300 against max_out = 300, 299, 256, 255, 1: only slots below max_out are
    written, in the count's own 256-lane block and in an earlier one; count is the full number."""
    case = rc.count_case(rc.MAX_OUT_COUNT)
    max_out = rc.max_outs(rc.MAX_OUT_COUNT)[which]
    counts, _ = _check(env, case, max_out, what="max_out=%d" % max_out)
    assert counts == [rc.MAX_OUT_COUNT] * 2


def test_uniform_host_entry(env):
    """tpamd_resample_uniform_host equals the device entry below each count (the host entry copies
    its whole output arrays back: only those slots say anything)."""
    case = EDGES["count_257"]
    dev = _resample(env, case, 260)
    host = _resample(env, case, 260, host=True)
    np.testing.assert_array_equal(host["count"], [257, 257])
    np.testing.assert_array_equal(host["count"], dev["count"])
    for i, M in enumerate(dev["count"]):
        for k in OUT:
            np.testing.assert_array_equal(host[k][i, :M], dev[k][i, :M], err_msg=k)


@pytest.mark.parametrize("D", rc.ALL_DOFS)
def test_skip_every_joint_count(env, D):
    """The same joint counts through resample_skip_flush: D >= 9 takes a second round of
    kResampleSkipGroup wave trips, D > 64 walks with 64 / D == 0, D = 1, 8, 16, 64 never or always
    wrap. N = 200, a full 64-entry register batch and a partial one; max_out = N + 1 and 70, a
    cut inside the second batch."""
    case = rc.skip_dof_case(D)
    for max_out in rc.SKIP_MAX_OUTS:
        cap = 201 if max_out is None else max_out
        counts, _ = _check(env, case, cap, skip=True, what="D=%d max_out=%d" % (D, cap))
        assert min(counts) - 1 > 70 and max(counts) - 1 < 128


@pytest.mark.parametrize("name", ["ticks_on_samples", "past_the_end", "tiny_bracket", "status", "two_samples"])
def test_skip_edges(env, name):
    """The skip method's first output on the uniform edge inputs (D = 3): a start on, between,
    before and past the samples (one output: the end sample), the sub-epsilon bracket, a
    skipped path, N = 2."""
    case = EDGES[name]
    N = case["sol"]["q"].shape[1]
    counts, _ = _check(env, case, N + 1, skip=True, what=name)
    if name == "past_the_end":
        assert counts == [1, 1, 1, 1]
    if name == "status":
        assert counts[1] == 0 and counts[0] > 1


# ---------------------------------------------------------------------------- query
@functools.lru_cache(maxsize=None)
def _query_reference(N, B, K):
    """The batch and the restatement's (ok, s, sd, sdd) [B][K]; s, sd, sdd are NaN where ok is 0
    (the reference leaves its outputs alone there, the kernel's are unspecified)."""
    qb = rc.query_batch(N, B, K)
    ref = np.full((4, B, K), np.nan)
    for b in range(B):
        rows = [qb[k][b].tolist() for k in ("time", "s", "sd", "sd2")]
        for j, t in enumerate(qb["tq"][b].tolist()):
            r = rr.query(*rows, t)
            ref[0, b, j] = r[0]
            if r[0]:
                ref[1:, b, j] = r[1:]
    return qb, ref


def _query(env, qb, status=None, with_ok=True, explicit_sd2=True, device_rows=None):
    """tpamd_query_device into sentinel-filled outputs with ok = -5. device_rows: time, s, sd
    tensors already on the device (a solve's outputs) instead of qb's."""
    B, K = qb["tq"].shape
    rows = device_rows or {k: _up(env, qb[k]) for k in ("time", "s", "sd")}
    outs, guards = zip(*[_guarded(env, (B, K), SENTINEL) for _ in range(3)])
    ok, ok_guard = _guarded(env, (B, K), -5, np.int32)
    sd2 = None if not explicit_sd2 else (qb["sd2"] if device_rows else _up(env, qb["sd2"]))
    env["E"].query(rows["time"], rows["s"], rows["sd"], _up(env, status), _up(env, qb["tq"]), *outs,
                   ok if with_ok else None, sd2=sd2)
    env["torch"].cuda.synchronize()
    for g in guards:
        assert bool((g == SENTINEL).all())
    assert bool((ok_guard == -5).all())
    return [o.cpu().numpy() for o in outs], ok.cpu().numpy()


def _assert_query(got, ok, ref, with_ok=True, what=""):
    good = ref[0] == 1
    if with_ok:
        np.testing.assert_array_equal(ok, ref[0].astype(np.int32), err_msg=what + " ok")
    else:
        assert (ok == -5).all()
    for name, g, r in zip(("s", "sd", "sdd"), got, ref[1:]):
        np.testing.assert_array_equal(g[good], r[good], err_msg="%s %s" % (what, name))


@pytest.mark.parametrize("B,K", rc.QUERY_SHAPES)
@pytest.mark.parametrize("N", rc.QUERY_SAMPLES)
def test_query_synthetic_rows(env, N, B, K):
    """N = 2 (the search loop never runs), 3, 65; K = 1, 255, 256, 257 with B K on each side of 256
    and 512. Queries at the first and last time stamps and nextafter around them, on every sample
    time, inside and at the ends of plateaus at both ends, and in the hand-set brackets: the
    ds > ds_ clamp, the saturation to s[k + 1], ok = 0 and the zero-velocity line."""
    qb, ref = _query_reference(N, B, K)
    got, ok = _query(env, qb)
    _assert_query(got, ok, ref, what="N=%d B=%d K=%d" % (N, B, K))
    if N == 65 and B >= 4:
        assert (ref[0] == 0).any()


def test_query_status_row_and_no_ok(env):
    """A row with status != 0 keeps the sentinel and gets ok = 0; ok = None is accepted and the
    values are the same."""
    N, B, K = 65, 8, 257
    qb, ref = _query_reference(N, B, K)
    status = np.array([0, 4, 0, 0, 0, 0, 1, 0], dtype=np.int32)
    got, ok = _query(env, qb, status=status)
    live = status == 0
    for g in got:
        assert (g[~live] == SENTINEL).all()
    assert (ok[~live] == 0).all()
    _assert_query([g[live] for g in got], ok[live], ref[:, live], what="status")
    got, ok = _query(env, qb, with_ok=False)
    _assert_query(got, ok, ref, with_ok=False, what="ok = None")
    got, ok = _query(env, qb, status=status, with_ok=False)
    for g in got:
        assert (g[~live] == SENTINEL).all()
    _assert_query([g[live] for g in got], ok[live], ref[:, live], with_ok=False, what="status, ok = None")


def test_query_solved_profiles(env):
    """Solved profiles with time plateaus at the ends (stop_first, stop_last) and inside: the
    query with the solve's sd2 output and with the engine's own copy of its last solve, against
    tpo.Profile.query and against the restatement on the solve's rows."""
    torch, eng, E, tpo = env["torch"], env["eng"], env["E"], env["tpo"]
    b = rc.solved_batch()
    B, N, D = len(rc.SOLVED_FAMILIES), rc.SOLVED_N, rc.SOLVED_D
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    out["sd2"] = torch.empty(B, N, dtype=torch.float64, device=env["dev"])
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    assert (out["status"].cpu().numpy() == 0).all()
    host = {k: out[k].cpu().numpy() for k in ("time", "s", "sd", "sd2")}
    pools = [rc.query_times(host["time"][i]) for i in range(B)]
    K = min(len(p) for p in pools)
    tq = np.stack([p[:K] for p in pools])
    ref = np.empty((4, B, K))
    plateaus = 0
    for i in range(B):
        p = rc.oracle_profile(tpo, b, i)
        np.testing.assert_array_equal(host["time"][i], p.time)
        rows = [host[k][i].tolist() for k in ("time", "s", "sd", "sd2")]
        for j, t in enumerate(tq[i].tolist()):
            r = rr.query(*rows, t)
            assert r == p.query(t), (i, float(t).hex())
            ref[:, i, j] = r
        plateaus += int((np.diff(host["time"][i]) == 0).any())
    assert plateaus >= 2 and (ref[0] == 1).all()
    qb = dict(tq=tq, sd2=out["sd2"])
    got, ok = _query(env, qb, device_rows=out)
    _assert_query(got, ok, ref, what="solved, sd2 given")
    got, ok = _query(env, qb, device_rows=out, explicit_sd2=False)
    _assert_query(got, ok, ref, what="solved, the engine's sd2")

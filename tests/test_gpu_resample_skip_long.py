"""The skip-method resampler (k_resample_skip, tpamd_resample_skip_*) at the edges of its 64-sample
chunks and its 64-entry register batches, and on histories longer than 32768 samples, against the
oracle's tpo.resample_skip path by path. Every comparison is bit for bit: the kernel copies samples
and repeats the reference's recurrence, so there is no tolerance.

The trajectories are random numbers on a time axis built per case: the resampler reads nothing but
the time stamps to decide, copies the rest, and interpolates its first output."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

SENTINEL = -7777.25
OUT = ("out_time", "out_s", "out_sd", "out_sdd", "out_q", "out_qd", "out_qdd")
SOL = ("time", "s", "sd", "sdd", "q", "qd", "qdd")


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


def _trajectory(rng, time, D):
    """A solution dict around the time stamps time [B][N], and limits small enough that the
    first output's acceleration clamp acts on some joints."""
    B, N = time.shape
    sol = dict(time=np.ascontiguousarray(time, dtype=np.float64))
    for k in ("s", "sd", "sdd"):
        sol[k] = rng.uniform(-1.0, 1.0, (B, N))
    for k in ("q", "qd", "qdd"):
        sol[k] = rng.uniform(-1.0, 1.0, (B, N, D))
    return sol, rng.uniform(0.2, 1.5, (B, D))


def _resample(env, sol, amax, start, dt, max_out, status=None, host=False):
    """tpamd_resample_skip_device (through Engine.resample_uniform) or _host into sentinel-filled
    outputs; returns them as numpy arrays."""
    torch, eng, E = env["torch"], env["eng"], env["E"]
    B, N, D = sol["q"].shape
    out = {k: np.full((B, max_out) + ((D,) if k in OUT[4:] else ()), SENTINEL) for k in OUT}
    out["count"] = np.full(B, -5, dtype=np.int32)
    start = np.array(np.broadcast_to(start, (B,)), dtype=np.float64)
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32)
    if host:
        args = eng._ResampleArgs(B, N, D, max_out, *[eng._ptr(sol[k]) for k in SOL], eng._ptr(amax),
                                 eng._ptr(start), float(dt), eng._ptr(st),
                                 *[eng._ptr(out[k]) for k in OUT + ("count",)])
        rc = E._lib.tpamd_resample_skip_host(E._h, C.byref(args))
        assert rc == 0, E._lib.tpamd_error_string(rc)
        return out
    up = lambda a: None if a is None else torch.from_numpy(a).to(env["dev"])
    dsol = {k: up(sol[k]) for k in SOL}
    dsol["status"] = up(st)
    dout = {k: up(v) for k, v in out.items()}
    E.resample_uniform(dsol, up(amax), up(start), dt, dout, skip=True)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dout.items()}


def _oracle(env, sol, amax, i, start, dt):
    return env["tpo"].resample_skip(*[sol[k][i] for k in SOL], float(start), dt, amax[i])


def _kept_indices(time, ref):
    """Indices of the kept samples (outputs 1..) of a path whose time stamps are distinct."""
    return np.searchsorted(time, ref[0][1:])


def _check(env, sol, amax, start, dt, max_out=None, what=""):
    """One device call for the batch; every path against the oracle. Returns the oracle's outputs."""
    B, N, D = sol["q"].shape
    start = np.broadcast_to(np.asarray(start, dtype=np.float64), (B,))
    cap = N + 1 if max_out is None else max_out
    got = _resample(env, sol, amax, start, dt, cap)
    refs = []
    for i in range(B):
        ref = _oracle(env, sol, amax, i, start[i], dt)
        M = len(ref[0])
        assert got["count"][i] == M, (what, i, got["count"][i], M)
        w = min(M, cap)      # with cap < M the oracle's special last sample is not among the first cap
        for k, r in zip(OUT, ref):
            np.testing.assert_array_equal(got[k][i, :w], r[:w], err_msg="%s path %d %s" % (what, i, k))
            assert (got[k][i, w:] == SENTINEL).all(), (what, i, k, "written past the count or max_out")
        refs.append(ref)
    return refs


@pytest.mark.parametrize("N", [2, 3, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193])
def test_chunk_edges(env, N):
    """Lengths on each side of one, two and three 64-sample chunks; a start before the first sample,
    inside, after the last (lower = N - 1, one output) and on a sample time at indices 62 .. 65, so
    that the lower index lands on each side of a chunk boundary. With the tiny time step nothing
    is skipped: N = 65, 66, 129, 130 kept samples are a full register batch and one more."""
    B, D = 12, 2
    rng = np.random.default_rng(9000 + N)
    time = 3.0 + np.cumsum(rng.uniform(0.001, 0.01, (B, N)), axis=1)
    sol, amax = _trajectory(rng, time, D)
    at = lambda b, i: time[b, min(i, N - 1)]
    span = time[:, -1] - time[:, 0]
    start = np.array([time[0, 0] - 0.5, time[1, 0] + 0.37 * span[1], time[2, -1] + 0.25, at(3, 62), at(4, 63),
                      at(5, 64), at(6, 65), at(7, 0), at(8, 1), time[9, -1], time[10, 0] + 0.9 * span[10],
                      at(11, N - 2)])
    refs = _check(env, sol, amax, start, 0.004, what="N=%d" % N)
    assert len(refs[2][0]) == 1 and len(refs[9][0]) == 1       # at or after the last sample: M = 1
    refs = _check(env, sol, amax, start, 1e-6, what="N=%d, nothing skipped" % N)
    assert len(refs[0][0]) == N and len(refs[7][0]) == N       # from before / at the first sample: every later one


def _clusters(N, jumps, fine=1e-5, jump=1.0):
    """Time stamps that advance by `fine`, and by `jump` before the listed indices."""
    gaps = np.full(N, fine)
    gaps[list(jumps)] = jump
    return np.cumsum(gaps)


def test_keep_patterns(env):
    N, D = 300, 3
    rng = np.random.default_rng(300)
    irregular = np.cumsum(rng.uniform(0.001, 0.01, N))
    duration = irregular[-1] - irregular[0]
    two_starts = lambda t: np.array([t[0] - 0.01, t[0] + 0.41 * (t[-1] - t[0])])

    def run(time, dt, start=None, what=""):
        t2 = np.stack([time, time])
        sol, amax = _trajectory(rng, t2, D)
        return _check(env, sol, amax, two_starts(time) if start is None else start, dt, what=what), time

    # nothing skipped: 299 kept from before the first sample, four full register batches and a tail
    refs, _ = run(irregular, 1e-6, what="nothing skipped")
    assert len(refs[0][0]) == N
    # everything skipped: the time step is longer than the trajectory, one output
    refs, _ = run(irregular, 10.0 * duration, what="everything skipped")
    assert len(refs[0][0]) == 1 and len(refs[1][0]) == 1
    # exactly one kept
    even = 0.001 * np.arange(N)
    refs, _ = run(even, 0.2 / 0.95, start=np.array([0.0, 0.05]), what="one kept")
    assert len(refs[0][0]) == 2 and len(refs[1][0]) == 2
    # runs of more than 64 and more than 128 skipped samples: chunks without a kept sample
    refs, t = run(_clusters(N, [5, 80, 220, 290]), 0.5, start=np.array([-1.0, 0.0]), what="long runs")
    run_lengths = np.diff(_kept_indices(t, refs[0]))
    assert (run_lengths > 64).sum() >= 2 and (run_lengths > 128).sum() >= 1
    # kept samples on lanes 0 and 63 of a chunk: from before the first sample the scan starts at
    # index 1, so index i is lane (i - 1) % 64
    refs, t = run(_clusters(N, [1, 64, 65, 128, 129, 192]), 0.01, start=np.array([-1.0, -2.0]), what="lanes 0 and 63")
    assert _kept_indices(t, refs[0]).tolist() == [1, 64, 65, 128, 129, 192]
    # duplicate time stamps
    refs, _ = run(np.cumsum(rng.choice([0.0, 0.0, 0.004, 0.002], N)), 0.004, what="duplicates")
    assert 20 < len(refs[0][0]) < N
    # gaps of k * (0.95 * time_step), summed in double: many comparisons within an ulp of the threshold
    dt = 0.004
    ulp = np.cumsum(rng.integers(1, 4, N) * (0.95 * dt))
    refs, t = run(ulp, dt, start=np.array([ulp[0], ulp[7]]), what="threshold ties")
    near = np.abs(np.diff(t) - 0.95 * dt) <= 4 * np.spacing(t[1:])
    assert near.sum() > 50 and 64 < len(refs[1][0]) < N
    # more than 64 and more than 128 kept: one and two full register batches with a partial tail
    for lo, hi, want in ((0.0009, 0.0016, (65, 128)), (0.0017, 0.0027, (129, 192))):
        tt = np.cumsum(rng.uniform(lo, hi, N))
        refs, _ = run(tt, 0.004, start=np.array([tt[0] - 1.0, tt[0] - 2.0]), what="kept in %s" % (want,))
        assert want[0] <= len(refs[0][0]) - 1 <= want[1], len(refs[0][0])


def test_max_out(env):
    """count reports the full number whatever max_out is; only slots below max_out are written."""
    N, D = 300, 3
    rng = np.random.default_rng(301)
    time = np.cumsum(rng.uniform(0.0017, 0.0027, (2, N)), axis=1)
    sol, amax = _trajectory(rng, time, D)
    start = np.array([time[0, 0] - 1.0, time[1, 40]])
    M = len(_oracle(env, sol, amax, 0, start[0], 0.004)[0])
    assert 130 <= M <= 193
    for max_out in (M, M - 1, 1, 65):
        _check(env, sol, amax, start, 0.004, max_out=max_out, what="max_out=%d" % max_out)


def test_status_skips_a_path(env):
    N, D = 150, 2
    rng = np.random.default_rng(302)
    time = np.cumsum(rng.uniform(0.001, 0.01, (3, N)), axis=1)
    sol, amax = _trajectory(rng, time, D)
    start = time[:, 3].copy()
    got = _resample(env, sol, amax, start, 0.004, N + 1, status=[0, 4, 0])
    assert got["count"][1] == 0
    for k in OUT:
        assert (got[k][1] == SENTINEL).all(), k
    for i in (0, 2):
        ref = _oracle(env, sol, amax, i, start[i], 0.004)
        M = len(ref[0])
        assert got["count"][i] == M
        for k, r in zip(OUT, ref):
            np.testing.assert_array_equal(got[k][i, :M], r)
            assert (got[k][i, M:] == SENTINEL).all()


def _long_case(N, seed):
    rng = np.random.default_rng(seed)
    time = 100.0 + np.cumsum(rng.uniform(0.002, 0.004, (3, N)), axis=1)
    sol, amax = _trajectory(rng, time, 2)
    start = np.array([time[0, 0] - 0.1, time[1, 1000] + 1e-4, time[2, N // 2]])
    return sol, amax, start


@pytest.mark.parametrize("N", [32768, 32769, 40000, 70001])
def test_long_histories(env, N):
    """About every second sample kept, and about one in a hundred (long skipped runs at large
    indices). Above 32768 samples the former kernel's LDS index list did not fit."""
    sol, amax, start = _long_case(N, N)
    refs = _check(env, sol, amax, start, 0.004, what="N=%d half" % N)
    assert 0.4 * N < len(refs[0][0]) < 0.6 * N
    refs = _check(env, sol, amax, start, 0.3, what="N=%d hundredth" % N)
    assert 0.005 * N < len(refs[0][0]) < 0.02 * N


def test_host_entry_long(env):
    """tpamd_resample_skip_host at 40000 samples gives what the device entry gives."""
    sol, amax, start = _long_case(40000, 41)
    dev = _resample(env, sol, amax, start, 0.004, 40001)
    host = _resample(env, sol, amax, start, 0.004, 40001, host=True)
    assert host["count"].min() > 10000
    np.testing.assert_array_equal(host["count"], dev["count"])
    for i, M in enumerate(dev["count"]):       # the host entry copies its whole output arrays back: only the
        for k in OUT:                          # slots below the count say anything
            np.testing.assert_array_equal(host[k][i, :M], dev[k][i, :M], err_msg=k)

"""Waypoint batches on the GPU (tpamd_fit_joint_waypoints_*, tpamd_time_waypoint_paths_*): one call
fits and times twelve paths with 0 .. 11 waypoints and 3 .. 300 samples (tests/waypoint_batch_cases.py).
Every output of every path is held bit-equal to the oracle -- tpo.joint_fit_spline, then
tpo.time_joint_batch on that one spline, delta = path_end / (n - 1) in numpy -- and to the existing
way (host fit, one tpamd_time_joint_paths_host call per path); the path without waypoints gets
TPAMD_PATH_NO_WAYPOINTS and keeps the sentinel in every row; the other paths are bit-equal to a call
without it; the _host and _device entries agree bit for bit; call-level errors write nothing."""
import ctypes as C
import importlib

import numpy as np
import pytest

import waypoint_batch_cases as wc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

N = wc.NUM_SAMPLES
ROWS = ("time", "s", "sd", "sdd", "q", "qd", "qdd")
PER_PATH = ("status", "last_extremal_index", "max_time_increment", "num_points", "path_end", "delta_used")
TPAMD_PLAN_INVALID_ARGUMENT = 3
E_INVALID, E_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(torch=torch, eng=eng, tpo=tpo, E=eng.Engine(0), dev=torch.device("cuda", 0), lib=eng.load_library())


def _slot(batch):
    return max(4, max(wc.fit_points(len(p)) for p in batch["paths"]))


def _sentinel_outputs(batch):
    B, D, S = batch["B"], batch["D"], _slot(batch)
    out = {k: np.full((B, N), wc.SENTINEL) for k in ("time", "s", "sd", "sdd")}
    out.update({k: np.full((B, N, D), wc.SENTINEL) for k in ("q", "qd", "qdd")})
    out.update({k: np.full(B, -7, dtype=np.int32) for k in ("status", "last_extremal_index", "num_points")})
    out.update({k: np.full(B, wc.SENTINEL) for k in ("max_time_increment", "path_end", "delta_used")})
    out["knots"] = np.full((B, S + 3), wc.SENTINEL)
    out["control_points"] = np.full((B, S, D), wc.SENTINEL)
    return out


def _time(env, batch, kw, host):
    """One call through Engine.time_waypoint_paths into sentinel-filled outputs; numpy arrays back."""
    torch, dev = env["torch"], env["dev"]
    out = _sentinel_outputs(batch)
    args = dict(num_samples_per_path=kw["ns"], delta=kw["delta"], rounding=batch["rounding"],
                time_start=kw["time_start"])
    if host:
        return env["E"].time_waypoint_paths(batch["waypoints"], batch["offsets"], batch["vmax"], batch["amax"], N,
                                            outputs=out, host=True, **args)
    up = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    got = env["E"].time_waypoint_paths(up(batch["waypoints"]), batch["offsets"], up(batch["vmax"]), up(batch["amax"]),
                                       N, outputs={k: up(v) for k, v in out.items()},
                                       **{k: up(v) for k, v in args.items()})
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def _same(a, b, what):
    assert a.tobytes() == b.tobytes(), what


def _check(got, batch, exp):
    solved = 0
    for k, e in enumerate(exp):
        if e is None:
            assert got["status"][k] == wc.NO_WAYPOINTS
            assert got["num_points"][k] == 0 and got["path_end"][k] == 0.0
            for r in ROWS:
                assert (got[r][k] == wc.SENTINEL).all(), (r, k)
            assert got["last_extremal_index"][k] == -7 and got["max_time_increment"][k] == wc.SENTINEL
            continue
        P, n, ref = e["P"], e["n"], e["ref"]
        assert got["num_points"][k] == P
        _same(got["path_end"][k:k + 1], np.array([e["path_end"]]), ("path_end", k))
        _same(got["delta_used"][k:k + 1], np.array([e["delta"]]), ("delta_used", k))
        _same(got["knots"][k, :P + 3], e["knots"], ("knots", k))
        _same(got["control_points"][k, :P], e["cps"], ("control_points", k))
        assert got["status"][k] == ref["status"][0], (k, got["status"][k], ref["status"][0])
        assert got["last_extremal_index"][k] == ref["last_extremal_index"][0], k
        if ref["status"][0] == 0:
            solved += 1
            for r in ROWS:
                _same(got[r][k, :n], ref["t" if r == "time" else r][0], (r, k, n))
                assert (got[r][k, n:] == wc.SENTINEL).all(), ("wrote past the path's sample count", r, k)
    assert solved >= 8          # the batch is about solved paths


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("D", wc.TIMING_DOFS)
def test_whole_path_delta_host_and_device(env, D, reverse):
    batch, exp, kw = wc.cached_case(D, reverse, "whole")
    dev = _time(env, batch, kw, host=False)
    _check(dev, batch, exp)
    host = _time(env, batch, kw, host=True)
    _check(host, batch, exp)
    for k in ROWS + PER_PATH:
        _same(dev[k], host[k], k)


@pytest.mark.parametrize("D", wc.TIMING_DOFS)
def test_given_deltas_short_and_past_the_end(env, D):
    batch, exp, kw = wc.cached_case(D, False, "given")
    _check(_time(env, batch, kw, host=False), batch, exp)
    _check(_time(env, batch, kw, host=True), batch, exp)


@pytest.mark.parametrize("D", wc.TIMING_DOFS)
def test_uniform_counts_and_batch_without_the_empty_paths(env, D):
    """No per-path counts: with the empty paths (which makes the launch ragged inside) and without them
    (the uniform launch); then the ragged batch without its empty paths against the batch with them."""
    batch, exp, kw = wc.cached_case(D, False, "uniform")
    _check(_time(env, batch, kw, host=False), batch, exp)
    small, keep = wc.without_empty(batch)
    _check(_time(env, small, kw, host=False), small, [exp[k] for k in keep])
    _check(_time(env, small, kw, host=True), small, [exp[k] for k in keep])
    batch, exp, kw = wc.cached_case(D, False, "whole")
    full = _time(env, batch, kw, host=False)
    small, keep = wc.without_empty(batch)
    part = _time(env, small, dict(kw, ns=small["ns"]), host=False)
    for k in ROWS + PER_PATH:
        _same(full[k][keep], part[k], k)
    for i, k in enumerate(keep):
        P = exp[k]["P"]
        _same(full["knots"][k, :P + 3], part["knots"][i, :P + 3], "knots")
        _same(full["control_points"][k, :P], part["control_points"][i, :P], "control_points")


@pytest.mark.parametrize("D", wc.TIMING_DOFS)
def test_existing_way_host_fit_then_one_call_per_path(env, D):
    """The entry this one feeds: every path fitted on the host, then tpamd_time_joint_paths_host."""
    batch, exp, kw = wc.cached_case(D, False, "whole")
    got = _time(env, batch, kw, host=False)
    for k, e in enumerate(exp):
        if e is None:
            continue
        n = e["n"]
        inp = dict(knots=e["knots"][None].copy(), control_points=e["cps"][None].copy(),
                   max_velocity=batch["vmax"][k:k + 1].copy(), max_acceleration=batch["amax"][k:k + 1].copy(),
                   path_start=np.zeros(1), delta=np.array([e["delta"]]), sd_start=np.zeros(1), time_start=np.zeros(1))
        out = {r: np.zeros((1, n)) for r in ("time", "s", "sd", "sdd")}
        out.update({r: np.zeros((1, n, D)) for r in ("q", "qd", "qdd")})
        out.update(status=np.full(1, -1, dtype=np.int32), last_extremal_index=np.zeros(1, dtype=np.int32))
        env["E"].time_joint_paths(inp, out, n, host=True)
        assert out["status"][0] == got["status"][k]
        assert out["last_extremal_index"][0] == got["last_extremal_index"][k]
        for r in ROWS:
            _same(out[r][0], got[r][k, :n], (r, k))


@pytest.mark.parametrize("D", range(1, 17))
def test_fit_entry_packed_at_every_joint_count(env, D):
    torch, dev, tpo = env["torch"], env["dev"], env["tpo"]
    for reverse in (False, True):
        batch = wc.make_batch(D, reverse)
        fits = wc.oracle_fits(tpo, batch)
        npts = np.array([wc.fit_points(len(p)) for p in batch["paths"]], dtype=np.int32)
        host = env["E"].fit_joint_waypoints(batch["waypoints"], batch["offsets"], batch["rounding"])
        d = env["E"].fit_joint_waypoints(torch.from_numpy(batch["waypoints"]).to(dev), batch["offsets"],
                                         torch.from_numpy(batch["rounding"]).to(dev))
        torch.cuda.synchronize()
        d = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in d.items()}
        for got in (host, d):
            np.testing.assert_array_equal(got["num_points"], npts)
            np.testing.assert_array_equal(got["point_offsets"], np.concatenate([[0], np.cumsum(npts)]))
            np.testing.assert_array_equal(got["status"], np.where(npts == 0, TPAMD_PLAN_INVALID_ARGUMENT, 0))
            assert got["knots"].shape == (int((npts + 3 * (npts > 0)).sum()),)
            assert got["control_points"].shape == (int(npts.sum()), D)
            ko = 0
            for k, f in enumerate(fits):
                if f is None:
                    assert got["path_end"][k] == 0.0
                    continue
                P, p0 = int(npts[k]), int(got["point_offsets"][k])
                _same(got["control_points"][p0:p0 + P], f[0], ("control points", D, k))
                _same(got["knots"][ko:ko + P + 3], f[1], ("knots", D, k))
                _same(got["path_end"][k:k + 1], f[1][-1:], ("path_end", D, k))
                ko += P + 3
        # rounding NULL is 0.2
        dflt = env["E"].fit_joint_waypoints(batch["waypoints"], batch["offsets"])
        same = env["E"].fit_joint_waypoints(batch["waypoints"], batch["offsets"], 0.2)
        for k in ("knots", "control_points", "path_end"):
            _same(dflt[k], same[k], k)


def test_call_level_errors_write_nothing(env):
    eng, lib, E = env["eng"], env["lib"], env["E"]
    batch = wc.make_batch(7)
    B, D = batch["B"], 7
    zeros = np.zeros(B)

    def call(num_dofs=D, num_samples=N, offsets=batch["offsets"], waypoints=batch["waypoints"], ns=None,
             engine=E._h, drop=None, vmax=batch["vmax"]):
        out = _sentinel_outputs(batch)
        before = {k: v.copy() for k, v in out.items()}
        p = lambda a: None if a is None else a.ctypes.data
        bt = eng._WaypointBatch(B, num_dofs, num_samples, 0, 0.8)
        wi = eng._WaypointInputs(p(offsets), p(waypoints), p(batch["rounding"]), p(vmax), p(batch["amax"]), p(ns),
                                 None, p(zeros), p(zeros))
        po = eng._PathOutputs(*[None if k == drop else p(out.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index", "max_time_increment", "status", "sd2")])
        fo = eng._WaypointFitOutputs(*[p(out[k]) for k in ("num_points", "path_end", "delta_used", "knots",
                                                           "control_points")])
        rc = lib.tpamd_time_waypoint_paths_host(engine, C.byref(bt), C.byref(wi), C.byref(po), C.byref(fo))
        for k in out:
            _same(out[k], before[k], k)
        return rc

    assert call(engine=None) == E_INVALID
    assert call(vmax=None) == E_INVALID
    assert call(waypoints=None) == E_INVALID
    assert call(offsets=None) == E_INVALID
    assert call(drop="status") == E_INVALID
    assert call(drop="time") == E_INVALID
    bad = batch["offsets"].copy(); bad[0] = 1
    assert call(offsets=bad) == E_INVALID
    bad = batch["offsets"].copy(); bad[3] = bad[2] - 1
    assert call(offsets=bad) == E_INVALID
    for dofs in (0, 17):
        assert call(num_dofs=dofs) == E_UNSUPPORTED
    for n in (2, 8193):
        assert call(num_samples=n) == E_UNSUPPORTED
    ns = batch["ns"].copy(); ns[4] = N + 1
    assert call(ns=ns) == E_INVALID
    assert lib.tpamd_time_waypoint_paths_host(E._h, None, None, None, None) == E_INVALID
    # the largest P's knots and control points must fit the sampling/LP kernel's LDS: at 16 joints and
    # the 64-thread blocks of a ragged batch, (17 P + 3 + 64 + 2048) * 8 <= 160 KB stops at P = 1080
    assert E_UNSUPPORTED == _lds_call(env, 361)       # P = 1081
    assert 0 == _lds_call(env, 360)                   # P = 1078
    # the fit entry: as the pose fit
    k, c = np.zeros(64), np.zeros((64, D))
    npts, pe, st = np.full(B, -7, dtype=np.int32), np.zeros(B), np.full(B, -7, dtype=np.int32)
    fit = lambda **a: lib.tpamd_fit_joint_waypoints_host(
        a.get("e", E._h), B, a.get("D", D), a.get("off", batch["offsets"]).ctypes.data, batch["waypoints"].ctypes.data,
        None, k.ctypes.data, c.ctypes.data, npts.ctypes.data, None, pe.ctypes.data,
        None if a.get("no_status") else st.ctypes.data)
    bad = batch["offsets"].copy(); bad[0] = 1
    assert fit(e=None) == E_INVALID and fit(D=0) == E_INVALID and fit(D=17) == E_INVALID
    assert fit(off=bad) == E_INVALID and fit(no_status=True) == E_INVALID
    assert (npts == -7).all() and (st == -7).all() and not k.any() and not c.any()


def _lds_call(env, W):
    """One 16-joint path of W waypoints, per-path counts given (64-thread blocks)."""
    eng, lib, E = env["eng"], env["lib"], env["E"]
    D, n = 16, 16
    rng = np.random.default_rng(W)
    wps = rng.uniform(-1, 1, size=(W, D))
    off = np.array([0, W], dtype=np.int32)
    lim = np.ones((1, D))
    ns = np.array([n], dtype=np.int32)
    out = {k: np.full((1, n), wc.SENTINEL) for k in ("time", "s", "sd", "sdd")}
    st = np.full(1, -7, dtype=np.int32)
    p = lambda a: a.ctypes.data
    bt = eng._WaypointBatch(1, D, n, 0, 0.8)
    wi = eng._WaypointInputs(p(off), p(wps), None, p(lim), p(lim), p(ns), None, None, None)
    po = eng._PathOutputs(p(out["time"]), p(out["s"]), p(out["sd"]), p(out["sdd"]), None, None, None, None, None, p(st),
                          None)
    rc = lib.tpamd_time_waypoint_paths_host(E._h, C.byref(bt), C.byref(wi), C.byref(po), None)
    if rc != 0:
        assert st[0] == -7 and all((v == wc.SENTINEL).all() for v in out.values())
    else:
        assert st[0] != -7
    return rc

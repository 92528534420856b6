"""The solution check for joint and waypoint batches on the GPU (tpamd_check_joint_paths_*,
Engine.check_joint_paths / check_waypoint_paths).

The engine solves the synthetic batches of tests/check_reference.py (asking for sd2), then checks its
own solution. Every comparison is bit equality (NaN by position) on sentinel-filled outputs:
  * the five outputs against tests/check_reference.py on the ORACLE's rows (tpo.joint_sample_path +
    tpo.joint_constraint_setup) with the engine's sd2 / sdd;
  * violations against the oracle's constraint_violations() of its own solve;
  * the same with sd2 * 1.01, which violates rows on every shape, so that a kernel that returns
    zeros fails everywhere;
  * a ragged batch (counts 3, 64, 65, 200, 257), a failed path, a start parameter inside the path
    with samples behind its end, the _host entry, and a waypoint batch against the uniform check
    of each path alone."""
import importlib

import numpy as np
import pytest

import check_reference as cr
import waypoint_batch_cases as wc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

PRE, PRE_INT = -7.25, -9


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
    return dict(knots=batch["knots"], control_points=batch["control_points"], max_velocity=batch["vmax"],
                max_acceleration=batch["amax"], path_start=batch["path_start"], delta=batch["delta"],
                sd_start=batch["sd_start"], time_start=batch["time_start"],
                num_samples_per_path=batch.get("num_samples_per_path"))


def solve(env, batch, N):
    """Engine.time_joint_paths on the device; time, s, sd, sdd, sd2, status as numpy arrays."""
    torch = env["torch"]
    B = batch["control_points"].shape[0]
    inp = {k: _up(env, v) for k, v in _inputs(batch).items()}
    out = {k: torch.full((B, N), PRE, dtype=torch.float64, device=env["dev"]) for k in ("time", "s", "sd", "sdd", "sd2")}
    out["status"] = torch.full((B,), PRE_INT, dtype=torch.int32, device=env["dev"])
    env["E"].time_joint_paths(inp, out, N, safety=batch["safety"])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(env, batch, N, sol, host=False, with_status=True, **kw):
    """Engine.check_joint_paths on sentinel-filled outputs; numpy arrays back."""
    B = batch["control_points"].shape[0]
    conv = (lambda a: None if a is None else np.ascontiguousarray(a)) if host else (lambda a: _up(env, a))
    solution = {k: conv(sol[k]) for k in ("sd2", "sdd") if k in sol}
    if "sd" in sol and "sd2" not in sol:
        solution["sd"] = conv(sol["sd"])
    if with_status:
        solution["status"] = conv(sol["status"])
    got = env["E"].check_joint_paths({k: conv(v) for k, v in _inputs(batch).items()}, solution, N,
                                     safety=batch["safety"], outputs={k: conv(v) for k, v in _sentinels(B).items()},
                                     host=host, **{k: conv(v) for k, v in kw.items()})
    if host:
        return got
    env["torch"].cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in got.items()}


def expected(env, batch, N, sol, with_status=True):
    """Per path the helper's record on the oracle's rows with the given sd2 / sdd."""
    B = batch["control_points"].shape[0]
    ns = batch.get("num_samples_per_path")
    recs = []
    for b in range(B):
        n = N if ns is None else int(ns[b])
        if (with_status and sol["status"][b] != 0) or n < 2 or n > N:
            recs.append(cr.NOT_CHECKED)
            continue
        rows = cr.joint_rows(env["tpo"], batch, b, n)
        recs.append(cr.check_rows(*rows, sol["sd2"][b, :n], sol["sdd"][b, :n]))
    return recs


def assert_records(got, want, what):
    for b, w in enumerate(want):
        assert cr.same_record(cr.record_of(got, b), w), (what, b, cr.record_of(got, b), w)


@pytest.mark.parametrize("shape", cr.JOINT_SHAPES)
def test_engine_solution_against_oracle_rows(env, shape):
    D, N, W = shape
    batch = env["syn"].make_joint_batch(16, D, N, W)
    sol = solve(env, batch, N)
    assert (sol["status"] == 0).all()
    want = expected(env, batch, N, sol)
    got = check(env, batch, N, sol)
    assert_records(got, want, "device")
    # the oracle's count on its own solve of the same path
    for b, (rc, viol, _, _) in enumerate(cr.oracle_counts(env["tpo"], batch)):
        assert rc == 0 and got["violations"][b] == viol, (b, got["violations"][b], viol)
    assert_records(check(env, batch, N, sol, host=True), want, "host")
    # a solution that is 1 % too fast violates rows on every shape
    fast = dict(sol, sd2=sol["sd2"] * 1.01)
    want = expected(env, batch, N, fast)
    assert any(w[0] > 0 for w in want), "the expectation must hold violated rows"
    assert_records(check(env, batch, N, fast), want, "1.01 device")
    assert_records(check(env, batch, N, fast, host=True), want, "1.01 host")


def test_ragged_batch_failed_path_and_sd_in_place_of_sd2(env):
    counts = np.array([3, 64, 65, 200, 257], np.int32)
    N = 257
    batch = env["syn"].make_joint_batch(5, 7, N, 4)
    batch["delta"] = np.ascontiguousarray(batch["knots"][:, -1] / (counts - 1))
    batch["num_samples_per_path"] = counts
    batch["sd_start"] = np.array([0.0, 0.0, -1.0, 0.0, 0.0])           # path 2 fails: negative start velocity
    sol = solve(env, batch, N)
    assert sol["status"][2] == 4 and (np.delete(sol["status"], 2) == 0).all()
    want = expected(env, batch, N, sol)
    assert want[2] is cr.NOT_CHECKED
    for host in (False, True):
        assert_records(check(env, batch, N, sol, host=host), want, ("ragged", host))
    fast = dict(sol, sd2=sol["sd2"] * 1.01)
    want = expected(env, batch, N, fast)
    assert sum(w[0] > 0 for w in want) >= 2
    assert_records(check(env, batch, N, fast), want, "ragged 1.01")
    # counts the solve refuses: below 2 and above the stride
    odd = dict(batch, num_samples_per_path=np.array([1, 64, 65, 258, 2], np.int32))
    ok = dict(fast, status=np.zeros(5, np.int32))
    want = expected(env, odd, N, ok)
    assert want[0] is cr.NOT_CHECKED and want[3] is cr.NOT_CHECKED and want[4][0] >= 0
    assert_records(check(env, odd, N, ok), want, "refused counts")
    # sd in place of sd2: the square of the square root
    sd = np.sqrt(np.where(fast["sd2"] >= 0, fast["sd2"], 0.0))
    want = expected(env, batch, N, dict(fast, sd2=sd * sd))
    assert_records(check(env, batch, N, dict(sdd=fast["sdd"], sd=sd, status=fast["status"])), want, "sd")


def test_start_inside_the_path_and_samples_behind_its_end(env):
    N = 129
    batch = env["syn"].make_joint_batch(6, 6, N, 5)
    end = batch["knots"][:, -1]
    batch["path_start"] = np.ascontiguousarray(0.35 * end)              # the last third of the samples lies behind the end
    sol = solve(env, batch, N)
    # whatever the solver makes of such a path, every path is checked when no status is given
    blank = {k: np.where(np.isfinite(sol[k]) & (sol[k] != PRE), sol[k], 0.25) for k in ("sd2", "sdd")}
    blank["sd2"] = blank["sd2"] * 1.01
    blank["status"] = np.zeros(6, np.int32)
    want = expected(env, batch, N, blank)
    rows = cr.joint_rows(env["tpo"], batch, 0, N)
    assert (rows[0][-20:] == 0).all() and (rows[1][-20:] == 0).all()     # the padding: zero derivatives
    assert any(w[0] > 0 for w in want)
    assert_records(check(env, batch, N, blank, with_status=False), want, "device")
    assert_records(check(env, batch, N, blank, host=True), want, "host")
    want = expected(env, batch, N, sol)
    assert_records(check(env, batch, N, sol), want, "the engine's own solution")


def test_waypoint_batch_against_each_path_alone(env):
    torch, E = env["torch"], env["E"]
    D, N = 7, wc.NUM_SAMPLES
    wb = wc.make_batch(D)
    B = wb["B"]
    S = max(4, max(wc.fit_points(len(p)) for p in wb["paths"]))
    out = {k: np.full((B, N), PRE) for k in ("time", "s", "sd", "sdd", "sd2")}
    out["knots"] = np.full((B, S + 3), PRE)
    out["control_points"] = np.full((B, S, D), PRE)
    got = E.time_waypoint_paths(_up(env, wb["waypoints"]), wb["offsets"], _up(env, wb["vmax"]), _up(env, wb["amax"]), N,
                                num_samples_per_path=_up(env, wb["ns"]), rounding=_up(env, wb["rounding"]),
                                outputs={k: _up(env, v) for k, v in out.items()})
    fast = dict(got, sd2=got["sd2"] * 1.01)
    for name, sol in (("own", got), ("1.01", fast)):
        rec = E.check_waypoint_paths(sol, _up(env, wb["vmax"]), _up(env, wb["amax"]), N,
                                     num_samples_per_path=_up(env, wb["ns"]),
                                     outputs={k: _up(env, v) for k, v in _sentinels(B).items()})
        torch.cuda.synchronize()
        rec = {k: v.cpu().numpy() for k, v in rec.items()}
        h = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in sol.items()}
        checked = 0
        for k in range(B):
            P, n = int(h["num_points"][k]), int(wb["ns"][k])
            if P == 0:
                assert h["status"][k] == wc.NO_WAYPOINTS
                assert cr.same_record(cr.record_of(rec, k), cr.NOT_CHECKED), k
                continue
            if h["status"][k] != 0:
                assert cr.same_record(cr.record_of(rec, k), cr.NOT_CHECKED), k
                continue
            checked += 1
            one = dict(knots=h["knots"][k:k + 1, :P + 3], control_points=h["control_points"][k:k + 1, :P],
                       vmax=wb["vmax"][k:k + 1], amax=wb["amax"][k:k + 1], path_start=np.zeros(1),
                       delta=h["delta_used"][k:k + 1], sd_start=np.zeros(1), time_start=np.zeros(1), safety=0.8)
            s1 = dict(sd2=h["sd2"][k:k + 1, :n], sdd=h["sdd"][k:k + 1, :n], status=h["status"][k:k + 1])
            alone = check(env, one, n, s1)
            assert cr.same_record(cr.record_of(rec, k), cr.record_of(alone, 0)), (name, k)
            want = cr.check_rows(*cr.joint_rows(env["tpo"], one, 0, n), s1["sd2"][0], s1["sdd"][0])
            assert cr.same_record(cr.record_of(rec, k), want), (name, k, cr.record_of(rec, k), want)
        assert checked >= 8
        if name == "1.01":
            assert (rec["violations"] > 0).any()


def test_call_level_errors_write_nothing(env):
    eng = env["eng"]
    batch = env["syn"].make_joint_batch(4, 3, 64, 3)
    sol = solve(env, batch, 64)
    out = {k: _up(env, v) for k, v in _sentinels(4).items()}
    inp = {k: _up(env, v) for k, v in _inputs(batch).items()}
    good = {k: _up(env, sol[k]) for k in ("sd2", "sdd", "status")}
    with pytest.raises(eng.TpamdError, match="-3"):                      # 2 samples: outside 3..8192
        env["E"].check_joint_paths(inp, good, 2, outputs=out)
    with pytest.raises(eng.TpamdError, match="-1"):
        env["E"].check_joint_paths(dict(inp, delta=None), good, 64, outputs=out)
    with pytest.raises(eng.TpamdError, match="-1"):
        env["E"].check_joint_paths(inp, dict(good, sdd=None), 64, outputs=out)
    with pytest.raises(eng.TpamdError, match="-1"):
        env["E"].check_joint_paths(inp, dict(sdd=good["sdd"]), 64, outputs=out)
    wide = env["syn"].make_joint_batch(2, 17, 64, 3)                     # 17 joints
    with pytest.raises(eng.TpamdError, match="-3"):
        env["E"].check_joint_paths({k: _up(env, v) for k, v in _inputs(wide).items()},
                                   {k: v[:2] for k, v in good.items()}, 64, outputs=out)
    env["torch"].cuda.synchronize()
    for k in cr.KEYS:
        assert (out[k].cpu().numpy() == (PRE if k == "worst_excess" else PRE_INT)).all(), k

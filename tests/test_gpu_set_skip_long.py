"""Planner sets whose histories are longer than 32768 samples (engine.PlannerSet against
tpo.Planner, bit for bit): a skip-method set created with such a capacity, one whose history grows
past it inside one Plan, and the same long history with the uniform method.

Growth scenario: 2 planners, D = 2, N = 512, delta = 0.02 and a 10 ms time step. Planner 0 follows a
zigzag of 12 waypoints some 1270 long, i.e. about 63000 path samples, at a velocity limit of 1.0:
a Plan with a 960 s horizon solves 140 windows (max_planning_iterations = 200 admits them) and
leaves more than 32768 history samples, so a set that starts with room for 20000 doubles its
histories to 40000 in the middle of the window loop. Planner 1's path is short (9 windows). The
oracle planner does not report its history count; with the skip method every resampled sample
past the first is a history sample, so its num_samples is a lower bound, and that is asserted."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
import structured_paths

pytestmark = pytest.mark.gpu

MS = 1_000_000
S = 1000 * MS


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(eng=eng, tpo=tpo, torch=torch, E=eng.Engine(0))


def _oracle_planners(tpo, D, N, wps, offsets, vmax, amax, delta, step_ns, skip, iterations):
    planners = []
    for b in range(len(offsets) - 1):
        o = tpo.Planner(D, N, delta=float(delta[b]), time_step_ns=step_ns, skip=skip,
                        max_planning_iterations=iterations, max_initial_velocity_error=1e-2)
        o.set_limits(vmax[b], amax[b])
        o.set_waypoints(wps[offsets[b]:offsets[b + 1]], 0.2)
        planners.append(o)
    return planners


def _plan_and_compare(env, ps, oracle, start, horizon):
    """One Plan of the set and of every oracle planner: summaries and trajectories must be equal."""
    summary = ps.plan(start, horizon)
    traj = ps.download_trajectories()
    env["torch"].cuda.synchronize()
    off = traj["offsets"].cpu().numpy()
    for b, o in enumerate(oracle):
        rc = o.plan(int(start[b]), int(horizon))
        assert int(summary["status"][b]) == rc == 0, (b, rc, int(summary["status"][b]))
        r = slice(int(off[b]), int(off[b + 1]))
        assert r.stop - r.start == o.num_samples == int(summary["num_samples"][b]), b
        assert _bits(traj["time"][r]) == _bits(o.time), b
        assert _bits(traj["s"][r]) == _bits(o.path_parameter), b
        assert _bits(traj["q"][r]) == _bits(o.positions), b
        assert _bits(traj["qd"][r]) == _bits(o.velocities), b
        assert _bits(traj["qdd"][r]) == _bits(o.accelerations), b
        assert int(summary["end_time_ns"][b]) == o.end_time, b
        assert int(summary["final_decel_start_ns"][b]) == o.final_decel_start, b
        assert int(summary["windows"][b]) == o.windows, b
        assert bool(summary["target_reached"][b]) == o.target_reached, b
    return summary


def test_configured_capacity_above_32768(env):
    """history_capacity = 40000 on a skip-method set: three Plans at advancing start times."""
    eng, tpo = env["eng"], env["tpo"]
    B, D, N, step_ns = 4, 3, 64, 40 * MS
    b = structured_paths.make_family("out_and_back", B, D, N)
    W = b["waypoints"].shape[1]
    wps = np.ascontiguousarray(b["waypoints"].reshape(B * W, D))
    offsets = (W * np.arange(B + 1)).astype(np.int32)
    delta = b["delta"] / 8.0                 # the path is eight windows long
    with eng.PlannerSet(env["E"], B, D, N, num_points=3 * W - 2, time_step_ns=step_ns, sampling_method=1,
                        history_capacity=40000) as ps:
        status, _ = ps.set_waypoints(wps, offsets, b["vmax"], b["amax"], delta)
        assert (status == 0).all()
        oracle = _oracle_planners(tpo, D, N, wps, offsets, b["vmax"], b["amax"], delta, step_ns, True, 200)
        start = np.full(B, 5 * S, dtype=np.int64)
        moved = 0
        for step in range(3):
            summary = _plan_and_compare(env, ps, oracle, start, 1200 * MS)
            moved += int((summary["windows"] > 0).sum())
            start = np.minimum(summary["end_time_ns"].numpy(), start + 700 * MS)
        assert moved >= 2 * B


def _zigzag(L, W):
    return np.stack([np.linspace(0.0, L * W / 2, W), np.where(np.arange(W) % 2 == 0, 0.0, 0.8 * L)], axis=1)


@pytest.mark.parametrize("method", [1, 0])
def test_history_grows_across_32768_inside_a_plan(env, method):
    """See the module docstring. method 0: the uniform resampler over the same long history, which
    guards grow_rows and the shared window loop."""
    eng, tpo = env["eng"], env["tpo"]
    B, D, N, step_ns, iterations = 2, 2, 512, 10 * MS, 200
    paths = [_zigzag(120.0, 12), _zigzag(20.0, 5)]
    wps = np.concatenate(paths)
    offsets = np.array([0, 12, 17], dtype=np.int32)
    vmax, amax = np.array([[1.0, 1.2]] * B), np.array([[2.0, 2.5]] * B)
    delta = np.full(B, 0.02)
    # the skip-method oracle planner's sample count bounds the history count from below
    probe = _oracle_planners(tpo, D, N, wps, offsets, vmax, amax, delta, step_ns, True, iterations)[0]
    assert probe.plan(S, 960 * S) == 0 and probe.num_samples > 32768 + 64, probe.num_samples
    windows = probe.windows
    assert windows <= iterations
    with eng.PlannerSet(env["E"], B, D, N, num_points=34, time_step_ns=step_ns, sampling_method=method,
                        max_planning_iterations=iterations, history_capacity=20000) as ps:
        status, _ = ps.set_waypoints(wps, offsets, vmax, amax, delta)
        assert (status == 0).all()
        oracle = _oracle_planners(tpo, D, N, wps, offsets, vmax, amax, delta, step_ns, bool(method), iterations)
        before = ps.device_bytes
        start = np.full(B, S, dtype=np.int64)
        summary = _plan_and_compare(env, ps, oracle, start, 960 * S)
        assert int(summary["windows"][0]) == windows             # the same windows, so the same history
        assert int(summary["history_count"][0]) > 32768 and int(summary["history_count"][1]) < 20000
        assert ps.device_bytes > before
        assert (summary["status"] != 4).all()                    # no internal error
        for ahead, horizon in ((300 * MS, 1000 * S), (700 * MS, 1050 * S)):
            summary = _plan_and_compare(env, ps, oracle, start + ahead, horizon)
            assert int(summary["history_count"][0]) > 32768

"""A planner set driven from PyTorch (engine.PlannerSet): waypoints in a CUDA tensor are fitted on
the device (set_waypoints, the _device entry on torch's current stream), then plan() runs until
every planner is at its end. A handful of planners are followed by the oracle's planner
(tpo.Planner.set_waypoints + plan): the resident spline and every step's trajectory must equal it
bit for bit. Setpoints sampled into CUDA tensors must equal the host entry's, and bad input raises
TpamdError."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

MS = 1_000_000


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("D,method", [(3, 0), (7, 1)])
def test_planner_set_from_cuda_tensors_against_oracle(D, method):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    B, N, step_ns = 48, 200, (4 if method else 1) * MS
    rng = np.random.default_rng(20261016 + D)
    W = rng.integers(2, 7, size=B)      # a single waypoint is a zero-length path: Plan fails (internal), as the mirror
    offsets = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    wps = rng.uniform(-2.5, 2.5, size=(int(offsets[-1]), D))
    vmax = rng.uniform(1.0, 2.0, size=(B, D))
    amax = rng.uniform(2.0, 4.0, size=(B, D))
    delta = rng.uniform(0.01, 0.03, size=B)
    rounding = 0.2
    dev = torch.device("cuda", 0)
    E = eng.Engine(0)
    with eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=step_ns, sampling_method=method) as ps:
        # the whole path from a CUDA tensor: no spline crosses PCIe
        status, num_points = ps.set_waypoints(torch.from_numpy(wps).to(dev), offsets,
                                              torch.from_numpy(vmax).to(dev), torch.from_numpy(amax).to(dev),
                                              torch.from_numpy(delta).to(dev), rounding=rounding)
        assert status.is_cuda and num_points.is_cuda
        assert (status.cpu() == 0).all()
        assert (num_points.cpu().numpy() == np.where(W == 1, 4, 3 * W - 2)).all()
        # every planner is followed by the oracle's planner: status, resident spline and trajectory
        oracle = []
        for b in range(B):
            o = tpo.Planner(D, N, delta=float(delta[b]), time_step_ns=step_ns, skip=bool(method),
                            max_planning_iterations=200, max_initial_velocity_error=1e-2)
            o.set_limits(vmax[b], amax[b])
            cps, knots = o.set_waypoints(wps[offsets[b]:offsets[b + 1]], rounding)
            k, c = ps.download_path(b)
            assert _bits(k) == _bits(knots) and _bits(c) == _bits(cps), b
            oracle.append(o)

        def plan_and_compare(start, horizon, who):
            """One Plan of the set; planners `who` against their oracle planners. Returns the summary
            and the planners whose Plan failed (alike in both)."""
            summary = ps.plan(start, horizon)
            traj = ps.download_trajectories()
            torch.cuda.synchronize()
            off = traj["offsets"].cpu().numpy()
            failed = []
            for b in who:
                o = oracle[b]
                rc = o.plan(int(start[b]), horizon)
                assert int(summary["status"][b]) == rc, (b, rc, summary["status"][b])
                if rc != 0:
                    failed.append(b)
                    continue
                r = slice(int(off[b]), int(off[b + 1]))
                assert r.stop - r.start == o.num_samples == int(summary["num_samples"][b])
                assert _bits(traj["time"][r]) == _bits(o.time), b
                assert _bits(traj["s"][r]) == _bits(o.path_parameter), b
                assert _bits(traj["q"][r]) == _bits(o.positions), b
                assert _bits(traj["qd"][r]) == _bits(o.velocities), b
                assert _bits(traj["qdd"][r]) == _bits(o.accelerations), b
                assert int(summary["end_time_ns"][b]) == o.end_time
            return summary, failed

        # plan until every planner is at its end. A planner at its end is planned again at its end
        # time (GetNextPlanStartTime), which the reference can refuse (with uniform time sampling:
        # nothing left to resample); the set must refuse it alike, and that planner is followed no
        # further.
        target, steps, compared = 1000 * MS, 0, 0
        start = np.full(B, target, dtype=np.int64)
        alive = np.ones(B, dtype=bool)
        reached = np.zeros(B, dtype=bool)
        while True:
            last = steps >= 40
            horizon = 100000 * MS if last else 500 * MS
            who = np.flatnonzero(alive)
            summary, failed = plan_and_compare(start, horizon, who)
            steps += 1
            compared += len(who) - len(failed)
            assert reached[failed].all(), "a Plan fails only after the planner reached its end"
            alive[failed] = False
            at_end = ((summary["target_reached"] != 0) & (summary["path_state"] != 1) &
                      (summary["path_state"] != 2)).numpy()
            reached |= at_end & alive
            if reached.all() or last:
                break
            # GetNextPlanStartTime(target): min(end, max(target, start))
            target += 150 * MS
            start = np.minimum(summary["end_time_ns"].numpy(), np.maximum(target, summary["start_time_ns"].numpy()))
        assert reached.all(), "every planner reaches its end"
        assert alive.sum() >= B // 2 and compared >= 10 * B

        # setpoints into CUDA tensors equal the host entry's
        T = 16
        t0 = summary["start_time_ns"].to(dev)
        got = ps.sample_at_ticks(t0, step_ns, T)
        torch.cuda.synchronize()
        want = ps.sample_at_ticks(summary["start_time_ns"], step_ns, T, host=True)
        assert _bits(got["status"]) == _bits(want["status"])
        ok = want["status"].numpy() == 0
        assert ok.sum() > B
        for k in ("q", "qd", "qdd"):
            assert _bits(got[k].cpu().numpy()[ok]) == _bits(want[k].numpy()[ok]), k

        # a new goal for a few planners mid-stream, from CUDA tensors on a side stream, against the
        # oracle's planners given the same waypoints
        a = np.flatnonzero(alive)
        ids = np.array([a[1], a[0], a[2]], dtype=np.int32)
        off2 = np.array([0, 2, 5, 6], dtype=np.int32)
        w2 = rng.uniform(-2.5, 2.5, size=(6, D))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            st2, np2 = ps.set_waypoints(torch.from_numpy(w2).to(dev), off2, torch.from_numpy(vmax[ids]).to(dev),
                                        torch.from_numpy(amax[ids]).to(dev), torch.from_numpy(delta[ids]).to(dev),
                                        ids=ids, rounding=0.0)
        side.synchronize()
        assert (st2.cpu() == 0).all() and np2.cpu().tolist() == [4, 7, 4]
        for k, b in enumerate(ids):
            oracle[b].set_limits(vmax[b], amax[b])
            cps, knots = oracle[b].set_waypoints(w2[off2[k]:off2[k + 1]], 0.0)
            kk, cc = ps.download_path(b)
            assert _bits(kk) == _bits(knots) and _bits(cc) == _bits(cps), b
        target += 150 * MS
        start = np.minimum(summary["end_time_ns"].numpy(), np.maximum(target, summary["start_time_ns"].numpy()))
        summary, failed = plan_and_compare(start, 500 * MS, ids)
        assert not failed and all(int(summary["path_state"][b]) == 3 for b in ids)

        # the other entries answer from the same set
        sp = ps.stop_parameters(summary["start_time_ns"].numpy() + 20 * MS)
        assert sp["status"].shape == (B,)
        stops = ps.stop_trajectories(summary["start_time_ns"].to(dev) + 20 * MS, torch.from_numpy(amax).to(dev), 0.004)
        torch.cuda.synchronize()
        assert stops["status"].shape == (B,) and int(stops["offsets"][-1]) == stops["time"].shape[0]
        ps.reset([5])
        assert ps.download_path(5)[0].size == 0


def test_planner_set_bad_input_raises():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    B, D = 8, 3
    dev = torch.device("cuda", 0)
    E = eng.Engine(0)
    ps = eng.PlannerSet(E, B, D, 100, num_points=4)
    w = torch.zeros((4, D), dtype=torch.float64, device=dev)
    lim = torch.ones((2, D), dtype=torch.float64, device=dev)
    good_off = np.array([0, 2, 4], dtype=np.int32)
    with pytest.raises(eng.TpamdError):       # an id listed twice
        ps.set_waypoints(w, good_off, lim, lim, 0.01, ids=[1, 1])
    with pytest.raises(eng.TpamdError):       # an id out of range
        ps.set_waypoints(w, good_off, lim, lim, 0.01, ids=[1, B])
    with pytest.raises(eng.TpamdError):       # offsets not from 0
        ps.set_waypoints(w, np.array([1, 2, 4], dtype=np.int32), lim, lim, 0.01)
    with pytest.raises(eng.TpamdError):       # decreasing offsets
        ps.set_waypoints(w, np.array([0, 3, 2], dtype=np.int32), lim, lim, 0.01)
    with pytest.raises(eng.TpamdError):       # limits of the wrong shape
        ps.set_waypoints(w, good_off, lim[:1], lim, 0.01)
    with pytest.raises(eng.TpamdError):       # the host entry checks the same
        ps.set_waypoints(w.cpu(), good_off, lim.cpu(), lim.cpu(), 0.01, ids=[0, 0])
    with pytest.raises(eng.TpamdError):
        ps.sample_at_ticks(torch.zeros(2, dtype=torch.int64, device=dev), 0, 4)      # step_ns <= 0
    # nothing changed: no planner has a path
    assert all(ps.download_path(b)[0].size == 0 for b in range(B))
    st, npts = ps.set_waypoints(w.cpu(), np.array([0, 0, 4], dtype=np.int32), lim.cpu(), lim.cpu(), 0.01)
    assert st.tolist() == [3, 0] and npts.tolist() == [0, 10]  # no waypoints: INVALID_ARGUMENT, no path
    ps.close()
    with pytest.raises(eng.TpamdError):
        ps.plan(0, 1)

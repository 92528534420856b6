"""PlannerSet.retarget (k_pset_retarget) at every joint count D = 1..16 from Python with CUDA
tensors, five planners each: retargeted at 15 %, 50 % and 90 % of their trajectories, one without
new waypoints, one at the last sample of its path (at rest where that sample's time can be named). Held against code that shares nothing with the
kernel: the readout against tests/switch_reference.py (TrajectoryBuffer's bracket and lerp), the
stopping point against the long-double restatement of tests/path_tools_reference.py within the
bound recorded in tests/test_path_tools_cpu.py, the fit against the oracle's joint_fit_spline bit
for bit, and the next Plan against oracle.tpo.Planner given that spline and the velocity as initial
velocity, bit for bit."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
import path_tools_reference as ref
import switch_reference as sw
from test_path_tools_cpu import STOP_ERROR_BOUND

pytestmark = pytest.mark.gpu

ALL_DOFS = list(range(1, 17))
MS = 1_000_000
B, N, DELTA, ROUNDING = 5, 100, 0.005, 0.2
START, HORIZON = 1000 * MS, 400 * MS
AT_END, NO_WAYPOINTS = 4, 3


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), tpo=tpo)


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("D", ALL_DOFS)
def test_retarget(env, D):
    torch, eng, E, dev, tpo = env["torch"], env["eng"], env["E"], env["dev"], env["tpo"]
    rng = np.random.default_rng(900 + D)
    cuda = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    first = [rng.uniform(-1.5, 1.5, size=(int(rng.integers(2, 5)), D)) for _ in range(B)]
    vmax, amax = rng.uniform(1, 2, size=(B, D)), rng.uniform(2, 5, size=(B, D))
    off = np.concatenate([[0], np.cumsum([len(w) for w in first])]).astype(np.int32)
    with eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=MS) as ps:
        status, _ = ps.set_waypoints(cuda(np.concatenate(first)), off, cuda(vmax), cuda(amax), DELTA, rounding=ROUNDING)
        horizon = np.full(B, HORIZON, dtype=np.int64)
        horizon[AT_END] = 100_000 * MS
        s1 = ps.plan(START, horizon)
        assert (status.cpu().numpy() == 0).all() and (s1["status"].numpy() == 0).all(), (D, s1["status"])
        traj = ps.download_trajectories()
        torch.cuda.synchronize()
        rows = traj["offsets"].cpu().numpy()
        tj = {k: traj[k].cpu().numpy() for k in ("time", "q", "qd")}
        # the oracle's planners follow from the start
        oracle = []
        for b in range(B):
            o = tpo.Planner(D, N, delta=DELTA, time_step_ns=MS, max_planning_iterations=200, max_initial_velocity_error=1e-2)
            o.set_limits(vmax[b], amax[b])
            o.set_waypoints(first[b], ROUNDING)
            assert o.plan(START, int(horizon[b])) == 0
            assert _bits(o.positions) == _bits(tj["q"][rows[b]:rows[b + 1]]), (D, b, "first plan")
            oracle.append(o)
        # the retarget: shuffled ids, CUDA tensors
        ids = rng.permutation(B).astype(np.int32)
        t0, t1 = s1["start_time_ns"].numpy(), s1["end_time_ns"].numpy()
        fraction = {0: 0.15, 1: 0.5, 2: 0.9, NO_WAYPOINTS: 0.5, AT_END: 1.0}
        t_ns = np.array([t0[b] + int(round(fraction[int(b)] * (t1[b] - t0[b]) / MS)) * MS for b in ids], dtype=np.int64)
        # the last sample of the planner at its path's end (at rest there), if its time is a whole
        # number of nanoseconds as a double; otherwise the nanosecond before it, where it still creeps
        last = float(tj["time"][rows[AT_END + 1] - 1])
        t_end = int(round(last * 1e9))
        t_ns[list(ids).index(AT_END)] = t_end - (1 if t_end / 1e9 > last else 0)
        new = [np.zeros((0, D)) if b == NO_WAYPOINTS else rng.uniform(-1.5, 1.5, size=(int(rng.integers(2, 5)), D))
               for b in ids]
        noff = np.concatenate([[0], np.cumsum([len(w) for w in new])]).astype(np.int32)
        nvmax, namax = rng.uniform(1, 2, size=(B, D)), rng.uniform(2, 5, size=(B, D))
        stop_acc = namax * np.array([1.0, 0.8, 0.72, 0.8, 1.0])[:, None]
        got = ps.retarget(cuda(t_ns), cuda(np.concatenate(new)), noff, cuda(nvmax), cuda(namax), DELTA, ids=ids,
                          rounding=ROUNDING, stopping_acceleration=cuda(stop_acc))
        assert all(v.is_cuda for v in got.values())
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in got.items()}
        assert (got["status"] == 0).all(), (D, got["status"])
        lists, moving = [], 0
        for k, b in enumerate(ids):
            where = (D, k, int(b))
            times = tj["time"][rows[b]:rows[b + 1]].tolist()
            t_sec = float(t_ns[k]) / 1e9
            # the readout: TrajectoryBuffer's bracket and lerp, restated
            for name, key in (("position", "q"), ("velocity", "qd")):
                st, want = sw.velocity_at_time(times, tj[key][rows[b]:rows[b + 1]].tolist(), t_sec)
                assert st == sw.OK and _bits(got[name][k]) == _bits(want), where + (name,)
            q, qd, stop = got["position"][k], got["velocity"][k], got["stopping_point"][k]
            # the stopping point: the long-double restatement and what a stopping point is
            st, want, parts = ref.compute_stopping_point(q, qd, stop_acc[k], ROUNDING)
            assert st == ref.OK
            at_rest = parts is None
            assert not at_rest or b == AT_END, where + ("at rest", np.abs(qd).max())
            if at_rest:
                assert _bits(stop) == _bits(q), where
            else:
                err = ref.stopping_point_error(stop, q, qd, stop_acc[k], ROUNDING)
                assert err <= STOP_ERROR_BOUND, where + (err,)
                ref.check_stopping_point(stop, q, qd, stop_acc[k], ROUNDING, rel=STOP_ERROR_BOUND)
                moving += 1
            # the fit of [position, stopping point, waypoints...]: the oracle's, bit for bit
            lst = np.concatenate([q[None], new[k]] if at_rest else [q[None], stop[None], new[k]])
            cps, knots = tpo.joint_fit_spline(lst, ROUNDING)
            path = ps.download_path(int(b))
            assert int(got["num_points"][k]) == len(cps) == (4 if len(lst) == 1 else 3 * len(lst) - 2), where
            assert _bits(path[0]) == _bits(knots) and _bits(path[1]) == _bits(cps), where + ("fit differs",)
            lists.append((cps, knots))
        assert moving >= B - 1
        # the next Plan, each planner from its retarget time: the oracle's planner on that spline
        start2 = np.zeros(B, dtype=np.int64)
        start2[ids] = t_ns
        s2 = ps.plan(start2, HORIZON)
        traj2 = ps.download_trajectories()
        torch.cuda.synchronize()
        rows2 = traj2["offsets"].cpu().numpy()
        tj2 = {k: traj2[k].cpu().numpy() for k in ("time", "s", "q", "qd", "qdd")}
        for k, b in enumerate(ids):
            where = (D, k, int(b), "plan")
            o = oracle[b]
            o.set_limits(nvmax[k], namax[k])
            o.set_spline(lists[k][1], lists[k][0], 1)
            o.set_initial_velocity(got["velocity"][k])
            rc = o.plan(int(t_ns[k]), HORIZON)
            assert int(s2["status"][b]) == rc, where + (int(s2["status"][b]), rc)
            if b != AT_END:
                assert rc == 0, where                  # a moving planner's first Plan after the retarget is OK
            if rc != 0:
                continue
            assert int(s2["num_samples"][b]) == o.num_samples, where
            sl = slice(rows2[b], rows2[b + 1])
            for key, want in (("time", o.time), ("s", o.path_parameter), ("q", o.positions), ("qd", o.velocities),
                              ("qdd", o.accelerations)):
                assert _bits(tj2[key][sl]) == _bits(want), where + (key,)

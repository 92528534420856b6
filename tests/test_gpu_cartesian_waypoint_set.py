"""Cartesian goals from pose waypoints to Plan on the GPU (PlannerSet.set_pose_waypoints and, through
tests/cpp/test_cartesian_waypoint_set_gpu.cc, PathTimingTrajectorySet::SetCartesianWaypointPaths): the
device fit, the row counts, the device targets, a device IK that returns the joint targets unchanged
and one fixed Jacobian per planner, and the resident tables. The joint targets are bit-exact, so the
tables equal the ones built on the host from the oracle's joint sampling and every Plan equals the
oracle's IK-table planner bit for bit."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pose_fit_reference as pfr
from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu

MS = 1_000_000
B, N = 6, 64
DELTA = 0.5
TPAMD_PLAN_INVALID_ARGUMENT = 3


def _oracle_planner(tpo, D, table_q, table_J, path_end, vmax, amax, vt, vr):
    """One oracle IK-table planner (oracle/tp_oracle_plan.c: tpo_planner_set_ik_table), driven as
    tests/cpp/test_cartesian_set_gpu.cc drives it."""
    p = tpo.Planner(D, N, delta=DELTA, safety=0.8, time_step_ns=4 * MS, max_planning_iterations=10000,
                    max_initial_velocity_error=1e-3)
    p.set_limits(vmax, amax)
    L = p._L
    L.tpo_planner_set_ik_table.restype = None
    L.tpo_planner_set_ik_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double,
                                           C.c_double, C.c_int]
    q, J = np.ascontiguousarray(table_q), np.ascontiguousarray(table_J)
    L.tpo_planner_set_ik_table(p._p, q.ctypes.data, J.ctypes.data, q.shape[0], float(path_end), float(vt), float(vr), 1)
    return p


def _host_table(tpo, knots, jcp, jacobian, rows):
    """Rows r * DELTA of the joint spline through the oracle (EvalCurve below knots.back() - delta, the
    last control point from there on) and the planner's fixed Jacobian on every row."""
    q = np.zeros((rows, jcp.shape[1]))
    for r in range(rows):
        u = r * DELTA
        if u < knots[-1] - DELTA:
            rc, q[r] = tpo.eval_curve(knots, 2, jcp, u)
            assert rc == 0
        else:
            q[r] = jcp[-1]
    return q, np.ascontiguousarray(np.broadcast_to(jacobian, (rows,) + jacobian.shape))


@pytest.mark.parametrize("D", [6, 7])
def test_pose_waypoints_to_plan_against_the_oracle(D):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(600 + D)
    goals = [pfr.make_case("random", 2 + b % 3, D, rng) for b in range(B)]
    jac = 0.25 * rng.uniform(-1, 1, (B, 6, D)) + (np.arange(6)[:, None] == np.arange(D)[None, :] % 6)
    vmax, amax = rng.uniform(0.6, 1.1, (B, D)), rng.uniform(1.5, 3.0, (B, D))
    vt, vr = rng.uniform(0.4, 0.6, B), rng.uniform(0.8, 1.2, B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    calls = []

    def make_ik(planners):
        def ik(pose_targets, joint_targets, row_offsets):
            assert pose_targets.is_cuda and joint_targets.is_cuda and pose_targets.shape == (row_offsets[-1], 7)
            calls.append((pose_targets.cpu().numpy(), joint_targets.cpu().numpy(), np.array(row_offsets)))
            counts = torch.as_tensor(np.diff(row_offsets), device=dev)
            J = torch.repeat_interleave(up(jac[planners]), counts, dim=0)
            return joint_targets.clone(), J.contiguous()
        return ik

    def pack(which):
        off = np.concatenate([[0], np.cumsum([goals[b][0].shape[0] for b in which])]).astype(np.int32)
        pose = np.concatenate([goals[b][0] for b in which] + [np.zeros((0, 7))])
        joints = np.concatenate([goals[b][1] for b in which] + [np.zeros((0, D))])
        return up(pose), up(joints), off

    E = eng.Engine(0)
    kw = dict(time_step_ns=4 * MS, max_planning_iterations=10000, max_initial_velocity_error=1e-3, cartesian=True)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as ps:
        pose, joints, off = pack(range(B))
        status, rows = ps.set_pose_waypoints(pose, joints, off, make_ik(list(range(B))), up(vmax), up(amax), up(vt), up(vr),
                                             DELTA, translation_rounding=0.05, rotation_rounding=0.2)
        assert (status == 0).all() and len(calls) == 1
        # the fit once more through the host entry: the knots and joint control points of the chain
        fit = E.fit_pose_waypoints(pose.cpu().numpy(), joints.cpu().numpy(), off, 0.05, 0.2)
        planners, ko = [], 0
        for b in range(B):
            P, p0 = int(fit["num_points"][b]), int(fit["point_offsets"][b])
            knots = fit["knots"][ko:ko + P + 3]
            ko += P + 3
            jcp = fit["joint_control_points"][p0:p0 + P]
            assert jcp.tobytes() == tpo.polyline_to_bspline3_waypoints(goals[b][1], 0.2).tobytes()
            want_rows = int(np.floor(knots[-1] / DELTA + 0.5)) + N + 1
            assert rows[b] == want_rows == E.ik_table_rows(knots[-1], DELTA, N)
            tq, tJ = _host_table(tpo, knots, jcp, jac[b], want_rows)
            gq, gJ = ps.download_ik_table(b)
            assert gq.tobytes() == tq.tobytes() and gJ.tobytes() == tJ.tobytes(), b
            planners.append(_oracle_planner(tpo, D, tq, tJ, knots[-1], vmax[b], amax[b], vt[b], vr[b]))
        # the IK saw one pose target per row: unit quaternions, padded rows equal to the last control pose
        pose_t, joint_t, ro = calls[0]
        assert np.allclose(np.linalg.norm(pose_t[:, 3:], axis=1), 1.0, atol=1e-12)
        assert pose_t[ro[1] - 1].tobytes() == np.concatenate([fit["translation_points"][fit["point_offsets"][1] - 1],
                                                              fit["rotation_points"][fit["point_offsets"][1] - 1]]).tobytes()
        # the first plan and two replans against the oracle planners
        start = np.zeros(B, dtype=np.int64)
        for step in range(3):
            s = ps.plan(start, 6000 * MS)
            t = ps.download_trajectories()
            torch.cuda.synchronize()
            offs = t["offsets"].cpu().numpy()
            for b in range(B):
                assert planners[b].plan(int(start[b]), 6000 * MS) == 0 and int(s["status"][b]) == 0, (step, b)
                assert int(s["num_samples"][b]) == planners[b].num_samples
                assert int(s["end_time_ns"][b]) == planners[b].end_time
                assert int(s["final_decel_start_ns"][b]) == planners[b].final_decel_start
                r = slice(int(offs[b]), int(offs[b + 1]))
                for name, ref in (("time", planners[b].time), ("s", planners[b].path_parameter),
                                  ("q", planners[b].positions), ("qd", planners[b].velocities),
                                  ("qdd", planners[b].accelerations)):
                    assert t[name][r].cpu().numpy().tobytes() == ref.tobytes(), (step, b, name)
            start = np.minimum(np.array([p.end_time for p in planners]), start + 2000 * MS)
        # an empty waypoint list: planner 2 keeps its path and plan, 0 and 4 get new goals
        before_q, before_J = ps.download_ik_table(2)
        before = {k: v.clone() for k, v in ps.download_trajectories(ids=[2]).items()}
        goals[0] = pfr.make_case("random", 3, D, rng)
        goals[4] = pfr.make_case("random", 4, D, rng)
        off3 = np.array([0, 3, 3, 7], dtype=np.int32)
        pose3, joints3 = up(np.concatenate([goals[0][0], goals[4][0]])), up(np.concatenate([goals[0][1], goals[4][1]]))
        sel = [0, 2, 4]
        status, rows3 = ps.set_pose_waypoints(pose3, joints3, off3, make_ik([0, 4]), up(vmax[sel]), up(amax[sel]),
                                              up(vt[sel]), up(vr[sel]), DELTA, ids=sel)
        assert status.tolist() == [0, TPAMD_PLAN_INVALID_ARGUMENT, 0] and rows3[1] == 0 and len(calls) == 2
        after_q, after_J = ps.download_ik_table(2)
        assert after_q.tobytes() == before_q.tobytes() and after_J.tobytes() == before_J.tobytes()
        after = ps.download_trajectories(ids=[2])
        torch.cuda.synchronize()
        for name in before:
            assert after[name].cpu().numpy().tobytes() == before[name].cpu().numpy().tobytes(), name
        fit3 = E.fit_pose_waypoints(pose3.cpu().numpy(), joints3.cpu().numpy(), np.array([0, 3, 7], dtype=np.int32), 0.05, 0.2)
        ko = 0
        for k, b in enumerate((0, 4)):
            P, p0 = int(fit3["num_points"][k]), int(fit3["point_offsets"][k])
            knots = fit3["knots"][ko:ko + P + 3]
            ko += P + 3
            tq, tJ = _host_table(tpo, knots, fit3["joint_control_points"][p0:p0 + P], jac[b], int(rows3[2 * k]))
            gq, gJ = ps.download_ik_table(b)
            assert gq.tobytes() == tq.tobytes() and gJ.tobytes() == tJ.tobytes(), b
        s = ps.plan(start, 6000 * MS)
        t = ps.download_trajectories()
        torch.cuda.synchronize()
        offs = t["offsets"].cpu().numpy()
        assert (s["status"] == 0).all()
        for b in (1, 2, 3, 5):                        # the others are not disturbed
            assert planners[b].plan(int(start[b]), 6000 * MS) == 0
            r = slice(int(offs[b]), int(offs[b + 1]))
            assert t["time"][r].cpu().numpy().tobytes() == planners[b].time.tobytes(), b
            assert t["q"][r].cpu().numpy().tobytes() == planners[b].positions.tobytes(), b
    with eng.PlannerSet(E, 2, D, N, time_step_ns=4 * MS) as joint_set:
        with pytest.raises(eng.TpamdError):
            joint_set.set_pose_waypoints(pose, joints, off[:2], make_ik([0]), np.ones((1, D)), np.ones((1, D)), 0.5, 1.0,
                                         DELTA, ids=[0])
        assert len(calls) == 2


def test_cartesian_waypoint_sets_through_the_mirror(tmp_path):
    """tests/cpp/test_cartesian_waypoint_set_gpu.cc: the same scenario through
    PathTimingTrajectorySet::SetCartesianWaypointPaths."""
    require_gpu()
    exe = build_driver("test_cartesian_waypoint_set_gpu.cc", tmp_path, libs=("host", "engine", "oracle", "hip", "m"),
                       flags=("-pthread",))
    out = run_driver(exe, timeout=600)
    for D in (6, 7):
        assert "D %d: 6 of 6 resident tables equal the host-built ones" % D in out
        assert "D %d: 18 of 18 plans equal the oracle planners" % D in out
        assert "D %d: empty waypoint list: InvalidArgument, planner kept, others loaded and undisturbed" % D in out
    assert "SetCartesianWaypointPaths on a joint set: refused" in out

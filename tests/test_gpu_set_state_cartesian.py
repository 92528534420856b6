"""Planner state records of Cartesian planner sets on the GPU: the resident IK rows, the Cartesian
limits and the path end travel with the planner.

A whole table: a set planned twice hands its planners (reversed ids, export + import) to a fresh
set with the smallest table capacity, both plan on, bit-equal. A streamed table after
discard_ik_rows (first_row > 0): the receiver (copy_planners, a smaller table) appends rows and
plans on with plan_streaming, bit-equal to the twin; what a host mirror knows about where the rows
come from (the fitted spline, the IK seed) is not part of a record and is handed over by the test.
A planner that waits for IK rows refuses export, import and copy. D in {6, 7}, N = 33, tables of 81
and 129 rows."""
import importlib

import numpy as np
import pytest

import pose_fit_reference as pfr
import set_state_cases as cases
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

MS = 1_000_000
B, N = 4, 33


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return dict(torch=torch, eng=eng, E=cases.engine(), dev=torch.device("cuda", 0))


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


def _setup(env, D, method, seed, fractions=(0.4, 0.25)):
    torch, dev = env["torch"], env["dev"]
    rng = np.random.default_rng(seed + D)
    goals = [pfr.make_case("random", 3 + b % 3, D, rng) for b in range(B)]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = torch.arange(6, device=dev, dtype=torch.float64)[None, :, None]
    d = torch.arange(D, device=dev, dtype=torch.float64)[None, None, :]

    def ik(pose_targets, joint_targets, row_offsets, seed_rows=None):
        q = joint_targets.clone()
        J = (0.2 * torch.sin(q[:, None, :] * (c + 1.0) + 0.31 * d) + (c == d)).contiguous()
        return q, J

    off = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in goals])]).astype(np.int32)
    pose, joints = up(np.concatenate([g[0] for g in goals])), up(np.concatenate([g[1] for g in goals]))
    fit = env["E"].fit_pose_waypoints(pose, joints, off, up(np.full(B, 0.05)), up(np.full(B, 0.2)))
    path_end = fit["path_end"].cpu().numpy()
    # a window covers this fraction of the path: tables of (N - 1) / fraction + 1 + N rows
    delta = np.where(np.arange(B) % 2, fractions[1], fractions[0]) * path_end / (N - 1)
    limits = (up(rng.uniform(0.6, 1.1, (B, D))), up(rng.uniform(1.5, 3.0, (B, D))), up(rng.uniform(0.4, 0.6, B)),
              up(rng.uniform(0.8, 1.2, B)), up(delta))
    kw = dict(time_step_ns=4 * MS, sampling_method=method, max_planning_iterations=10000,
              max_initial_velocity_error=1e-3, cartesian=True)
    return dict(ik=ik, off=off, pose=pose, joints=joints, limits=limits, kw=kw)


def _same_dict(a, b, what):
    assert a.keys() == b.keys()
    for name in a:
        if not name.startswith("_"):
            assert _bits(a[name]) == _bits(b[name]), (what, name)


@pytest.mark.parametrize("D,method", [(6, 0), (7, 1)])
def test_whole_tables_move_and_plan_on(env, D, method):
    torch, eng, E = env["torch"], env["eng"], env["E"]
    s = _setup(env, D, method, 4100)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **s["kw"]) as a, \
            eng.PlannerSet(E, B + 2, D, N, table_capacity=1, history_capacity=2 * N, trajectory_capacity=8, **s["kw"]) as b:
        st, rows = a.set_pose_waypoints(s["pose"], s["joints"], s["off"], s["ik"], *s["limits"])
        assert (st == 0).all() and len(set(rows.tolist())) == 2 and 40 <= rows.min() and rows.max() <= 200, rows
        start = np.zeros(B, dtype=np.int64)
        for _ in range(2):
            sa = a.plan(start, 400 * MS)
            assert (sa["status"].numpy() == 0).all()
            start = np.minimum(sa["end_time_ns"].numpy(), start + 150 * MS)
        info = a.state_info()
        assert info["table_rows"].tolist() == rows.tolist() and (info["first_row"] == 0).all()
        assert (info["num_points"] == 0).all() and (info["history_count"] > 0).all()
        blob, off = a.export_state()
        recs = cases.split(blob, off)
        for j, r in enumerate(recs):
            p = cases.parse_record(r)
            assert p["pad_ok"] and p["head"]["kind"] == 1 and p["head"]["table_rows"] == rows[j]
            q, J = a.download_ik_table(j)
            assert _bits(p["table_q"]) == _bits(q) and _bits(p["table_J"]) == _bits(J), j
        rev = np.array([4, 3, 2, 1], dtype=np.int32)
        got = b.import_state(blob.cpu().numpy(), off, ids=rev)
        assert (got["status"].numpy() == 0).all()
        assert cases.split(*b.export_state(ids=rev)) == recs
        assert [b.ik_table_info(int(x))[:2] for x in rev] == [(0, int(r)) for r in rows]
        for step in range(3):
            sa = a.plan(start, 400 * MS)
            sb_start = np.zeros(B + 2, dtype=np.int64)
            sb_start[rev] = start
            sb = b.plan(sb_start, 400 * MS)
            for name in sa:
                assert _bits(sa[name]) == _bits(sb[name][torch.from_numpy(rev.astype(np.int64))]), (step, name)
            ta, tb = a.download_trajectories(), b.download_trajectories(ids=rev)
            torch.cuda.synchronize()
            _same_dict(ta, tb, step)
            start = np.minimum(sa["end_time_ns"].numpy(), start + 150 * MS)
        assert cases.split(*b.export_state(ids=rev)) == cases.split(*a.export_state())


@pytest.mark.parametrize("D,method", [(6, 1), (7, 0)])
def test_discarded_tables_move_and_stream_on(env, D, method):
    torch, eng, E = env["torch"], env["eng"], env["E"]
    s = _setup(env, D, method, 4200, fractions=(0.2, 0.25))
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **s["kw"]) as a, \
            eng.PlannerSet(E, B, D, N, table_capacity=2, history_capacity=2 * N, **s["kw"]) as b:
        st, rows = a.set_pose_waypoints(s["pose"], s["joints"], s["off"], s["ik"], *s["limits"], streaming=True)
        assert (st == 0).all() and (rows == N).all()
        start = np.zeros(B, dtype=np.int64)
        for step in range(20):
            sa, _, need = a.plan_streaming(start, 150 * MS, s["ik"], discard=True)
            assert (sa["status"].numpy() == 0).all() and not need.any()
            start = np.minimum(sa["end_time_ns"].numpy(), start + 100 * MS)
            if all(a.ik_table_info(j)[0] > 0 for j in range(B)):
                break
        info = a.state_info()
        assert (info["first_row"] > 0).all() and (info["table_rows"] > info["first_row"]).all(), info
        full = a._stream_fit["full_rows"]
        assert 40 <= full.min() and full.max() <= 200 and (info["table_rows"] < full).any(), (info["table_rows"], full)
        got = b.copy_from(a)
        assert (got["status"].numpy() == 0).all()
        recs = cases.split(*a.export_state())
        assert cases.split(*b.export_state()) == recs
        for j in range(B):
            p = cases.parse_record(recs[j])
            f, q, J = a.download_ik_rows(j)
            assert p["pad_ok"] and p["head"]["first_row"] == f == b.ik_table_info(j)[0]
            assert _bits(p["table_q"]) == _bits(q) and _bits(p["table_J"]) == _bits(J), j
            assert b.ik_table_info(j)[:2] == a.ik_table_info(j)[:2]
        # where the rows come from is the mirror's knowledge, not the record's
        b._stream_fit, b._stream_last = a._stream_fit, a._stream_last.clone()
        appended = 0
        for step in range(12):
            if step >= 3 and appended > 0:
                break
            sa, _, _ = a.plan_streaming(start, 800 * MS, s["ik"], discard=True)
            appended += a.last_stream_stats["appended_rows"]
            sb, _, _ = b.plan_streaming(start, 800 * MS, s["ik"], discard=True)
            assert a.last_stream_stats["appended_rows"] == b.last_stream_stats["appended_rows"]
            _same_dict(sa, sb, step)
            ta, tb = a.download_trajectories(), b.download_trajectories()
            torch.cuda.synchronize()
            _same_dict(ta, tb, step)
            start = np.minimum(sa["end_time_ns"].numpy(), start + 400 * MS)
        assert appended > 0, "the receiver appended rows behind the ones it was handed"
        assert cases.split(*b.export_state()) == cases.split(*a.export_state())


def test_a_planner_that_waits_for_rows_is_refused(env):
    torch, eng, E = env["torch"], env["eng"], env["E"]
    D = 6
    s = _setup(env, D, 0, 4300)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **s["kw"]) as a, \
            eng.PlannerSet(E, B, D, N, table_capacity=N, **s["kw"]) as b:
        a.set_pose_waypoints(s["pose"], s["joints"], s["off"], s["ik"], *s["limits"], streaming=True)
        clean = cases.split(*a.export_state())
        summary, need_first, need_count = a._plan_streaming(np.zeros(B, dtype=np.int64), 600000 * MS)
        waits = need_count > 0
        assert waits.any(), "a long horizon reaches past the first N rows"
        want = np.where(waits, cases.FAILED_PRECONDITION, 0).tolist()
        assert a.state_info()["status"].tolist() == want
        blob, off = a.export_state()
        torch.cuda.synchronize()
        assert a.last_export_status.cpu().numpy().tolist() == want
        # nothing is imported into a planner that waits
        before = cases.split(blob, off)
        cb, co = cases.pack(clean)
        assert a.import_state(cb, co)["status"].numpy().tolist() == want
        got = a.import_state(torch.from_numpy(cb).cuda(), co)
        torch.cuda.synchronize()
        assert got["status"].cpu().numpy().tolist() == want
        # and nothing is copied out of a set while one of the listed planners waits
        untouched = cases.split(*b.export_state())
        assert b.copy_from(a)["status"].numpy().tolist() == want
        assert cases.split(*b.export_state()) == untouched
        del before

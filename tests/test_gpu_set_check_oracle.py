"""Planner-set checking against the CPU oracle, one window per planner: paths whose N samples cover
the whole spline (or IK table) are planned from start 0 with a horizon longer than any of them, so
every planner finishes in its first window and that window is the oracle's solve of the same path
with sd_start = time_start = 0. The set's record must then be the record check_reference.check_rows
gives on the oracle's own rows and solution, bit for bit, and its count the oracle's
SolutionSatisfiesConstraints count.

Which inputs violate is established on the CPU (each test asserts it before it creates a set):
make_joint_batch(64, 7, 200, 10) has violating paths (INTEGRATION.md counts 3 of 64), the Cartesian
batch (16, 14, 129, 6) 14 of 16."""
import importlib

import numpy as np
import pytest

import check_reference as cr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

HORIZON_NS = 10 ** 12          # longer than any of the paths takes
FIELDS = ("violations", "worst_excess", "worst_sample", "worst_row", "first_sample")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    from oracle import tpo
    tpo.build()
    eng = importlib.import_module(PKG_NAME + ".engine")
    E = eng.Engine(0)
    yield dict(tpo=tpo, eng=eng, syn=importlib.import_module(PKG_NAME + ".synthetic"), E=E)
    E.close()


def oracle_windows(tpo, rows_of, B, s_end):
    """Per path: (rc, SolutionSatisfiesConstraints count, check_rows record, the oracle's s)."""
    out = []
    for b in range(B):
        rows = rows_of(b)
        rc, p = cr.oracle_profile(tpo, rows, 0.0, s_end[b], 0.0, 0.0)
        rec = cr.check_rows(*rows, p.sd2, p.sdd) if rc == 0 else cr.NOT_CHECKED
        out.append((rc, p.constraint_violations(), rec, p.s))
    return out


def compare(summary, got, want, need_violations):
    solved = violating = 0
    for b, (rc, count, rec, s) in enumerate(want):
        if rc != 0:
            continue
        solved += 1
        g = got[b]
        assert int(summary["status"][b]) == 0 and int(summary["windows"][b]) == 1, b
        assert g["windows"] == 1, b
        assert g["violations"] == count and g["last_window_violations"] == count, (b, g, count)
        assert cr.same_record(tuple(g[k] for k in FIELDS), rec), (b, g, rec)
        assert g["worst_window"] == 0 and g["first_window"] == (0 if count else -1), (b, g)
        assert g["worst_parameter"].tobytes() == np.float64(s[rec[2]]).tobytes(), (b, g, s[rec[2]])
        violating += count > 0
    assert solved > 0
    if need_violations:
        assert violating > 0
    return solved, violating


def plan_once(ps, B):
    zeros = np.zeros(B, dtype=np.int64)
    return ps.plan(zeros, np.full(B, HORIZON_NS, dtype=np.int64))


@pytest.mark.parametrize("shape,need_violations", [((64, 7, 200, 10), True), ((16, 1, 3, 2), False),
                                                   ((16, 16, 33, 3), True)])
def test_joint_window_records_equal_the_oracle(env, shape, need_violations):
    B, D, N, W = shape
    eng, tpo = env["eng"], env["tpo"]
    batch = env["syn"].make_joint_batch(B, D, N, W)
    want = oracle_windows(tpo, lambda b: cr.joint_rows(tpo, batch, b, N), B, batch["delta"] * (N - 1))
    if need_violations:      # known before anything runs on the GPU
        assert any(rc == 0 and count > 0 for rc, count, _, _ in want)
    P = batch["control_points"].shape[1]
    with eng.PlannerSet(env["E"], B, D, N, num_points=P) as ps:
        assert not ps.checking
        bytes_off = ps.device_bytes
        ps.set_checking(True)
        assert ps.checking and ps.device_bytes >= bytes_off + B * N * 8 + B * 48
        ps.set_paths(batch["knots"], batch["control_points"], np.full(B, P), batch["vmax"], batch["amax"],
                     batch["delta"])
        summary = plan_once(ps, B)
        compare(summary, ps.check_results(), want, need_violations)
        # a subset, in another order
        ids = np.array([B - 1, 0, 3], dtype=np.int32)
        sub, full = ps.check_results(ids), ps.check_results()
        assert sub.tobytes() == full[ids].tobytes()
        # switched off: "nothing checked", whatever the records hold
        ps.set_checking(False)
        off = ps.check_results()
        assert (off["windows"] == 0).all() and (off["violations"] == -1).all() and np.isnan(off["worst_excess"]).all()


def test_ragged_waypoint_paths_equal_the_oracle(env):
    """2 .. 6 waypoints per planner through set_waypoints: every planner's own control-point count."""
    B, D, N = 20, 7, 64
    eng, tpo, syn = env["eng"], env["tpo"], env["syn"]
    rng = np.random.default_rng(7)
    counts = 2 + np.arange(B) % 5
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    wps = rng.uniform(-2.0, 2.0, (int(offsets[-1]), D))
    vmax, amax = rng.uniform(1.0, 2.0, (B, D)), rng.uniform(2.0, 4.0, (B, D))
    # delta from the host fit's parameter length, so that N samples cover the path
    delta = np.array([syn.fit_joint_splines(wps[None, offsets[b]:offsets[b + 1]])[1][0, -1] / (N - 1) for b in range(B)])
    with eng.PlannerSet(env["E"], B, D, N) as ps:
        ps.set_checking(True)
        status, num_points = ps.set_waypoints(wps, offsets, vmax, amax, delta)
        assert (status.numpy() == 0).all() and len(set(num_points.numpy().tolist())) > 1
        paths = [ps.download_path(b) for b in range(B)]

        def rows_of(b):
            knots, cps = (np.asarray(x, dtype=np.float64) for x in paths[b][-2:])
            _, q1, q2 = tpo.joint_sample_path(knots, cps.reshape(-1, D), 0.0, delta[b], N)
            return tpo.joint_constraint_setup(q1, q2, vmax[b], amax[b], 0.8)

        want = oracle_windows(tpo, rows_of, B, delta * (N - 1))
        summary = plan_once(ps, B)
        compare(summary, ps.check_results(), want, False)


def test_cartesian_window_records_equal_the_oracle(env):
    B, D, N, W = 16, 14, 129, 6
    eng, tpo = env["eng"], env["tpo"]
    batch = env["syn"].make_cartesian_batch(B, D, N, W)
    want = oracle_windows(tpo, lambda b: cr.cartesian_batch_rows(tpo, batch, b), B, batch["delta"] * (N - 1))
    assert sum(rc == 0 and count > 0 for rc, count, _, _ in want) >= 1
    offsets = np.arange(B + 1, dtype=np.int32) * N
    with eng.PlannerSet(env["E"], B, D, N, cartesian=True) as ps:
        ps.set_checking(True)
        ps.set_ik_tables(batch["ik_positions"].reshape(-1, D), batch["jacobians"].reshape(-1, 6, D), offsets,
                         batch["delta"] * (N - 1), batch["vmax"], batch["amax"], batch["vtrans"], batch["vrot"],
                         batch["delta"])
        summary = plan_once(ps, B)
        compare(summary, ps.check_results(), want, True)


def test_cartesian_records_do_not_depend_on_discarded_rows(env):
    """first_row != 0: windows of 65 samples on tables of 200 rows whose path ends at row 135 (a window
    needs its 65 rows resident, so the table reaches 64 rows past the end of the path). After two
    Plans one set discards the rows below its planners' safe floors, its twin keeps them; the replan's
    windows then read slots first - first_row in the one and first in the other and must give the same
    records (a single window cannot start above row 0, so the oracle comparison above cannot reach
    this case)."""
    B, D, M, W, N = 16, 14, 200, 6, 65
    eng = env["eng"]
    batch = env["syn"].make_cartesian_batch(B, D, M, W)
    offsets = np.arange(B + 1, dtype=np.int32) * M
    ms = 1_000_000
    records, first_rows = [], []
    for discard in (True, False):
        with eng.PlannerSet(env["E"], B, D, N, cartesian=True, time_step_ns=ms) as ps:
            ps.set_checking(True)
            ps.set_ik_tables(batch["ik_positions"].reshape(-1, D), batch["jacobians"].reshape(-1, 6, D), offsets,
                             batch["delta"] * (M - N), batch["vmax"], batch["amax"], batch["vtrans"], batch["vrot"],
                             batch["delta"])
            # the floor below which rows may go is the row of the last Plan's start: two plans first
            for start in (0, 500):
                early = ps.plan(np.full(B, start * ms, dtype=np.int64), np.full(B, 800 * ms, dtype=np.int64))
                assert (early["status"].numpy() == 0).all()
            if discard:
                ps.discard_ik_rows()
            first_rows.append([ps.ik_table_info(b)[0] for b in range(B)])
            second = ps.plan(np.full(B, 700 * ms, dtype=np.int64), np.full(B, HORIZON_NS, dtype=np.int64))
            assert (second["status"].numpy() == 0).all() and (second["windows"].numpy() >= 1).all()
            records.append(ps.check_results())
            print("discard", discard, "first rows", first_rows[-1], "windows", records[-1]["windows"].tolist(),
                  "violations", records[-1]["violations"].tolist())
    assert max(first_rows[0]) > 0 and max(first_rows[1]) == 0
    assert records[0].tobytes() == records[1].tobytes()
    assert (records[0]["windows"] >= 1).all() and (records[0]["violations"] > 0).any()

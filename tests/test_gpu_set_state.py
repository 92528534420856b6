"""Planner state records on the GPU (tpamd_planner_set_export_state_* / import_state_* /
copy_planners, engine.PlannerSet.export_state / import_state / copy_from), joint sets.

Twin equality: set A runs an eight-planner scenario up to a hand-over point at which it holds one
planner of every class (no path; a new, unplanned path; mid-motion after three replans; a
trajectory whose front was erased; at its target; a modified path after switch_paths; after a
retarget; a history of exactly 64 samples and one of 65 or more; an uploaded 3-point spline) and
continues. Set B, created with other capacities and one planner more, takes A's planners by
export + import in reversed id order and runs the same continuation (three plans, a switch, a
retarget, a plan, stop parameters, setpoints at ticks, stopping trajectories, the trajectories)
on the permuted ids: every output, every summary and the final records must be bit-equal. Set C
does the same through copy_planners. A rotation of a set onto itself is held against the host-side
permutation of the exports.

A history holds offset + N samples after a window that connected at sample `offset`, so "exactly
64" is reachable at N = 33 (offset 31, which the scenario steers for) and not at N = 65, where the
class is "65 or more" alone (set_state_cases.check_classes).

Canonical form: two exports are identical, export(import(r)) == r, the host and the device export
agree, every pad byte is zero (parsed by an independent restatement of the format). Refusals use
well-formed records only; malformed ones are the CPU test's (tests/test_state_record_cpu.py)."""
import numpy as np
import pytest

import set_state_cases as cases

pytestmark = pytest.mark.gpu

SHAPES = [(D, N, method) for D in (1, 7, 16) for N in (33, 65) for method in (0, 1)]


@pytest.fixture(scope="module", autouse=True)
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")


@pytest.mark.parametrize("D,N,method", SHAPES)
def test_scenario_holds_every_class(D, N, method):
    res = cases.run_case(D, N, method)
    cases.check_classes(res["info"], N)
    assert res["capacity_before"][0] == (2 * N, 48)          # B starts smaller than what it takes
    assert res["capacity_after"][0][0] >= int(res["info"]["history_count"].max())
    assert res["capacity_after"][0][1] >= int(res["info"]["trajectory_count"].max())


@pytest.mark.parametrize("D,N,method", SHAPES)
def test_canonical_form(D, N, method):
    res = cases.run_case(D, N, method)
    recs = res["records"]
    assert (res["status_device"] == 0).all()
    assert [len(r) for r in recs] == res["info"]["bytes"].tolist()
    assert recs == res["records_again"], "exporting twice gives identical bytes"
    rc, status, host = res["records_host"]
    assert rc == 0 and (status == 0).all() and host == recs, "the host and the device export agree"
    assert res["records_B"] == recs, "export(import(blob)) == blob, through a set of other capacities"
    assert res["records_C"] == recs, "copy_planners moves the same bytes"
    for j, r in enumerate(recs):
        p = cases.parse_record(r)
        h, i = p["head"], res["info"][j]
        assert p["pad_ok"], j
        assert (h["kind"], h["num_dofs"], h["num_samples"], h["sampling_method"], h["time_step_ns"]) == \
            (0, D, N, method, cases.STEP_NS)
        assert np.float64(0.8).view(np.uint64) == h["constraint_safety_bits"]
        assert np.float64(1e-2).view(np.uint64) == h["max_initial_velocity_error_bits"]
        for name in ("num_points", "history_count", "trajectory_count", "has_path", "path_state", "initial_plan",
                     "planned_to_end", "target_reached"):
            assert h[name] == i[name], (j, name)
        assert h["table_rows"] == 0 and h["first_row"] == 0 and h["reserved"] == 0
        if h["trajectory_count"]:
            assert (np.diff(p["t_time"]) > 0).all()
    # the trajectory of the planner whose front was erased is stored from its first live sample
    last = res["scenario"][-1]
    erased = cases.parse_record(recs[cases.ERASED])
    assert erased["head"]["trajectory_count"] == int(last["num_samples"][cases.ERASED])
    assert erased["t_time"][0] >= int(last["start_time_ns"][cases.ERASED]) / 1e9 - cases.STEP_NS / 1e9
    assert int(last["start_time_ns"][cases.ERASED]) > cases.T0 + 100 * cases.MS


@pytest.mark.parametrize("D,N,method", SHAPES)
def test_import_summaries(D, N, method):
    res = cases.run_case(D, N, method)
    last = res["scenario"][-1]
    rs, rsum = res["import_R"]
    assert (rs == 0).all(), rs
    for got in (res["import_B"], res["copy_C"]):
        assert (got["status"].numpy() == 0).all(), got["status"]
        for name in ("end_time_ns", "final_decel_start_ns", "start_time_ns", "num_samples", "target_reached",
                     "planned_to_end", "history_count"):
            assert got[name].numpy().tolist() == last[name].numpy().tolist(), name
            assert rsum[name].tolist() == last[name].numpy().tolist(), name
        assert got["path_state"].numpy().tolist() == res["info"]["path_state"].tolist()
        assert (got["windows"].numpy() == 0).all()


@pytest.mark.parametrize("twin", ["B", "C"])
@pytest.mark.parametrize("D,N,method", SHAPES)
def test_twin_continues_bit_equal(D, N, method, twin):
    res = cases.run_case(D, N, method)
    a, b = res["A"], res[twin]
    assert a.keys() == b.keys() and len(a) > 60
    for key in a:
        assert cases.same(a[key], b[key]), (twin, key)
    # the continuation did something: the movers planned, the switch and the retarget took
    for k in range(3):
        st = a["plan%d.status" % k]
        assert (st[[cases.MID_MOTION, cases.SWITCHED, cases.RETARGETED, cases.NEW_PATH]] == 0).all(), (k, st)
    assert (a["plan3.status"] == 0).sum() >= 4, a["plan3.status"]      # on the switched and retargeted paths
    assert (a["switch.status"] == 0).all() and (a["retarget.status"] == 0).all()
    assert a["trajectories.offsets"][-1] > 8 and (a["ticks.status"] == 0).sum() > 12
    assert a["final_records"] != res["records"]


@pytest.mark.parametrize("D,N,method", SHAPES)
def test_rotation_in_place(D, N, method):
    res = cases.run_case(D, N, method)
    got = res["rotate_R"]
    assert (got["status"].numpy() == 0).all()
    # planner (j + 3) % 8 now holds what planner j held: exported in the order of the rotation
    assert res["records_R"] == res["records"]


def _small_set(eng, **over):
    kw = dict(num_points=16, time_step_ns=cases.STEP_NS, sampling_method=0)
    D, N = over.pop("D", 7), over.pop("N", 33)
    kw.update(over)
    return eng.PlannerSet(cases.engine(), cases.B, D, N, **kw)


def test_refusals():
    import torch
    torch, eng = cases.env()
    res = cases.run_case(7, 33, 0)
    recs = res["records"]
    blob, off = cases.pack(recs)
    # a set of another shape refuses the whole call and keeps its state
    for over in (dict(D=6), dict(N=65), dict(sampling_method=1), dict(time_step_ns=2 * cases.STEP_NS),
                 dict(constraint_safety=0.75), dict(max_initial_velocity_error=2e-2)):
        with _small_set(eng, **over) as ps:
            before = cases.split(*ps.export_state())
            with pytest.raises(eng.TpamdError):
                ps.import_state(blob, off)
            with pytest.raises(eng.TpamdError):
                ps.import_state(blob[:off[1]], off[:2], ids=[5])
            assert cases.split(*ps.export_state()) == before, over
            # the device entry refuses per planner
            got = ps.import_state(torch.from_numpy(blob).cuda(), off)
            torch.cuda.synchronize()
            assert (got["status"].cpu().numpy() == cases.INVALID_ARGUMENT).all(), over
            assert cases.split(*ps.export_state()) == before, over
    with _small_set(eng) as ps:
        before = cases.split(*ps.export_state())
        # repeated ids, ids outside the set, offsets that are no multiples of 16
        for ids in ([0, 1, 2, 3, 4, 5, 6, 0], [0, 1, 2, 3, 4, 5, 6, 8], [-1, 1, 2, 3, 4, 5, 6, 7]):
            with pytest.raises(eng.TpamdError):
                ps.import_state(blob, off, ids=ids)
        with pytest.raises(eng.TpamdError):
            ps.import_state(np.concatenate([np.zeros(8, np.uint8), blob]), off + 8)
        with pytest.raises(eng.TpamdError):
            ps.copy_from(ps, src_ids=[0, 1], dst_ids=[2, 2])
        with pytest.raises(eng.TpamdError):                      # more planners than the set has
            ps.export_state(ids=list(range(cases.B)) + [0])
        bound = ps.state_bytes_bound
        many = torch.zeros(16, dtype=torch.uint8, device="cuda")
        assert ps._lib.tpamd_planner_set_export_state_device(ps._handle(), cases.B + 1, None, many.data_ptr(),
                                                             many.data_ptr(), many.data_ptr(), None) == -1
        assert cases.split(*ps.export_state()) == before
        # count == 0 returns 0 and touches nothing
        none = np.zeros(0, dtype=np.int32)
        lib, h = ps._lib, ps._handle()
        assert lib.tpamd_planner_set_export_state_host(h, 0, None, None, None, None) == 0
        assert lib.tpamd_planner_set_export_state_device(h, 0, None, None, None, None, None) == 0
        assert lib.tpamd_planner_set_import_state_host(h, 0, None, None, None, None, None) == 0
        assert lib.tpamd_planner_set_import_state_device(h, 0, None, None, None, None, None, None) == 0
        assert lib.tpamd_planner_set_copy_planners(h, None, h, None, 0, None, None) == 0
        assert lib.tpamd_planner_set_state_info(h, 0, None, None) == 0
        assert ps.state_info(none).shape == (0,)
        assert cases.split(*ps.export_state()) == before
        assert ps.state_bytes_bound >= max(len(r) for r in before) and ps.state_bytes_bound % 16 == 0

    # the device import allocates nothing: without reserved room a planner is refused and keeps its
    # state, the others are taken
    info = res["info"]
    with eng.PlannerSet(cases.engine(), cases.B, 7, 33, num_points=16, time_step_ns=cases.STEP_NS, history_capacity=66,
                        trajectory_capacity=8) as ps:
        hist, traj = ps.capacity()
        fits = (info["history_count"] <= hist) & (info["trajectory_count"] <= traj) & (info["num_points"] <= 16)
        assert fits.any() and not fits.all()
        before = cases.split(*ps.export_state())
        got = ps.import_state(torch.from_numpy(blob).cuda(), off)
        torch.cuda.synchronize()
        assert got["status"].cpu().numpy().tolist() == [0 if f else cases.RESOURCE_EXHAUSTED for f in fits]
        assert ps.capacity() == (hist, traj)
        after = cases.split(*ps.export_state())
        for j in range(cases.B):
            assert after[j] == (recs[j] if fits[j] else before[j]), j

    # a slot that is too small: RESOURCE_EXHAUSTED for that planner (its header alone is written),
    # the rest exported
    with _small_set(eng) as ps:
        assert (ps.import_state(blob, off)["status"].numpy() == 0).all()
        sizes = np.array([len(r) for r in recs])
        slots = sizes.copy()
        slots[cases.MID_MOTION] -= 16
        slots[cases.AT_TARGET] = 192
        slots[cases.NO_PATH] = 64
        tight = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
        out = torch.full((int(tight[-1]),), 0xEE, dtype=torch.uint8, device="cuda")
        got, _ = ps.export_state(out=out, offsets=tight)
        torch.cuda.synchronize()
        status = ps.last_export_status.cpu().numpy()
        small = [cases.MID_MOTION, cases.AT_TARGET, cases.NO_PATH]
        assert status.tolist() == [cases.RESOURCE_EXHAUSTED if j in small else 0 for j in range(cases.B)]
        parts = cases.split(got, tight)
        for j in range(cases.B):
            if j not in small:
                assert parts[j] == recs[j], j
        for j in (cases.MID_MOTION, cases.AT_TARGET):
            assert parts[j][:192] == recs[j][:192] and set(parts[j][192:]) <= {0xEE}, j
        assert set(parts[cases.NO_PATH]) == {0xEE}


def test_host_export_leaves_uncovered_bytes_alone():
    """Bytes of the blob between the records, and behind the header of a slot that is too small,
    keep what they held, in the host entry as in the device entry."""
    torch, eng = cases.env()
    res = cases.run_case(7, 33, 0)
    recs = res["records"]
    blob, off = cases.pack(recs)
    with _small_set(eng) as ps:
        assert (ps.import_state(blob, off)["status"].numpy() == 0).all()
        slots = np.array([len(r) + 32 for r in recs])
        slots[cases.MID_MOTION] = 192 + 48
        wide = np.concatenate([[0], np.cumsum(slots)]).astype(np.int64)
        host = np.full(int(wide[-1]), 0xCD, dtype=np.uint8)
        status = np.full(cases.B, -1, dtype=np.int32)
        assert ps._lib.tpamd_planner_set_export_state_host(ps._handle(), cases.B, None, host.ctypes.data,
                                                           wide.ctypes.data, status.ctypes.data) == 0
        dev = torch.full((int(wide[-1]),), 0xCD, dtype=torch.uint8, device="cuda")
        ps.export_state(out=dev, offsets=wide)
        torch.cuda.synchronize()
        assert host.tobytes() == dev.cpu().numpy().tobytes()
        assert status.tolist() == ps.last_export_status.cpu().tolist()
        assert status.tolist() == [cases.RESOURCE_EXHAUSTED if j == cases.MID_MOTION else 0 for j in range(cases.B)]
        for j, part in enumerate(cases.split(host, wide)):
            if j == cases.MID_MOTION:
                assert part[:192] == recs[j][:192] and set(part[192:]) == {0xCD}
            else:
                assert part[:len(recs[j])] == recs[j] and set(part[len(recs[j]):]) == {0xCD}, j


def test_import_clears_the_check_record():
    """With checking on, a planner that imports OK reports "nothing checked" until its next Plan: the
    windows checked in its slot were another planner's. A planner that is refused keeps its record."""
    torch, eng = cases.env()
    res = cases.run_case(7, 33, 0)
    recs = res["records"]
    blob, off = cases.pack(recs)
    inp = res["inp"]

    def nothing(r):
        return (r["windows"] == 0 and r["violations"] == -1 and r["last_window_violations"] == -1 and
                r["worst_window"] == -1 and r["first_sample"] == -1 and np.isnan(r["worst_excess"]) and
                np.isnan(r["worst_parameter"]))

    def planned_set():
        ps = _small_set(eng)
        ps.set_checking(True)
        cases._set_waypoints(ps, inp, [cases.MID_MOTION, cases.SWITCHED, cases.RETARGETED, cases.ERASED], 33)
        s = ps.plan(cases.T0, 500 * cases.MS)
        assert (s["status"].numpy()[[cases.MID_MOTION, cases.SWITCHED, cases.RETARGETED, cases.ERASED]] == 0).all()
        return ps

    checked = [cases.MID_MOTION, cases.SWITCHED, cases.RETARGETED, cases.ERASED]
    for route in ("host", "device", "rotate"):
        with planned_set() as ps:
            before = ps.check_results()
            assert all(before["windows"][j] > 0 for j in checked) and nothing(before[cases.NO_PATH])
            if route == "host":
                # planners 2 and 5 take records; the others are not listed
                got = ps.import_state(*cases.pack([recs[cases.AT_TARGET], recs[cases.MID_MOTION]]),
                                      ids=[cases.MID_MOTION, cases.SWITCHED])
                assert got["status"].tolist() == [0, 0]
                cleared, kept = [cases.MID_MOTION, cases.SWITCHED], [cases.RETARGETED, cases.ERASED]
            elif route == "device":
                # without reserved trajectory room only the small records are taken
                b2, o2 = cases.pack([recs[cases.NO_PATH], recs[cases.MID_MOTION]])
                hist, traj = ps.capacity()
                assert res["info"]["history_count"][cases.MID_MOTION] <= hist
                fits = res["info"]["trajectory_count"][cases.MID_MOTION] <= traj
                got = ps.import_state(torch.from_numpy(b2).cuda(), o2, ids=[cases.RETARGETED, cases.ERASED])
                torch.cuda.synchronize()
                assert got["status"].cpu().tolist() == [0, 0 if fits else cases.RESOURCE_EXHAUSTED]
                cleared = [cases.RETARGETED] + ([cases.ERASED] if fits else [])
                kept = [cases.MID_MOTION, cases.SWITCHED] + ([] if fits else [cases.ERASED])
            else:
                ids = np.arange(cases.B, dtype=np.int32)
                got = ps.copy_from(ps, src_ids=ids, dst_ids=(ids + 3) % cases.B)
                assert (got["status"].numpy() == 0).all()
                cleared, kept = list(range(cases.B)), []
            after = ps.check_results()
            for j in cleared:
                assert nothing(after[j]), (route, j, after[j])
            for j in kept:
                assert after[j].tobytes() == before[j].tobytes(), (route, j)
            # the next Plan checks the planner's own windows again
            # (planner SWITCHED holds the mid-motion record: planned 1000 ms ahead of an earlier start and
            # not to its path's end, so a Plan 1000 ms ahead of a later start has to solve a window)
            if route == "host":
                s = ps.plan(int(res["scenario"][-1]["start_time_ns"][cases.MID_MOTION]) + 20 * cases.MS, 1000 * cases.MS)
                assert int(s["status"][cases.SWITCHED]) == 0 and int(s["windows"][cases.SWITCHED]) > 0, s
                assert ps.check_results()[cases.SWITCHED]["windows"] == int(s["windows"][cases.SWITCHED])
    # with checking off nothing is touched and every record reads "nothing checked"
    with _small_set(eng) as ps:
        assert (ps.import_state(blob, off)["status"].numpy() == 0).all()
        assert all(nothing(r) for r in ps.check_results())

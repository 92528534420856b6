"""What the planner-state tests share (tests/test_gpu_set_state*.py): an independent restatement of
the record format of csrc/tpamd_state.h (parse_record: header fields, sections, pad bytes), the
eight-planner scenario that brings a joint set to the hand-over point with one planner of every
class that matters to a hand-over, the continuation both twins run after it, and a per-shape cache so that the
scenario, the hand-over and the continuation run once per shape however many tests look at them."""
import functools
import importlib

import numpy as np

from conftest import PKG_NAME

MS = 1_000_000
T0 = 1000 * MS
STEP_NS = 4 * MS
B = 8
(NO_PATH, NEW_PATH, MID_MOTION, ERASED, AT_TARGET, SWITCHED, RETARGETED, SPLINE) = range(8)
PLAN_OK, FAILED_PRECONDITION, INVALID_ARGUMENT, RESOURCE_EXHAUSTED = 0, 1, 3, 8

HEADER_DTYPE = np.dtype([
    ("magic", "<u4"), ("version", "<u4"), ("bytes", "<u8"),
    ("kind", "<i4"), ("num_dofs", "<i4"), ("num_samples", "<i4"), ("sampling_method", "<i4"),
    ("time_step_ns", "<i8"), ("constraint_safety_bits", "<u8"), ("max_initial_velocity_error_bits", "<u8"),
    ("num_points", "<i4"), ("history_count", "<i4"), ("trajectory_count", "<i4"), ("table_rows", "<i4"),
    ("first_row", "<i4"), ("has_path", "<i4"), ("path_state", "<i4"),
    ("initial_plan", "<i4"), ("planned_to_end", "<i4"), ("target_reached", "<i4"), ("w_lei", "<i4"),
    ("reserved", "<i4"),
    ("path_horizon", "<f8"), ("path_start", "<f8"), ("path_start_velocity", "<f8"), ("path_time_start", "<f8"),
    ("start_time_ns", "<i8"), ("end_time_ns", "<i8"), ("final_decel_start_ns", "<i8"),
    ("delta", "<f8"), ("path_end", "<f8"), ("vtrans", "<f8"), ("vrot", "<f8")])
assert HEADER_DTYPE.itemsize == 192
MAGIC = 0x54535054

SECTIONS = ("knots", "control_points", "vmax", "amax", "initial_velocity",
            "h_time", "h_s", "h_sd", "h_sdd", "h_q", "h_qd", "h_qdd", "w_time",
            "t_time", "t_s", "t_sd", "t_sdd", "t_q", "t_qd", "t_qdd", "table_q", "table_J")


def section_words(h):
    D, N = int(h["num_dofs"]), int(h["num_samples"])
    P, hc, tc = int(h["num_points"]), int(h["history_count"]), int(h["trajectory_count"])
    live = int(h["table_rows"]) - int(h["first_row"])
    lim = D if h["has_path"] else 0
    return [P + 3 if P else 0, P * D, lim, lim, lim, hc, hc, hc, hc, hc * D, hc * D, hc * D,
            N if h["initial_plan"] else 0, tc, tc, tc, tc, tc * D, tc * D, tc * D, live * D, live * 6 * D]


def parse_record(raw):
    """One record (bytes or uint8 array, exactly the record): dict of the header record `head`,
    the sections as float64 arrays under their names, and `pad_ok` (every byte outside the header
    and the sections is zero and every section starts on a 16-byte boundary)."""
    raw = np.frombuffer(bytes(raw), dtype=np.uint8)
    head = raw[:192].view(HEADER_DTYPE)[0]
    assert head["magic"] == MAGIC and head["version"] == 1 and head["bytes"] == raw.size, head
    out = dict(head=head)
    covered = np.zeros(raw.size, dtype=bool)
    covered[:192] = True
    at = 192
    for name, words in zip(SECTIONS, section_words(head)):
        assert at % 16 == 0
        out[name] = raw[at:at + 8 * words].view("<f8").copy()
        covered[at:at + 8 * words] = True
        at += 8 * (words + (words & 1))
    assert at == raw.size, (at, raw.size)
    out["pad_ok"] = bool((raw[~covered] == 0).all())
    return out


def split(blob, offsets):
    """The records of a blob as a list of bytes objects."""
    b = blob.detach().cpu().numpy() if hasattr(blob, "detach") else np.asarray(blob)
    o = np.asarray(offsets.cpu() if hasattr(offsets, "cpu") else offsets).astype(np.int64)
    return [b[o[k]:o[k + 1]].tobytes() for k in range(o.size - 1)]


def pack(records):
    """(blob uint8 numpy, offsets int64) of a list of records."""
    off = np.concatenate([[0], np.cumsum([len(r) for r in records])]).astype(np.int64)
    return np.frombuffer(b"".join(records), dtype=np.uint8).copy(), off


def env():
    import torch
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return torch, eng


@functools.lru_cache(maxsize=None)
def engine():
    _, eng = env()
    return eng.Engine(0)


def _delta(N):
    return 0.64 / (N - 1)          # every window covers 0.64 of path parameter


def make_inputs(D, N, method):
    rng = np.random.default_rng(7000 + 100 * D + N + method)
    sign = np.where(rng.random(D) < 0.5, -1.0, 1.0)
    unit = sign / np.sqrt(D)
    wps = {
        NEW_PATH: rng.uniform(-2, 2, size=(2, D)),
        MID_MOTION: rng.uniform(-2, 2, size=(6, D)),
        ERASED: np.stack([0.3 * unit, 0.9 * unit]),                 # 0.6 long: inside one window
        AT_TARGET: np.stack([-0.25 * unit, 0.3 * unit]),
        SWITCHED: rng.uniform(-2, 2, size=(6, D)),
        RETARGETED: np.stack([-2.0 * unit, 2.0 * unit]),
    }
    spline = np.stack([-1.8 * unit, 0.4 * unit * np.where(np.arange(D) % 2, -1.0, 1.0), 1.8 * unit])
    length = float(np.linalg.norm(spline[1] - spline[0]) + np.linalg.norm(spline[2] - spline[1]))
    return dict(rng=rng, wps=wps, spline=spline, spline_knots=np.array([0, 0, 0, length, length, length], dtype=np.float64),
                vmax=rng.uniform(1.0, 2.0, size=(B, D)), amax=rng.uniform(2.0, 4.0, size=(B, D)),
                switch_wps=rng.uniform(-2, 2, size=(3, D)), retarget_wps=rng.uniform(-2, 2, size=(2, D)),
                later_switch=rng.uniform(-2, 2, size=(2, 3, D)), later_retarget=rng.uniform(-2, 2, size=(2, 2, D)))


def _set_waypoints(ps, inp, who, N):
    w = [inp["wps"][b] for b in who]
    off = np.concatenate([[0], np.cumsum([len(x) for x in w])]).astype(np.int32)
    ids = np.array(who, dtype=np.int32)
    st, _ = ps.set_waypoints(np.concatenate(w), off, inp["vmax"][ids], inp["amax"][ids], _delta(N), ids=ids)
    assert (st.numpy() == 0).all(), st


def run_scenario(ps, inp, D, N):
    """Drives set `ps` (B planners) to the hand-over point. Returns the summaries of its plans."""
    _set_waypoints(ps, inp, [MID_MOTION, ERASED, AT_TARGET, SWITCHED, RETARGETED], N)
    ps.set_paths(inp["spline_knots"], inp["spline"], [3], inp["vmax"][[SPLINE]], inp["amax"][[SPLINE]], _delta(N),
                 ids=[SPLINE])
    summaries = []
    start = np.full(B, T0, dtype=np.int64)
    horizon = np.full(B, 1000 * MS, dtype=np.int64)
    horizon[[ERASED, AT_TARGET]] = 5000 * MS          # the whole short path at once
    horizon[SPLINE] = MS                              # exactly one window
    s = ps.plan(start, horizon)
    summaries.append(s)
    movers = [MID_MOTION, ERASED, AT_TARGET, SWITCHED, RETARGETED, SPLINE]
    assert (s["status"].numpy()[movers] == 0).all(), s["status"]
    assert s["status"].numpy()[[NO_PATH, NEW_PATH]].tolist() == [FAILED_PRECONDITION] * 2
    end_target = int(s["end_time_ns"][AT_TARGET])
    # a tenth of its motion per step: well before the final deceleration starts, past several samples
    erase_step = (int(s["end_time_ns"][ERASED]) - T0) // (10 * MS) * MS
    # the spline planner's second window connects at history sample N - 2 at N = 33: 31 + 33 = 64
    blob, off = ps.export_state(ids=[SPLINE])
    rec = parse_record(split(blob, off)[0])
    assert rec["head"]["history_count"] == N
    ht = rec["h_time"]
    spline_start = int((ht[N - 2] + ht[N - 1]) / 2 * 1e9) if N == 33 else T0 + 50 * MS
    for k in (1, 2, 3):
        start = np.full(B, T0 + 50 * k * MS, dtype=np.int64)
        horizon = np.full(B, 1000 * MS, dtype=np.int64)
        start[ERASED] = T0 + k * erase_step
        horizon[ERASED] = STEP_NS                     # planned far enough: only the front is erased
        horizon[AT_TARGET] = 20 * MS
        if k == 3:
            start[AT_TARGET] = end_target - 2 * STEP_NS
        start[SPLINE] = spline_start
        horizon[SPLINE] = MS
        s = ps.plan(start, horizon)
        summaries.append(s)
        assert (s["status"].numpy()[movers] == 0).all(), (k, s["status"])
    t = np.array([T0 + 250 * MS], dtype=np.int64)
    got = ps.switch_paths(t, inp["switch_wps"], np.array([0, 3], dtype=np.int32), ids=[SWITCHED])
    assert got["status"].tolist() == [0], got
    got = ps.retarget(t, inp["retarget_wps"], np.array([0, 2], dtype=np.int32), inp["vmax"][[RETARGETED]],
                      inp["amax"][[RETARGETED]], _delta(N), ids=[RETARGETED])
    assert got["status"].tolist() == [0], got
    _set_waypoints(ps, inp, [NEW_PATH], N)
    return summaries


def check_classes(info, N):
    """Every planner class is present at the hand-over point (info: state_info of planners 0..7)."""
    i = info
    assert i["has_path"][NO_PATH] == 0 and i["history_count"][NO_PATH] == 0, "(a) no path"
    assert i["has_path"][NEW_PATH] == 1 and i["path_state"][NEW_PATH] == 1 and i["initial_plan"][NEW_PATH] == 0, "(b)"
    m = MID_MOTION
    assert (i["initial_plan"][m] == 1 and i["planned_to_end"][m] == 0 and i["target_reached"][m] == 0 and
            i["path_state"][m] == 3 and i["trajectory_count"][m] > 1), "(c) mid-motion"
    assert i["trajectory_first"][ERASED] > 0 and i["trajectory_count"][ERASED] > 0, ("(d) front erased", i[ERASED])
    assert i["target_reached"][AT_TARGET] == 1 and i["planned_to_end"][AT_TARGET] == 1, ("(e) at its target", i[AT_TARGET])
    assert i["path_state"][SWITCHED] == 2 and i["initial_plan"][SWITCHED] == 1, "(f) modified path"
    assert i["path_state"][RETARGETED] == 1 and i["initial_plan"][RETARGETED] == 1, "(g) retargeted"
    assert i["num_points"][SPLINE] == 3, "the uploaded spline with 3 control points"
    # (h) the history grows by whole windows from the sample a replan connects to, count = offset + N:
    # exactly 64 exists at N = 33 (offset 31) and cannot at N = 65, where every planned history has
    # 65 or more
    if N == 33:
        assert i["history_count"][SPLINE] == 64, ("(h) a history of exactly 64", i[SPLINE])
    assert (i["history_count"] >= 65).any(), "(h) a history of 65 or more"
    assert (i["bytes"] % 16 == 0).all() and (i["status"] == 0).all()


def next_start(summary, target):
    """GetNextPlanStartTime(target) per planner from its last summary: min(end, max(target, start));
    a planner that has not planned starts at target."""
    s, e = np.asarray(summary["start_time_ns"]), np.asarray(summary["end_time_ns"])
    out = np.minimum(e, np.maximum(target, s))
    return np.where(e == 0, target, out).astype(np.int64)


def continuation(ps, inp, D, N, ids, last):
    """What both twins do after the hand-over. ids[j]: the planner of `ps` that holds scenario planner
    j; last: the (start_time_ns, end_time_ns) of the scenario planners at the hand-over. Returns
    everything the calls gave back, per scenario planner, as numpy arrays."""
    import torch
    ids = np.asarray(ids, dtype=np.int32)
    nB = ps.B
    out = {}
    state = dict(start_time_ns=np.asarray(last["start_time_ns"]).copy(), end_time_ns=np.asarray(last["end_time_ns"]).copy())

    def plan(tag, target):
        st = next_start(state, target)
        start = np.full(nB, target, dtype=np.int64)
        start[ids] = st
        s = ps.plan(start, 1000 * MS)
        for name, v in s.items():
            out["%s.%s" % (tag, name)] = v.numpy()[ids]
        ok = s["status"].numpy()[ids] == 0
        for name in ("start_time_ns", "end_time_ns"):
            state[name] = np.where(ok, s[name].numpy()[ids], state[name])

    for k in range(3):
        plan("plan%d" % k, T0 + (300 + 50 * k) * MS)
    who = [MID_MOTION, SWITCHED]
    t = state["start_time_ns"][who] + 60 * MS
    got = ps.switch_paths(t, inp["later_switch"].reshape(-1, D), np.array([0, 3, 6], dtype=np.int32), ids=ids[who])
    out.update({"switch." + k: v.numpy() for k, v in got.items()})
    who = [RETARGETED, SPLINE]
    t = state["start_time_ns"][who] + 40 * MS
    got = ps.retarget(t, inp["later_retarget"].reshape(-1, D), np.array([0, 2, 4], dtype=np.int32), inp["vmax"][who],
                      inp["amax"][who], _delta(N), ids=ids[who])
    out.update({"retarget." + k: v.numpy() for k, v in got.items()})
    plan("plan3", T0 + 480 * MS)
    t = state["start_time_ns"] + 24 * MS
    got = ps.stop_parameters(t, ids=ids)
    out.update({"stop_parameters." + k: v.numpy() for k, v in got.items()})
    got = ps.sample_at_ticks(state["start_time_ns"], STEP_NS, 12, ids=ids, host=True)
    out.update({"ticks." + k: v.numpy() for k, v in got.items()})
    dev = torch.device("cuda", ps.device)
    got = ps.stop_trajectories(torch.from_numpy(t).to(dev), torch.from_numpy(inp["amax"]).to(dev), STEP_NS / 1e9,
                               ids=torch.from_numpy(ids).to(dev))
    torch.cuda.synchronize()
    out.update({"stop_trajectories." + k: v.cpu().numpy() for k, v in got.items()})
    got = ps.download_trajectories(ids=ids)
    torch.cuda.synchronize()
    out.update({"trajectories." + k: v.cpu().numpy() for k, v in got.items() if not k.startswith("_")})
    blob, off = ps.export_state(ids=ids)
    torch.cuda.synchronize()
    out["final_records"] = split(blob, off)
    return out


def same(a, b):
    if isinstance(a, list):
        return a == b
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def run_case(D, N, method):
    """The whole experiment at one shape, once: set A runs the scenario; B (other capacities, one
    planner more) takes A's planners by export + import in reversed order, C by copy_planners, R
    (A's configuration) takes them in place and is rotated onto itself; A, B and C continue."""
    import torch
    torch_, eng = env()
    E = engine()
    inp = make_inputs(D, N, method)
    kw = dict(time_step_ns=STEP_NS, sampling_method=method)
    res = dict(inp=inp)
    A = eng.PlannerSet(E, B, D, N, num_points=16, **kw)
    Bs = eng.PlannerSet(E, B + 1, D, N, num_points=4, history_capacity=2 * N, trajectory_capacity=48, **kw)
    Cs = eng.PlannerSet(E, B + 1, D, N, num_points=3, history_capacity=3 * N, trajectory_capacity=16, **kw)
    R = eng.PlannerSet(E, B, D, N, num_points=64, **kw)
    try:
        res["scenario"] = run_scenario(A, inp, D, N)
        res["info"] = A.state_info()
        res["capacity_before"] = (Bs.capacity(), Cs.capacity())
        # the hand-over: every export form
        blob, off = A.export_state()
        torch.cuda.synchronize()
        res["status_device"] = A.last_export_status.cpu().numpy()
        res["records"] = split(blob, off)
        blob2, off2 = A.export_state()
        torch.cuda.synchronize()
        res["records_again"] = split(blob2, off2)
        host_blob = np.full(int(off[-1]), 0xCD, dtype=np.uint8)
        host_status = np.full(B, -1, dtype=np.int32)
        off_np = np.ascontiguousarray(off.numpy())
        rc = A._lib.tpamd_planner_set_export_state_host(A._handle(), B, None, host_blob.ctypes.data,
                                                        off_np.ctypes.data, host_status.ctypes.data)
        res["records_host"] = (rc, host_status, split(host_blob, off))
        # B: reversed ids through export + import (host blob: the set grows)
        rev = np.arange(B, 0, -1).astype(np.int32)             # scenario planner j -> planner B - j of Bs
        res["import_B"] = Bs.import_state(blob.cpu().numpy(), off, ids=rev)
        res["capacity_after"] = (Bs.capacity(),)
        b2, o2 = Bs.export_state(ids=rev)
        torch.cuda.synchronize()
        res["records_B"] = split(b2, o2)
        # C: the same through copy_planners
        res["copy_C"] = Cs.copy_from(A, src_ids=np.arange(B, dtype=np.int32), dst_ids=rev)
        b3, o3 = Cs.export_state(ids=rev)
        torch.cuda.synchronize()
        res["records_C"] = split(b3, o3)
        # R: A's planners in place through the device import, then rotated onto itself
        R.reserve(history=max(int(res["info"]["history_count"].max()), 2 * N),
                  trajectory=int(res["info"]["trajectory_count"].max()))
        got = R.import_state(blob, off)
        torch.cuda.synchronize()
        res["import_R"] = (got["status"].cpu().numpy(), got["summary"].cpu().numpy().view(eng.PLANNER_SUMMARY_DTYPE)[:, 0])
        rot = ((np.arange(B) + 3) % B).astype(np.int32)
        res["rotate_R"] = R.copy_from(R, src_ids=np.arange(B, dtype=np.int32), dst_ids=rot)
        b4, o4 = R.export_state(ids=rot)
        torch.cuda.synchronize()
        res["records_R"] = split(b4, o4)
        last = res["scenario"][-1]
        last = dict(start_time_ns=last["start_time_ns"].numpy(), end_time_ns=last["end_time_ns"].numpy())
        res["A"] = continuation(A, inp, D, N, np.arange(B), last)
        res["B"] = continuation(Bs, inp, D, N, rev, {k: res["import_B"][k].numpy() for k in last})
        res["C"] = continuation(Cs, inp, D, N, rev, {k: res["copy_C"][k].numpy() for k in last})
    finally:
        for s in (A, Bs, Cs, R):
            s.close()
    return res

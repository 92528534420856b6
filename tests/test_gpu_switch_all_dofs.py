"""The path-switch kernel (k_pset_switch) and the waypoint-fit kernel (k_pset_set_waypoints) at
every joint count D = 1..16 through engine.PlannerSet, against tests/switch_reference.py: the
restatement written from the reference's sources (bit for bit) and the exact-arithmetic property
checkers, which share no order of operations with the kernels.

Per D a set of 70 planners (67 listed: two waves, three live lanes in the last; P = 4..19) is
created with num_points = 4, so that the upload and the switch both grow P_cap. One Plan leaves a
resident trajectory. The first switch call gives the generator's stop parameters (every category
of switch_reference.CATEGORIES, a shuffled ids list, switch times on and between samples, one
before and one after a trajectory); the second lets the stop kernel feed the switch. After
the next Plan a third call gives stop parameters again, generated on the splines as they then are,
and is checked through download_path alone: a stop-fed switch early in a trajectory leaves a path a
few samples long, and after one more switch the oracle's Plan was seen not to return on such a
path (D = 1, a path of parameter range 0.028), so no Plan follows the third switch. Planners that
fill their work area stand in front of a planner of the same wave whose switch succeeds. Every status,
point count, stop parameter and downloaded spline must equal the restatement's, failed and
unlisted planners keep their bytes and their path state, and eight planners per D are followed
through the next Plan by the oracle's planner given the restated spline and the restated velocity
at the switch time: the only way the committed initial velocity shows."""
import collections
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
import switch_reference as sw
from test_fastest_stop_cpu import fastest_stop_at_time
from test_switch_reference_cpu import rounds

pytestmark = pytest.mark.gpu

ALL_DOFS = list(range(1, 17))
MS = 1_000_000
B, LISTED, N = sw.NUM_PLANNERS, sw.NUM_LISTED, 64
STEP_NS, START, HORIZON, SWITCH_TICKS = MS, 1000 * MS, 500 * MS, 25
FOLLOWED = ("inside", "past_knot", "before_knot", "first_span", "last_span", "at_umax", "wmax", "negative_t_all_kept")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), tpo=tpo,
                sync=torch.cuda.synchronize)


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a, dtype=np.float64)
    return np.ascontiguousarray(a).tobytes()


def _flat(rows):
    return [x for r in rows for x in r]


def _same_spline(got, knots, points):
    return _bits(got[0]) == _bits(knots) and _bits(got[1].reshape(-1)) == _bits(_flat(points))


def _trajectories(ps, sync):
    traj = ps.download_trajectories()
    sync()
    off = traj["offsets"].cpu().numpy()
    tj = {k: traj[k].cpu().numpy() for k in ("time", "s", "q", "qd", "qdd")}
    return [{k: tj[k][int(off[b]):int(off[b + 1])].tolist() for k in tj} for b in range(len(off) - 1)]


PAIR_SLOTS = (4, 13, 22, 31, 40, 49)     # where (widest planner, neighbour) pairs go: one wave, never its last lane


def _placed_ids(rng, widest, neighbours):
    """The listed planners in a random order, except that up to six planners with the call's
    largest W (they may fill their work area to the last double) stand at PAIR_SLOTS, each directly
    followed, in the same wave, by one of `neighbours` (planners whose switch is to succeed): an
    overrun lands in the scratch of the query behind it and shows in what that query commits.
    The call's last query is never one of the widest. Returns (ids, [(slot, widest, neighbour)])."""
    fill = sorted(widest)[:len(PAIR_SLOTS)]
    near = [b for b in sorted(neighbours) if b not in widest][:len(fill)]
    assert len(near) == len(fill), (fill, near)
    paired = set(fill) | set(near)
    rest = [int(b) for b in rng.permutation(LISTED) if int(b) not in paired]
    tail = next(i for i in range(len(rest) - 1, -1, -1) if rest[i] not in widest)
    rest.append(rest.pop(tail))
    pairs = []
    for slot, f, g in zip(PAIR_SLOTS, fill, near):
        rest[slot:slot] = [f, g]
        pairs.append((slot, f, g))
    ids = np.array(rest, dtype=np.int32)
    assert sorted(ids.tolist()) == list(range(LISTED)) and int(ids[-1]) not in widest
    for slot, f, g in pairs:
        assert ids[slot] == f and ids[slot + 1] == g and slot // 64 == (slot + 1) // 64
    return ids, pairs


def _switch_call(ps, ids, t_ns, wps, keep):
    W = [len(w) for w in wps]
    offsets = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    flat = np.asarray([r for w in wps for r in w], dtype=np.float64).reshape(-1, ps.D)
    got = ps.switch_paths(t_ns, flat, offsets, ids=ids, keep_path_until=keep)
    return {k: v.numpy() for k, v in got.items()}


@pytest.mark.parametrize("D", ALL_DOFS)
def test_switch(env, D):
    eng, E, tpo, sync = env["eng"], env["E"], env["tpo"], env["sync"]
    planners, rows = rounds(D)
    everyone = planners + planners[:B - LISTED]                  # the unlisted planners have paths too
    labels = [p["label"] for p in planners]
    raw = {b for b, l in enumerate(labels) if l == "nonzero_first_knot"}
    followed = [labels.index(l) for l in FOLLOWED]
    before_b, after_b = [b for b, l in enumerate(labels) if l == "inside" and b not in followed][:2]
    state = [(p["knots"], p["points"]) for p in everyone]
    vmax, amax = np.array([p["vmax"] for p in everyone]), np.array([p["amax"] for p in everyone])
    delta = np.array([p["delta"] for p in everyone])
    rng = np.random.default_rng(4242 + D)
    seen = collections.Counter()
    with eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=STEP_NS) as ps:
        ps.set_paths(_flat(s[0] for s in state), _flat(_flat(s[1]) for s in state), [len(s[1]) for s in state],
                     vmax, amax, delta)
        for b in range(B):
            assert _same_spline(ps.download_path(b), *state[b]), (D, b, "upload")
        summary1 = ps.plan(START, HORIZON)
        assert (summary1["status"].numpy() == 0).all(), (D, summary1["status"])
        assert (summary1["num_samples"].numpy() > 2 * SWITCH_TICKS).all(), (D, summary1["num_samples"])
        traj = _trajectories(ps, sync)
        first_traj = list(traj)
        t_follow = START + SWITCH_TICKS * STEP_NS
        velocity = {}                                              # planner -> the restated committed velocity

        def times_for(ids, with_outside, on_grid=True):
            t_ns = np.zeros(len(ids), dtype=np.int64)
            for k, b in enumerate(ids):
                t = traj[b]["time"]
                lo, hi = int(round(t[0] * 1e9)), int(round(t[-1] * 1e9))
                if on_grid and b in followed:
                    t_ns[k] = t_follow
                elif with_outside and b == before_b:
                    t_ns[k] = lo - MS
                elif with_outside and b == after_b:
                    t_ns[k] = hi + MS
                else:
                    j = int(rng.integers(1, len(t) - 1))
                    t_ns[k] = int(round(t[j] * 1e9)) + (STEP_NS // 2 if k % 2 else 0)
            return t_ns

        def verify(name, ids, t_ns, wps, got, keep=None, cases=None):
            changed = set()
            for k, b in enumerate(ids):
                b, where = int(b), (D, name, k, int(b), labels[b])
                r, t_sec = traj[b], float(t_ns[k]) / 1e9
                knots, points = state[b]
                status, stop = sw.OK, None
                if keep is not None:
                    stop = float(keep[k])
                else:                                              # the stop kernel feeds the switch
                    status, stop_s = fastest_stop_at_time(r["time"], r["s"], r["qd"], r["qdd"], amax[b].tolist(), t_sec)[:2]
                    if status == sw.OK:
                        stop = float(stop_s)
                vel = res = None
                if status == sw.OK:
                    status, vel = sw.velocity_at_time(r["time"], r["qd"], t_sec)
                    sw.check_velocity(r["time"], r["qd"], t_sec, status, vel)
                if status == sw.OK:
                    res = sw.switch_to_waypoint_path(knots, points, stop, wps[k])
                    status = res["status"]
                assert int(got["status"][k]) == status, where + (int(got["status"][k]), status)
                if stop is not None:
                    assert _bits(got["stop_parameter"][k]) == _bits(np.float64(stop)), where + ("stop parameter",)
                path = ps.download_path(b)
                if status == sw.OK:
                    assert int(got["num_points"][k]) == len(res["points"]) <= sw.points_bound(len(points), len(wps[k])), where
                    assert _same_spline(path, res["knots"], res["points"]), where + ("spline differs",)
                    if b not in raw:
                        info = sw.check_switch(knots, points, stop, wps[k], path[0].tolist(), path[1].tolist())
                        if cases is not None and cases[b]["label"] == "negative_t_all_kept" and D > 1:
                            assert info["has_proj"] and info["first"] == 0 and info["num_new"] == sw.WMAX + 1, where
                    state[b] = (res["knots"], res["points"])
                    velocity[b] = vel
                    changed.add(b)
                else:
                    assert int(got["num_points"][k]) == len(points), where
                    assert _same_spline(path, knots, points), where + ("a failed switch changed the spline",)
                if cases is not None:
                    if b == before_b or b == after_b:
                        assert status == sw.OUT_OF_RANGE, where
                        seen["time_before" if b == before_b else "time_after"] += 1
                    else:
                        assert sw.reached(cases[b], int(got["status"][k]), len(points), int(got["num_points"][k])), where
                        seen[labels[b]] += 1
                seen[name + "/" + sw.STATUS_NAMES[status]] += 1
            for b in range(LISTED, B):
                assert _same_spline(ps.download_path(b), *state[b]), (D, name, b, "an unlisted planner changed")
            return changed

        def widest_of(lists):
            w = max(len(x) for x in lists)
            return {b for b, x in enumerate(lists) if len(x) == w}

        steady = {b for b, l in enumerate(labels) if l in ("past_knot", "before_knot", "first_span", "last_span", "at_umax")}

        # 1. the generator's stop parameters, every category
        cases = [e["case"] for e in rows[0]]
        assert max(len(c["waypoints"]) for c in cases) == sw.WMAX
        ids, pairs = _placed_ids(rng, widest_of([c["waypoints"] for c in cases]), steady)
        assert {b for b, l in enumerate(labels) if l == "negative_t_all_kept"} <= {f for _, f, _ in pairs}
        t_ns = times_for(ids, True)
        wps = [cases[b]["waypoints"] for b in ids]
        keep = np.array([cases[b]["keep"] for b in ids])
        got = _switch_call(ps, ids, t_ns, wps, keep)
        for slot, f, g in pairs:          # every filling planner has a neighbour in its wave that commits
            assert int(got["status"][slot + 1]) == sw.OK == cases[g]["status"], (D, "neighbour", slot, f, g)
        changed = verify("keep", ids, t_ns, wps, got, keep=keep, cases=cases)
        missing = [k for k, _ in sw.CATEGORIES if not seen[k]] + [k for k in ("time_before", "time_after") if not seen[k]]
        assert missing == [], (D, missing)
        # 2. the stop kernel feeds the switch
        lists = [e["case"]["waypoints"] for e in rows[1]]
        ids, _ = _placed_ids(rng, widest_of(lists), steady)
        t_ns = times_for(ids, False)
        wps = [lists[b] for b in ids]
        changed |= verify("stop", ids, t_ns, wps, _switch_call(ps, ids, t_ns, wps, None))
        assert seen["stop/ok"] >= LISTED // 2, (D, seen)
        # the next Plan: the committed velocity, and the path state of what did not change
        summary2 = ps.plan(t_follow, HORIZON)
        traj2 = _trajectories(ps, sync)
        for b in range(B):
            if b not in changed:
                assert int(summary2["path_state"][b]) == int(summary1["path_state"][b]), (D, b, "path state")
        diverged = 0
        for b in followed:
            p, where = planners[b], (D, b, labels[b], "oracle")
            assert b in changed, where
            o = tpo.Planner(D, N, delta=p["delta"], time_step_ns=STEP_NS, max_planning_iterations=200,
                            max_initial_velocity_error=1e-2)
            o.set_limits(p["vmax"], p["amax"])
            o.set_spline(p["knots"], p["points"], 1)
            assert o.plan(START, HORIZON) == 0 and _bits(o.velocities) == _bits(np.array(first_traj[b]["qd"])), where
            o.set_spline(state[b][0], np.array(state[b][1]), 2)
            o.set_initial_velocity(velocity[b])
            rc = o.plan(t_follow, HORIZON)
            assert int(summary2["status"][b]) == rc, where + (int(summary2["status"][b]), rc)
            if rc == sw.INVALID_ARGUMENT:                          # DESIGN.md "Path switch": a failed first window
                diverged += 1
                continue
            if rc == 0:
                assert int(summary2["num_samples"][b]) == o.num_samples, where
                for k, want in (("time", o.time), ("s", o.path_parameter), ("q", o.positions), ("qd", o.velocities),
                                ("qdd", o.accelerations)):
                    assert _bits(np.array(traj2[b][k])) == _bits(want), where + (k,)
                seen["followed"] += 1
        # all eight are compared bit for bit but for the documented divergence, at most two of them
        assert diverged <= 2 and seen["followed"] + diverged == len(followed) == 8, (D, diverged, seen)
        # 3. a third switch in a row, on the second Plan's trajectories: the generator's round-2
        # categories on the splines as they now are. No Plan follows it (see the module docstring).
        traj[:] = traj2
        alive = [b for b in range(LISTED) if int(summary2["status"][b]) == 0 and len(traj2[b]["time"]) > 2]
        assert len(alive) >= LISTED // 2, (D, len(alive))
        third = {b: sw.make_case(rows[2][b]["case"]["label"], rng, *state[b]) for b in alive}
        order = [int(b) for b in rng.permutation(alive)]
        widest = max(len(third[b]["waypoints"]) for b in alive)
        while len(third[order[-1]]["waypoints"]) == widest:      # the call's last query is not a widest one
            order.insert(0, order.pop())
        ids = np.array(order, dtype=np.int32)
        t_ns = times_for(ids, False, on_grid=False)
        wps = [third[b]["waypoints"] for b in ids]
        keep = np.array([third[b]["keep"] for b in ids])
        verify("third", ids, t_ns, wps, _switch_call(ps, ids, t_ns, wps, keep), keep=keep)
        assert seen["third/ok"] >= len(alive) // 2, (D, seen)
    print("D = %2d: %s" % (D, dict(sorted(seen.items()))))


@pytest.mark.parametrize("D", ALL_DOFS)
def test_fit(env, D):
    """set_waypoints from host arrays and from CUDA tensors (the _device entry) against the
    restatement and the oracle's fit; a planner without waypoints keeps its path."""
    torch, eng, E, dev, tpo, sync = env["torch"], env["eng"], env["E"], env["dev"], env["tpo"], env["sync"]
    cases = sw.make_fit_cases(D)
    by_rounding = {r: [c for c in cases if c["rounding"] == r and c["waypoints"]] for r in sw.FIT_ROUNDINGS}
    n = len(by_rounding[0.2]) + 1                                  # the last planner: no waypoints after the first call
    rng = np.random.default_rng(77 + D)
    vmax, amax, delta = rng.uniform(1, 2, size=(n, D)), rng.uniform(2, 4, size=(n, D)), rng.uniform(0.01, 0.03, size=n)
    for device in (False, True):
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if device else (lambda a: a)
        with eng.PlannerSet(E, n, D, N, num_points=4, time_step_ns=STEP_NS) as ps:
            keeper = None
            for i, rounding in enumerate(sw.FIT_ROUNDINGS):
                lists = [c["waypoints"] for c in by_rounding[rounding]]
                lists.append([[0.5] * D, [1.5] * D] if i == 0 else [])
                offsets = np.concatenate([[0], np.cumsum([len(w) for w in lists])]).astype(np.int32)
                flat = np.asarray(_flat(lists), dtype=np.float64).reshape(-1, D)
                status, num_points = ps.set_waypoints(conv(flat), offsets, conv(vmax), conv(amax), conv(delta),
                                                      rounding=rounding)
                sync()
                status, num_points = status.cpu().numpy(), num_points.cpu().numpy()
                for b, w in enumerate(lists):
                    where = (D, "device" if device else "host", rounding, b, len(w))
                    st, knots, points = sw.fit_spline_to_waypoints(w, rounding)
                    assert int(status[b]) == st, where + (int(status[b]), st)
                    got = ps.download_path(b)
                    if st != sw.OK:
                        assert st == sw.INVALID_ARGUMENT and _same_spline(got, *keeper), where + ("W = 0 changed the path",)
                        continue
                    assert int(num_points[b]) == len(points), where
                    assert _same_spline(got, knots, points), where + ("fit differs",)
                    cps, kn = tpo.joint_fit_spline(np.asarray(w), rounding)
                    assert _same_spline(got, kn.tolist(), cps.tolist()), where + ("oracle differs",)
                    sw.check_fit(w, rounding, got[0].tolist(), got[1].tolist())
                    if b == n - 1:
                        keeper = (knots, points)

"""The spline edits against an independent statement of what they are (tests/switch_reference.py),
on the CPU: the restatement of SwitchToWaypointPath / FitSplineToWaypoints / GetVelocityAtTime
equals the host-compilable routines of the kernels (sw_switch_to_waypoint_path,
sw_velocity_at_time of csrc/tpamd_switch.h, fit_waypoints of csrc/tpamd_fit.h), the mirror
(host/timeable_path_joint_spline.cc, host/spline_edit.cc, host/trajectory_buffer.cc) and the
oracle's fit bit for bit for every D = 1..16 on the cases the GPU test uses
(tests/cpp/test_switch_reference.cc); the exact-arithmetic property checkers pass on all of them
within tolerances measured here on the restatement; every category is reached for every D by the
restatement, the routines and the mirror; the checkers notice mutations. No GPU needed."""
import collections
import functools
import struct
import subprocess
import time

import numpy as np
import pytest

import native_driver
import switch_reference as sw

ALL_DOFS = list(range(1, 17))
LOOSE = {"kept": 1e-9, "join": 1e-9}        # for measuring: any wrong curve is far above this


@functools.lru_cache(maxsize=None)
def rounds(D):
    return sw.make_rounds(D)


@functools.lru_cache(maxsize=None)
def checked(D):
    """check_switch on every successful switch of the restatement (the planner with a non-zero
    first knot apart): (residuals, {(round, b): info})."""
    planners, rows = rounds(D)
    residuals, infos = {}, {}
    for r, row in enumerate(rows):
        for b, e in enumerate(row):
            if e["result"]["status"] != sw.OK or planners[b]["label"] == "nonzero_first_knot":
                continue
            knots, points = e["before"]
            infos[r, b] = sw.check_switch(knots, points, e["case"]["keep"], e["case"]["waypoints"], e["result"]["knots"],
                                          e["result"]["points"], tolerances=LOOSE, residuals=residuals)
    return residuals, infos


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return native_driver.build_driver("test_switch_reference.cc", tmp_path_factory.mktemp("switch_reference"),
                                      libs=("host", "engine"), opt="-O2", timeout=600)


def _hex(values):
    return " ".join(float(x).hex() for x in values)


def _flat(rows):
    return [x for r in rows for x in r]


def run_driver(exe, tmp_path, records):
    """records: text records of the driver. Returns per record ((status, doubles) of R, of M);
    doubles is None where the driver wrote count -1 (the mirror was not run)."""
    src, dst = tmp_path / "cases.txt", tmp_path / "results.bin"
    with open(src, "w") as f:
        f.write("%d\n" % len(records))
        f.write("\n".join(records) + "\n")
    out = subprocess.run([exe, str(src), str(dst)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    data = open(dst, "rb").read()
    pos, parsed = 0, []
    for _ in records:
        pair = []
        for _who in "RM":
            status, count = struct.unpack_from("<ii", data, pos)
            pos += 8
            values = None if count < 0 else np.frombuffer(data, dtype="<f8", count=count, offset=pos)
            pos += 8 * max(count, 0)
            pair.append((status, values))
        parsed.append(tuple(pair))
    assert pos == len(data)
    return parsed


def _spline_bits(knots, points):
    return np.asarray(list(knots) + _flat(points), dtype=np.float64).tobytes()


# ------------------------------------------------------------------ the switch
@pytest.mark.parametrize("D", ALL_DOFS)
def test_switch_restatement_routines_and_mirror_bit_for_bit(driver, tmp_path, D):
    planners, rows = rounds(D)
    residuals, infos = checked(D)
    records, index = [], []
    for r, row in enumerate(rows):
        for b, e in enumerate(row):
            knots, points = e["before"]
            c = e["case"]
            raw = planners[b]["label"] == "nonzero_first_knot"
            rec = "S %d %d %d %d %d %d %s %s" % (b, D, int(r == 0), int(raw), len(points), len(c["waypoints"]),
                                                  float(c["keep"]).hex(), _hex(list(knots) + _flat(points) + _flat(c["waypoints"])))
            if r == 0:
                rec += " %d %s" % (len(planners[b]["waypoints"]), _hex(_flat(planners[b]["waypoints"])))
            records.append(rec)
            index.append((r, b))
    parsed = run_driver(driver, tmp_path, records)
    seen = {who: collections.Counter() for who in ("restatement", "routines", "mirror")}
    for (r, b), ((st_r, val_r), (st_m, val_m)) in zip(index, parsed):
        e = rows[r][b]
        res, c, (knots, points) = e["result"], e["case"], e["before"]
        where = (D, r, b, c["label"])
        P = len(points)
        assert st_r == res["status"], where + ("routines", st_r, res["status"])
        if res["status"] == sw.OK:
            want = _spline_bits(res["knots"], res["points"])
            assert val_r.tobytes() == want, where + ("routines differ",)
            P_after = len(res["points"])
        else:
            want, P_after = _spline_bits(knots, points), P
        if val_m is not None:
            assert st_m == res["status"], where + ("mirror", st_m, res["status"])
            assert val_m.tobytes() == want, where + ("mirror differs",)      # a failed switch changes nothing
        if r == 0:
            for who, st in (("restatement", res["status"]), ("routines", st_r), ("mirror", st_m)):
                if who == "mirror" and val_m is None:
                    st = c["status"]         # bit parity with the restatement only (a non-zero first knot)
                assert sw.reached(c, st, P, P_after), where + (who, st, P, P_after)
                seen[who][c["label"]] += 1
        if (r, b) in infos:
            # the routines' and the mirror's splines are the restatement's bits: the checker's pass holds for all
            info = infos[r, b]
            assert info["residual_kept"] <= sw.TOLERANCES["kept"] and info["residual_join"] <= sw.TOLERANCES["join"], where
            assert not info["in_slack"], where + ("the case sits inside the checker's decision slack",)
            if c["num_new"] is not None:
                assert info["num_new"] == c["num_new"], where
            if c["label"] == "negative_t_all_kept" and D > 1:
                assert info["has_proj"] and info["first"] == 0 and info["num_new"] == sw.WMAX + 1, where
            if c["label"] == "near_projection":
                assert not info["has_proj"], where
    for who, counts in seen.items():
        assert [k for k, _ in sw.CATEGORIES if not counts[k]] == [], (D, who)


def test_tolerances_are_measured_on_the_restatement():
    """Prints the worst residuals of B.1 / B.2 over every successful switch of make_rounds(D),
    D = 1..16, and holds the recorded figures (MEASURED_RESIDUALS, TOLERANCES = 8 x) to them."""
    t0 = time.time()
    worst, count = {}, 0
    for D in ALL_DOFS:
        residuals, infos = checked(D)
        count += len(infos)
        for k, v in residuals.items():
            worst[k] = max(worst.get(k, 0.0), v)
    print("check_switch on %d successful switches, D = 1..16: %.1f s" % (count, time.time() - t0))
    print("measured residuals:", {k: "%.3g" % v for k, v in sorted(worst.items())})
    print("tolerances:", {k: "%.3g" % v for k, v in sorted(sw.TOLERANCES.items())})
    assert count >= 16 * 3 * 40
    for k in ("kept", "join"):
        assert worst[k] <= sw.MEASURED_RESIDUALS[k] <= 1.25 * worst[k] + 1e-18, (k, worst[k])
        assert sw.TOLERANCES[k] == 8 * sw.MEASURED_RESIDUALS[k]


def test_restatement_capacity_and_refused_splines():
    """What the generated cases do not reach: the capacity rule (taken as an argument) and the
    checks a spline is refused with."""
    planners, _ = rounds(3)
    p = next(q for q in planners if len(q["points"]) >= 10)
    knots, points = p["knots"], p["points"]
    keep, wps = 0.5 * knots[-1], [[1.0, 2.0, 3.0], [2.0, 2.0, 2.0], [0.0, 1.0, 0.0]]
    nk = len(knots)
    assert sw.switch_to_waypoint_path(knots, points, keep, wps)["status"] == sw.OK
    assert sw.switch_to_waypoint_path(knots, points, keep, wps, capacity=nk + 2)["status"] == sw.FAILED_PRECONDITION
    res = sw.switch_to_waypoint_path(knots, points, keep, wps, capacity=nk + 3)       # the insertion fits, the extension may not
    full = sw.switch_to_waypoint_path(knots, points, keep, wps)
    assert res["status"] == (sw.OK if len(full["knots"]) <= nk + 3 else sw.FAILED_PRECONDITION)
    assert sw.switch_to_waypoint_path(knots, points, keep, wps, capacity=nk - 1)["status"] == sw.OUT_OF_RANGE
    assert sw.switch_to_waypoint_path([], [], keep, wps)["status"] == sw.FAILED_PRECONDITION
    assert sw.switch_to_waypoint_path(knots[:5], points[:2], keep, wps)["status"] == sw.OUT_OF_RANGE
    assert sw.switch_to_waypoint_path(knots, points[:-1], keep, wps)["status"] == sw.INVALID_ARGUMENT
    bad = list(knots)
    bad[4], bad[5] = bad[5], bad[4]
    assert sw.switch_to_waypoint_path(bad, points, keep, wps)["status"] == sw.INVALID_ARGUMENT
    assert sw.device_capacity(22, 6) == 100 and sw.device_capacity(60, 6) == 146


# ------------------------------------------------------------------ the fit
@pytest.mark.parametrize("D", ALL_DOFS)
def test_fit_restatement_routine_mirror_and_oracle_bit_for_bit(driver, tmp_path, D):
    from oracle import tpo
    cases = sw.make_fit_cases(D)
    records = ["F %d %d %s %s" % (D, len(c["waypoints"]), float(c["rounding"]).hex(), _hex(_flat(c["waypoints"])))
               for c in cases]
    parsed = run_driver(driver, tmp_path, records)
    seen = collections.Counter()
    for c, ((st_r, val_r), (st_m, val_m)) in zip(cases, parsed):
        where = (D, c["label"])
        st, knots, points = sw.fit_spline_to_waypoints(c["waypoints"], c["rounding"])
        assert st_r == st_m == st, where + (st_r, st_m, st)
        if st != sw.OK:
            assert not c["waypoints"] and st == sw.INVALID_ARGUMENT, where
            seen["empty"] += 1
            continue
        want = _spline_bits(knots, points)
        assert val_r.tobytes() == want, where + ("routine differs",)
        assert val_m.tobytes() == want, where + ("mirror differs",)
        cps, kn = tpo.joint_fit_spline(np.asarray(c["waypoints"]), c["rounding"])
        assert _spline_bits(kn.tolist(), cps.tolist()) == want, where + ("oracle differs",)
        sw.check_fit(c["waypoints"], c["rounding"], knots, points)
        seen[c["label"].split("/")[0]] += 1
        seen["short_polygon" if knots[-1] == 0.1 else "long_polygon"] += 1
    for k in ("W1", "W2", "W40", "repeated", "collinear", "short", "empty", "short_polygon", "long_polygon"):
        assert seen[k], (D, k, seen)


# ------------------------------------------------------------------ the velocity
@pytest.mark.parametrize("D", ALL_DOFS)
def test_velocity_restatement_routine_and_mirror_bit_for_bit(driver, tmp_path, D):
    cases = sw.make_velocity_cases(D)
    records = ["V %d %d %s %s" % (D, len(c["time"]), float(c["query"]).hex(), _hex(list(c["time"]) + _flat(c["velocity"])))
               for c in cases]
    parsed = run_driver(driver, tmp_path, records)
    seen = collections.Counter()
    for c, ((st_r, val_r), (st_m, val_m)) in zip(cases, parsed):
        where = (D, c["label"], len(c["time"]))
        st, v = sw.velocity_at_time(c["time"], c["velocity"], c["query"])
        assert st_r == st_m == st, where + (st_r, st_m, st)
        if st == sw.OK:
            want = np.asarray(v, dtype=np.float64).tobytes()
            assert val_r.tobytes() == want and val_m.tobytes() == want, where
        sw.check_velocity(c["time"], c["velocity"], c["query"], st, v)
        seen[c["label"], sw.STATUS_NAMES[st]] += 1
    for k in (("no_samples", "failed_precondition"), ("on_sample", "ok"), ("between", "ok"), ("first", "ok"),
              ("last", "ok"), ("inside", "ok"), ("before", "out_of_range"), ("after", "out_of_range")):
        assert seen[k], (D, k, seen)


# ------------------------------------------------------------------ the checkers notice errors
def _mutation_case():
    planners, rows = rounds(4)
    for b, e in enumerate(rows[0]):
        if e["case"]["label"] == "negative_t_all_kept":
            return e
    raise AssertionError("no such planner")


def _copy(res):
    return [float(x) for x in res["knots"]], [list(p) for p in res["points"]]


MUTATIONS = ("kept_point", "join_point", "join_knot_doubled", "last_point", "projected_point_dropped",
             "first_waypoint_dropped", "projected_point_moved", "lerp_wrong_row", "bracket_off_by_one",
             "fit_last_knot", "fit_knots_not_uniform", "fit_corner_not_waypoint")


@pytest.mark.parametrize("mutation", MUTATIONS)
def test_the_checkers_notice(mutation):
    e = _mutation_case()
    (knots, points), c, res = e["before"], e["case"], e["result"]
    sw.check_switch(knots, points, c["keep"], c["waypoints"], res["knots"], res["points"])
    nk, npts = _copy(res)
    kept = res["np_kept"]
    err = sw.SwitchCheckError
    if mutation in ("lerp_wrong_row", "bracket_off_by_one"):
        vc = next(v for v in sw.make_velocity_cases(4) if v["label"] == "between" and len(v["time"]) == 33)
        t, v, q = vc["time"], vc["velocity"], vc["query"]
        st, good = sw.velocity_at_time(t, v, q)
        sw.check_velocity(t, v, q, st, good)
        _, lo, up = sw.get_offset_bracket(t, q)
        f = (q - t[lo]) / (t[up] - t[lo])
        if mutation == "lerp_wrong_row":
            bad = [a + f * (b - a) for a, b in zip(v[lo], v[up + 1 if up + 1 < len(t) else lo - 1])]
        else:
            f = (q - t[lo - 1]) / (t[lo] - t[lo - 1])
            bad = [a + f * (b - a) for a, b in zip(v[lo - 1], v[lo])]
        with pytest.raises(err):
            sw.check_velocity(t, v, q, st, bad)
        return
    if mutation.startswith("fit_"):
        fc = next(f for f in sw.make_fit_cases(4) if f["label"] == "W6/r0.2")
        _, fk, fp = sw.fit_spline_to_waypoints(fc["waypoints"], fc["rounding"])
        sw.check_fit(fc["waypoints"], fc["rounding"], fk, fp)
        fk, fp = list(fk), [list(p) for p in fp]
        if mutation == "fit_last_knot":
            fk = [k * (1.0 + 1e-13) for k in fk]
        elif mutation == "fit_knots_not_uniform":
            fk[5] += 1e-12
        else:
            fp[3][0] = float(np.nextafter(fp[3][0], np.inf))
        with pytest.raises(err):
            sw.check_fit(fc["waypoints"], fc["rounding"], fk, fp)
        return
    wps = c["waypoints"]
    if mutation == "kept_point":
        npts[1][0] += 1e-13
    elif mutation == "join_point":
        npts[kept - 1][0] += 1e-11
    elif mutation == "join_knot_doubled":
        nk[kept + 1] = nk[kept]
    elif mutation == "last_point":
        npts[-1][0] = float(np.nextafter(npts[-1][0], np.inf))
    elif mutation == "projected_point_dropped":       # the polygon of the given waypoints alone
        del npts[kept:kept + 3]
        del nk[kept + 1:kept + 4]
    elif mutation == "first_waypoint_dropped":        # as if the line parameter were >= 0
        del npts[kept + 3:kept + 6]
        del nk[kept + 1:kept + 4]
    elif mutation == "projected_point_moved":
        npts[kept] = [x + 1e-9 for x in npts[kept]]
    with pytest.raises(err) as info:
        sw.check_switch(knots, points, c["keep"], wps, nk, npts)
    print("%s: %s" % (mutation, info.value))

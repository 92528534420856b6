"""The independent high-precision reference (tests/hp_reference.py) and the structured path
families (tests/structured_paths.py) on the CPU oracle: the reference against the spline
fixtures, every family's statuses, properties and regime, the straight family's analytic time,
and negative controls that the property checker must reject."""
import json
import os

import numpy as np
import pytest

import hp_reference as hp
import structured_paths as sp
from oracle import tpo

# families whose rest-to-rest N = 2000 paths keep the acceleration rule with no exception
# beyond the checker's (hp_reference.check_profile docstring)
ACCEL_STRICT = ("straight_linear", "straight_long", "idle_one", "idle_most", "near_idle",
                "tie_scaled", "tie_mirror", "velocity_bound", "stop_first", "out_and_back")

# Everywhere else the rule has exceptions: samples over safety * amax that are not next to an
# sdd == 0 sample. Per family: (how many, largest ratio to safety * amax) over all the batches of
# test_family_on_the_oracle, as measured on the oracle. The test fails if a family gets more or
# larger ones. The large ratios sit where sd2 reaches the LP's kMaxSd2 = 1e6 cap (the reference
# caps there too, time_optimal_path_timing.cc:1094-1095, :1217-1220): at a cusp where every q'
# nearly vanishes at once (tie_all), or on a joint whose acceleration limit is 1e4 below another's
# (spread_down, accel_bound), the sd of a neighbouring sample times q'' overshoots its bound.
ACCEL_EXCEPTIONS = {
    "straight_linear": (0, 0.0), "straight_long": (3, 1.709), "idle_one": (3, 1.078),
    "idle_most": (11, 8.003), "near_idle": (6, 1.187), "tie_scaled": (10, 13.26),
    "tie_mirror": (6, 1.781), "tie_all": (16, 15.46), "spread_up": (12, 9.64),
    "spread_down": (14, 1.932e4), "velocity_bound": (5, 1.048), "accel_bound": (27, 4.904e5),
    "stop_interior": (15, 14.43), "stop_first": (13, 15.38), "stop_last": (6, 14.15),
    "out_and_back": (16, 7.615),
}


def test_reference_spline_matches_the_golden_tables(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "bspline_golden.json")))
    knots = np.array(g["knots"], float)
    pts = np.array(g["control_points"], float)
    n = g["num_samples"]
    du = (knots[-1] - knots[0]) / (n - 1)
    u = np.array([knots[0] + i * du for i in range(n)])
    vals = hp.eval_spline(knots, g["degree"], pts, u, 3).astype(float)
    tol = g["tolerance_error_norm"]
    assert np.linalg.norm(vals[0, :, 0] - g["tables"]["X"]) <= tol
    assert np.linalg.norm(vals[0, :, 1] - g["tables"]["Y"]) <= tol
    for k, (nx, ny) in enumerate([("Xp", "Yp"), ("Xpp", "Ypp"), ("Xppp", "Yppp")], 1):
        assert np.sum((vals[k, :, 0] - g["tables"][nx]) ** 2) <= tol, nx
        assert np.sum((vals[k, :, 1] - g["tables"][ny]) ** 2) <= tol, ny
    # mpmath, from the recursive definition, on a few points (the end point included)
    for x in (0.0, 0.1234, 0.5, 0.75, 1.0):
        ref = hp.eval_spline_mp(knots, g["degree"], pts, x, 3)
        got = hp.eval_spline(knots, g["degree"], pts, np.array([x]), 3)
        for d in range(4):
            for c in range(2):
                assert abs(float(got[d, 0, c]) - float(ref[d][c])) <= 1e-13 * (1 + abs(float(ref[d][c])))


def test_reference_spline_matches_mpmath_on_fitted_degree2_paths():
    b = sp.make_family("stop_interior", 2, 5, 100)
    for i in range(2):
        kn, cp = b["knots"][i], b["control_points"][i]
        us = [kn[0], kn[5], 0.5 * (kn[6] + kn[7]), kn[-1] * 0.9, kn[-1]]
        got = hp.eval_spline(kn, 2, cp, np.array(us), 2)
        for m, x in enumerate(us):
            ref = hp.eval_spline_mp(kn, 2, cp, x, 2)
            for d in range(3):
                for c in range(5):
                    r = float(ref[d][c])
                    assert abs(float(got[d, m, c]) - r) <= 1e-13 * (1 + abs(r)), (i, x, d, c)


def _regime(name, b, r):
    """Assert, on the oracle's output, that family `name` reaches the regime it is built for."""
    B, N = r["t"].shape
    D = b["vmax"].shape[1]
    q1 = np.stack([tpo.joint_sample_path(b["knots"][i], b["control_points"][i], b["path_start"][i],
                                         b["delta"][i], N)[1] for i in range(B)])
    qd, sd = r["qd"], r["sd"]
    vel = np.abs(qd) >= 0.8 * b["vmax"][:, None, :] * (1 - 1e-9)
    if name == "straight_linear":
        q2 = np.stack([hp.sample_path(b["knots"][i], b["control_points"][i], 0.0, b["delta"][i], N)[2]
                       for i in range(B)])
        assert np.abs(q2).max() <= 1e-9
    elif name == "straight_long":
        assert (np.abs(q1[:, 1:-1] - q1[:, N // 2:N // 2 + 1]).max(axis=(1, 2)) > 1e-3).all()
    elif name == "idle_one":
        assert (np.abs(q1[:, :, 0]) < tpo.KTINY).all()        # rows the solver skips
    elif name == "idle_most":
        assert (np.abs(q1[:, :, :-1]) < tpo.KTINY).all() and vel[:, :, -1].any(axis=1).all()
    elif name == "near_idle":
        a = np.abs(q1[:, 1:-1, 0])
        assert ((a < tpo.KTINY) & (a > 0)).any(axis=1).all() and (a > tpo.KTINY).any()
    elif name == "tie_scaled" and D >= 2:
        assert (q1[:, :, 1] == 4.0 * q1[:, :, 0]).all() and (qd[:, :, 1] == 4.0 * qd[:, :, 0]).all()
    elif name == "tie_mirror" and D >= 2:
        j = min(2, D - 1)
        assert (q1[:, :, j] == -q1[:, :, 0]).all() and (qd[:, :, j] == -qd[:, :, 0]).all()
    elif name == "tie_all":
        assert (qd == qd[:, :, :1]).all()
    elif name in ("spread_up", "spread_down") and D >= 2:
        ratio = b["vmax"][:, 0] / b["vmax"][:, -1]
        ratio = ratio if name == "spread_down" else 1 / ratio
        assert ((ratio > 5e3) & (ratio < 2e4)).all()
        assert vel.any()
    elif name == "velocity_bound":
        assert vel[:, 1:-1].any(axis=2).mean() > 0.5
    elif name == "accel_bound":
        assert not vel.any()
    elif name == "stop_interior":
        inner = sd[:, 1:-1]
        assert (np.abs(q1).max(axis=2) < tpo.KTINY).any(axis=1).all()   # stationary stretches
        assert (inner == 1000.0).any() and (inner == 0.0).any()          # the sd^2 cap, stops
    elif name in ("stop_first", "stop_last"):
        assert (np.abs(q1).max(axis=2) < tpo.KTINY).any(axis=1).all()   # stationary stretches
        assert (np.diff(r["t"], axis=1) == 0).any(axis=1).all()         # time plateaus
    elif name == "out_and_back":
        # the path turns back: some later sample moves every moving joint the other way
        qdm = qd[:, :, np.abs(q1).max(axis=(0, 1)) > 1e-9]
        for i in range(B):
            mid = qdm[i, N // 8]
            assert (np.sign(qdm[i, N // 8:]) == -np.sign(mid)).all(axis=1).any(), i


@pytest.mark.parametrize("name", sp.FAMILIES)
def test_family_on_the_oracle(name):
    stop = name in sp.STOP_FAMILIES
    count, ratio = 0, 0.0
    for D, N in ((7, 2000), (3, 17), (16, 65), (1, 64)):
        b = sp.make_family(name, 4, D, N)
        r = sp.oracle_solve(tpo, b, N)
        assert (r["status"] == 0).all(), r["status"]
        strict = N == 2000 and name in ACCEL_STRICT
        reps = [hp.check_profile(b, r, stationary_ok=stop, accel_allowance=0 if strict else None)]
        if D >= 3 and N == 2000:
            _regime(name, b, r)
        bs = sp.with_starts(sp.make_family(name, 4, D, N, seed=1), seed=D)
        rs = sp.oracle_solve(tpo, bs, N)
        assert (rs["status"] == 0).all(), rs["status"]
        reps.append(hp.check_profile(bs, rs, stationary_ok=stop, accel_allowance=None))
        count += sum(x["accel_unexcused"] for x in reps)
        ratio = max([ratio] + [x["accel_unexcused_max_ratio"] for x in reps])
    pinned_count, pinned_ratio = ACCEL_EXCEPTIONS[name]
    assert count <= pinned_count and ratio <= pinned_ratio * (1 + 1e-3), (count, ratio)


def test_straight_moves_match_the_analytic_bang_bang_time():
    N = 2000
    for D in (1, 3, 7, 16):
        b = sp.make_family("straight_linear", 6, D, N)
        r = sp.oracle_solve(tpo, b, N)
        assert (r["status"] == 0).all()
        for i in range(6):
            T = hp.bang_bang_time(b["knots"][i], b["control_points"][i], b["vmax"][i], b["amax"][i],
                                  0.8)
            assert abs(r["t"][i, -1] - T) <= 1e-6 * T, (D, i, r["t"][i, -1], T)


def test_property_checker_rejects_perturbed_profiles():
    N = 2000
    b = sp.make_family("tie_scaled", 3, 7, N)
    r = sp.oracle_solve(tpo, b, N)
    hp.check_profile(b, r)

    def fails(mutate):
        bad = {k: np.array(v, copy=True) for k, v in r.items()}
        mutate(bad)
        with pytest.raises(AssertionError):
            hp.check_profile(b, bad)

    i, j = np.unravel_index(np.argmax(np.abs(r["qd"][0])), r["qd"][0].shape)

    def qd_rel(o):
        o["qd"][0, i, j] *= 1 + 1e-9
    fails(qd_rel)

    def drop_step(o):                      # one time step left out: every later t moves back
        k = N // 2
        o["t"][0, k:] -= o["t"][0, k] - o["t"][0, k - 1]
    fails(drop_step)

    sdd = r["sdd"][0]
    near0 = np.zeros(N, bool)
    near0[np.flatnonzero(sdd == 0.0)[:, None] + np.array([-2, -1, 0, 1, 2])] = True
    q1 = hp.sample_path(b["knots"][0], b["control_points"][0], 0.0, b["delta"][0], N)[1]
    qdd = r["qdd"][0]
    # a sample on the acceleration bound, away from every fallback sample
    onb = np.flatnonzero(~near0 & (np.abs(qdd) >= 0.8 * b["amax"][0] * (1 - 1e-9)).any(axis=1)
                         & (np.abs(sdd) > 1e-3))
    assert onb.size
    k = onb[0]
    jj = int(np.argmax(np.abs(qdd[k]) / b["amax"][0]))
    assert abs(float(q1[k, jj])) > 1e-3

    def sdd_scaled(o):
        o["sdd"][0, k] *= 1.01
        # keep qdd consistent with the scaled sdd, so that only the acceleration bound can fail
        qd_, qdd_ = tpo.epilogue(*tpo.joint_sample_path(b["knots"][0], b["control_points"][0], 0.0,
                                                        b["delta"][0], N)[1:],
                                 o["sd"][0], o["sdd"][0], b["amax"][0])
        o["qdd"][0] = qdd_
    with pytest.raises(AssertionError, match="acceleration"):
        bad = {kk: np.array(v, copy=True) for kk, v in r.items()}
        sdd_scaled(bad)
        hp.check_profile(b, bad)

"""The Cartesian half of the independent reference (tests/hp_reference.py) on the CPU: mpmath
against longdouble, the quaternion definitions against the reference's Mathematica table, the
pose sampler against the oracle at the edges of quat_log / quat_power, every Cartesian family of
tests/cartesian_paths.py through check_cartesian_profile and the straight moves' time window, and
negative controls the checker must reject."""
import json
import os

import numpy as np
import pytest

import cartesian_paths as cp
import hp_reference as hp
from oracle import tpo

DOFS = (1, 2, 6, 7, 15, 16)

# Samples over safety * amax that check_cartesian_profile does not excuse (not next to an
# sdd == 0 sample or a stationary one), per family, summed over test_family_on_the_oracle's
# batches (DOFS x cp.SAMPLE_COUNTS, 4 paths each), with the largest ratio to safety * amax, as
# measured on the oracle. The test fails if a family gets more or larger ones. The straight moves
# keep the rule everywhere. The curved families break it where check_profile's table says the
# joint families do: on the coarse N = 64 grids (the reference's sdd of a sample is the
# acceleration of the step that leaves it) and behind a start velocity. idle's many and large
# ones sit on the edges of its stops: the forward differences put the whole turn of the path into
# one q'' row next to a q' that vanishes, sd^2 there reaches the LP's 1e6 cap, and the
# neighbouring sample's q'' sd^2 overshoots by up to 1e4 (the reference computes the same).
ACCEL_EXCEPTIONS = {
    "straight_trans": (0, 0.0), "straight_rot": (0, 0.0), "straight_joint": (0, 0.0),
    "straight_accel": (0, 0.0), "zero_jacobian": (10, 5.166), "singular": (27, 19.04),
    "idle": (970, 1.0243e4),
}


def _solve(name, D, N, B=4, seed=0):
    b = cp.make_family(name, B, D, N, seed)
    if name in cp.CURVED:
        b = cp.with_starts(b, seed)
    return b, cp.oracle_solve(tpo, b)


# ------------------------------------------------------------------ quaternions
def test_reference_quat_exp_reproduces_the_golden_table(golden_dir):
    g = json.load(open(os.path.join(golden_dir, "quat_exp_golden.json")))
    for q, e in zip(g["input"], g["exp"]):
        e = np.asarray(e)
        # the table prints 16 significant digits: the reference's IsApprox 1e-12
        quat = hp.quat_exp_mp(q)
        assert np.linalg.norm(quat - e) <= 1e-12 * np.linalg.norm(e), q
        ld = hp.quat_exp(np.array(q)).astype(float)
        assert np.linalg.norm(ld - e) <= 1e-12 * np.linalg.norm(e), q
        # log inverts exp on the principal branch (|v| of the log below pi)
        lg = hp.quat_log_mp(e)
        if np.linalg.norm(q[1:]) < np.pi:
            assert np.allclose(lg, q, rtol=0, atol=1e-13 * np.linalg.norm(q)), q


def test_quat_power_edges_mpmath_and_longdouble_agree():
    rng = np.random.default_rng(3)
    qs = [rng.standard_normal(4) for _ in range(6)]
    qs += [np.array([1.0, 0, 0, 0]), np.array([-1.0, 0, 0, 0]),           # |v| = 0, w = +-1
           np.array([1.0, 3e-13, -2e-13, 1e-13]),                           # |v| < 1e-12
           np.array([-1.0, 3e-13, -2e-13, 1e-13]),                          # the same, w < 0
           np.array([5e-7, 0.6, 0.8, 0.0]), np.array([-5e-7, 0.6, 0.8, 0.0]),   # w ~ 0
           np.array([0.0, 0.0, 1.0, 0.0])]                                  # w = 0 exactly
    M, _, _, _, _, power = hp._mp_quat()
    for q in qs:
        q = q / np.linalg.norm(q)
        for p in (0.0, 0.3, 0.5, 1.0):
            ld = hp.quat_power(q, p).astype(float)
            with M.workdps(hp.MP_DPS):
                mp = np.array([float(x) for x in power(tuple(M.mpf(float(x)) for x in q), p)])
            assert np.max(np.abs(ld - mp)) <= 1e-18, (q, p)
            # the flip to w >= 0 first: q and -q have the same powers, and q^1 is q up to sign
            assert np.max(np.abs(hp.quat_power(-q, p).astype(float) - ld)) <= 1e-18 or q[0] == 0
            if p == 1.0:
                assert np.max(np.abs(ld - (q if q[0] >= 0 else -q))) <= 1e-18
    # an antipodal pair is one orientation: the power of -1 is the identity
    assert np.array_equal(hp.quat_power(np.array([-1.0, 0, 0, 0]), 0.37).astype(float), [1, 0, 0, 0])


@pytest.mark.parametrize("P,N", [(16, 400), (3, 80)])
def test_pose_sampling_mpmath_and_longdouble_agree(P, N):
    e = cp.pose_edge_paths(P, N)
    idx = sorted({0, 1, 7, 8, 62, 63, N // 2, N - 41, N - 40, N - 1})
    for b in range(e["knots"].shape[0]):
        args = (e["knots"][b], e["translation"][b], e["rotation"][b], e["path_start"][b],
                e["delta"][b], N)
        ld = hp.sample_poses(*args)
        mp = hp.sample_poses_mp(*args, idx)
        assert np.max(np.abs(ld[idx].astype(float) - mp)) <= 1e-17, b


@pytest.mark.parametrize("P,N", [(16, 400), (3, 80), (1023, 1100)])
def test_reference_pose_sampling_matches_the_oracle_at_the_edges(P, N):
    """Measured: at most 5.8e-16 between the oracle and the reference (P = 1023 included), on the
    translations 2.2e-16; the bound is 4e-15, about 20 ulp of a unit quaternion."""
    e = cp.pose_edge_paths(P, N)
    for b in range(e["knots"].shape[0]):
        args = (e["knots"][b], e["translation"][b], e["rotation"][b], e["path_start"][b],
                e["delta"][b], N)
        ref = hp.sample_poses(*args)
        orc = tpo.sample_pose_spline(*args)
        assert np.max(np.abs(orc - ref.astype(float))) <= 4e-15, b
        par, pad = hp.pose_parameters(e["knots"][b], e["path_start"][b], e["delta"][b], N)
        assert np.array_equal(orc[pad, 3:], np.broadcast_to(e["rotation"][b, -1], (pad.sum(), 4)))
        assert np.all(orc[~pad, 3] >= 0)
    # the edges are reached: path 5 on the knots, path 6 exactly on k_end - delta
    kn = e["knots"][5]
    par5, pad5 = hp.pose_parameters(kn, e["path_start"][5], e["delta"][5], N)
    assert np.isin(par5[~pad5], kn).sum() >= P - 3
    par6, pad6 = hp.pose_parameters(e["knots"][6], 0.0, e["delta"][6], N)
    kend = e["knots"][6, -1]
    assert par6[63] == kend - e["delta"][6] and pad6[63] and not pad6[62]


def test_near_pi_relative_rotations_turn_the_way_the_flip_says():
    """Path 3 of pose_edge_paths puts p0^-1 p1 on both sides of a rotation by pi (w = +-5e-7), so
    that the flip to w >= 0 reverses the direction of interpolation on one pair and not on the
    other; the sampling tests above then hold the oracle and the engine to the reference there."""
    e = cp.pose_edge_paths(16, 400)
    rot = e["rotation"][3]
    w = [hp._qmul(hp._qinv(rot[j - 1].astype(hp.LD)), rot[j].astype(hp.LD))[0] for j in (1, 4)]
    assert float(w[0]) > 0 > float(w[1]) and max(abs(float(x)) for x in w) < 1e-6


# ------------------------------------------------------------- profile checks
@pytest.mark.parametrize("name", cp.FAMILIES)
def test_family_on_the_oracle(name):
    unexcused, ratio = 0, 0.0
    for D in DOFS:
        for N in cp.SAMPLE_COUNTS:
            b, r = _solve(name, D, N)
            assert (r["status"] == 0).all(), (name, D, N, r["status"])
            rep = hp.check_cartesian_profile(b, r, accel_allowance=None)
            unexcused += rep["accel_unexcused"]
            ratio = max(ratio, rep["accel_unexcused_max_ratio"])
            if N >= 64:
                _regime(name, b, r, rep)
    n, top = ACCEL_EXCEPTIONS[name]
    assert unexcused <= n and ratio <= top * (1 + 1e-3), (name, unexcused, ratio)


def _regime(name, b, r, rep):
    """Assert that family `name` reaches the regime it is built for (N >= 64)."""
    B, N = r["t"].shape
    if name == "straight_trans":
        assert rep["trans_active"] >= B * N // 4 and rep["rot_max_ratio"] <= 0.11
    elif name == "straight_rot":
        assert rep["rot_active"] >= B * N // 4 and rep["trans_max_ratio"] <= 0.11
    elif name == "straight_joint":
        assert rep["vel_active"] >= B * N // 8
        assert max(rep["trans_max_ratio"], rep["rot_max_ratio"]) <= 0.11
    elif name == "straight_accel":
        assert rep["vel_active"] == 0 and max(rep["trans_max_ratio"], rep["rot_max_ratio"]) < 0.01
    elif name == "zero_jacobian":
        assert rep["trans_max_ratio"] == 0.0 and rep["rot_max_ratio"] == 0.0
    elif name == "singular":
        m = N // 2
        q1, _ = hp.cartesian_derivatives(b["ik_positions"][0], b["delta"][0])
        vt, vr, mt, mr = hp.cartesian_velocities(b["jacobians"][0], q1)
        assert vt[m] <= 1e-14 * mt[m] and vr[m] <= 1e-14 * mr[m] and vt[m - 1] > 1e-3 * mt[m - 1]
    elif name == "idle":
        q1, _ = hp.cartesian_derivatives(b["ik_positions"][0], b["delta"][0])
        still = (q1 == 0).all(axis=1)
        assert still[N // 3:N // 3 + N // 5].all() and still[:N // 20].all()
        assert rep["trans_active"] + rep["rot_active"] > 0


@pytest.mark.parametrize("name", cp.STRAIGHT)
@pytest.mark.parametrize("D", [1, 6, 16])
@pytest.mark.parametrize("N", [64, 2000])
def test_straight_moves_end_in_the_bang_bang_window_on_the_oracle(name, D, N):
    b, r = _solve(name, D, N)
    for i in range(4):
        assert r["sd"][i, -2] == 0.0                      # at rest one sample early (end rule)
        lo, hi = hp.straight_window(b, i)
        t = r["t"][i, -2] - r["t"][i, 0]
        assert lo <= t <= hi, (i, lo, t, hi)
        assert r["t"][i, -1] == r["t"][i, -2]


# ------------------------------------------------------------ negative controls
def test_checker_rejects_perturbed_profiles():
    b, r = _solve("singular", 6, 400)
    hp.check_cartesian_profile(b, r)
    # sd raised by 1e-6 at one sample on the translation limit
    rep_t = hp.cartesian_velocities(b["jacobians"][0], hp.cartesian_derivatives(
        b["ik_positions"][0], b["delta"][0])[0])[0] * r["sd"][0]
    k = int(np.argmax(rep_t[1:-1] / b["vtrans"][0])) + 1
    bad = {key: v.copy() for key, v in r.items()}
    bad["sd"][0, k] *= 1 + 1e-6
    bad["qd"][0, k] *= 1 + 1e-6                          # consistent qd: only the limit is off
    with pytest.raises(AssertionError, match="over its limit"):
        hp.check_cartesian_profile(b, bad, paths=[0])
    # one time step changed
    bad = {key: v.copy() for key, v in r.items()}
    bad["t"][0, 200:] += 1e-9 * bad["t"][0, -1]
    with pytest.raises(AssertionError, match="time steps"):
        hp.check_cartesian_profile(b, bad, paths=[0])
    # q'' at sample 0 not forced to 0 (sd_start > 0 on path 1 makes it visible in qdd)
    assert b["sd_start"][1] > 0
    q1, q2 = hp.cartesian_derivatives(b["ik_positions"][1], b["delta"][1])
    bad = {key: v.copy() for key, v in r.items()}
    q20 = (q1[1] - q1[0]) / hp.LD(b["delta"][1])
    bad["qdd"][1, 0] = np.clip((q1[0] * hp.LD(r["sdd"][1, 0]) + q20 * hp.LD(r["sd"][1, 0]) ** 2)
                               .astype(float), -b["amax"][1], b["amax"][1])
    with pytest.raises(AssertionError, match="qdd"):
        hp.check_cartesian_profile(b, bad, paths=[1])


def test_safety_on_v_trans_is_caught():
    """A solver that applied the joint safety factor to v_trans as well: its profile is feasible
    (it is slower) but leaves the straight-move window, and the translation row is never active."""
    b, r = _solve("straight_trans", 6, 2000)
    slow = dict(b, vtrans=b["vtrans"] * 0.8)
    rs = cp.oracle_solve(tpo, slow)
    rep = hp.check_cartesian_profile(b, rs)             # feasible against the true limits
    assert rep["trans_active"] == 0 and rep["trans_max_ratio"] <= 0.8 + 1e-9
    for i in range(4):
        lo, hi = hp.straight_window(b, i)
        assert rs["t"][i, -2] - rs["t"][i, 0] > hi

"""Seeded joint-path families with structured or degenerate geometry (test helper).

`synthetic.make_joint_batch` draws every waypoint uniformly and keeps every joint's limits
within 2x of the others, so random batches never reach idle joints, exact ties between
constraint rows, the sd^2 cap of the LP or stationary stretches of a path. Each family below
starts from `make_joint_batch` and edits the waypoints (refitted with
`synthetic.fit_joint_splines`), the control points or the limits, so that it reaches one of
those regimes. Every family returns a batch dict in `make_joint_batch`'s format.

Families (name: what it does):
  straight_linear   two waypoints, |w1 - w0| <= 0.8: control points at exactly 1/4 and 3/4
                    of the segment, so the path is linear in u (known bang-bang answer)
  straight_long     two waypoints 1.5 .. 3 apart: not linear near the ends
  idle_one          joint 0 held constant (equal control points in its column)
  idle_most         every joint but the last held constant: one velocity and one
                    acceleration row carry the whole path
  near_idle         joint 0's control points scaled by 1e-10 .. 1e-11, so |q'| crosses kTiny
  tie_scaled        joint 1 = 4 * joint 0 with 4x its limits: bit-identical row quotients
  tie_mirror        joint 2 = -joint 0 with equal limits: upper / lower bound ties
  tie_all           every joint equal to joint 0, equal limits: a D-way tie
  spread_up         vmax * logspace(-2, 2, D), amax * logspace(2, -2, D)
  spread_down       vmax * logspace(2, -2, D), amax * logspace(-2, 2, D)
  velocity_bound    amax * 1000: the velocity limit binds almost everywhere
  accel_bound       vmax * 1000: the velocity limit is never reached
  stop_interior     a repeated interior waypoint (wp[2] = wp[1])
  stop_first        a repeated first waypoint (wp[1] = wp[0])
  stop_last         a repeated last waypoint (wp[-1] = wp[-2])
  out_and_back      wp[2] = wp[0]

At D = 1 there is no second joint to tie: tie_scaled and tie_mirror are then the unedited
random paths, and tie_all is trivially itself. The tests check the tie regimes at D >= 3.
"""
import importlib

import numpy as np

from conftest import PKG_NAME

syn = importlib.import_module(PKG_NAME + ".synthetic")

FAMILIES = ("straight_linear", "straight_long", "idle_one", "idle_most", "near_idle",
            "tie_scaled", "tie_mirror", "tie_all", "spread_up", "spread_down",
            "velocity_bound", "accel_bound", "stop_interior", "stop_first", "stop_last",
            "out_and_back")
STOP_FAMILIES = ("stop_interior", "stop_first", "stop_last")
SPECIALISED_DOFS = (3, 4, 5, 6, 7, 8, 14)
GENERIC_DOFS = (1, 2, 16)
SAMPLE_COUNTS = (3, 17, 63, 64, 65, 2000)

_SEED = {name: 7_000_000 + 10_000 * k for k, name in enumerate(FAMILIES)}
_WAYPOINTS = {"straight_linear": 2, "straight_long": 2}
WAYPOINTS = 6          # every other family: 3 * 6 - 2 = 16 control points


def _refit(b, wp, N):
    cps, knots = syn.fit_joint_splines(wp)
    b["waypoints"] = wp
    b["control_points"] = np.ascontiguousarray(cps)
    b["knots"] = np.ascontiguousarray(knots)
    b["delta"] = np.ascontiguousarray(knots[:, -1] / (N - 1))


def make_family(name, B, D, N, seed=0):
    """B paths of family `name` with D joints and N samples, seeded by (name, D, seed)."""
    W = _WAYPOINTS.get(name, WAYPOINTS)
    first = _SEED[name] + 100 * D + 1000 * seed
    b = syn.make_joint_batch(B, D, N, num_waypoints=W, first_path_index=first)
    wp = b["waypoints"].copy()
    rng = np.random.default_rng(first)
    if name in ("straight_linear", "straight_long"):
        d = wp[:, 1] - wp[:, 0]
        norm = np.sqrt((d * d).sum(-1, keepdims=True))
        length = rng.uniform(0.3, 0.8, (B, 1)) if name == "straight_linear" else \
            rng.uniform(1.5, 3.0, (B, 1))
        wp[:, 1] = wp[:, 0] + d / norm * length
        _refit(b, wp, N)
    elif name == "idle_one":
        wp[:, :, 0] = wp[:, :1, 0]
        _refit(b, wp, N)
    elif name == "idle_most":
        wp[:, :, :-1] = wp[:, :1, :-1]
        _refit(b, wp, N)
    elif name == "near_idle":
        scale = 10.0 ** rng.uniform(-11.0, -10.0, B)
        b["control_points"][:, :, 0] *= scale[:, None]
    elif name == "tie_scaled" and D >= 2:
        wp[:, :, 1] = 4.0 * wp[:, :, 0]
        b["vmax"][:, 1] = 4.0 * b["vmax"][:, 0]
        b["amax"][:, 1] = 4.0 * b["amax"][:, 0]
        _refit(b, wp, N)
    elif name == "tie_mirror" and D >= 2:
        j = min(2, D - 1)
        wp[:, :, j] = -wp[:, :, 0]
        b["vmax"][:, j] = b["vmax"][:, 0]
        b["amax"][:, j] = b["amax"][:, 0]
        _refit(b, wp, N)
    elif name == "tie_all":
        wp[:] = wp[:, :, :1]
        b["vmax"][:] = b["vmax"][:, :1]
        b["amax"][:] = b["amax"][:, :1]
        _refit(b, wp, N)
    elif name in ("spread_up", "spread_down"):
        up = np.logspace(-2.0, 2.0, D)
        down = np.logspace(2.0, -2.0, D)
        b["vmax"] = b["vmax"] * (up if name == "spread_up" else down)
        b["amax"] = b["amax"] * (down if name == "spread_up" else up)
    elif name == "velocity_bound":
        b["amax"] = b["amax"] * 1000.0
    elif name == "accel_bound":
        b["vmax"] = b["vmax"] * 1000.0
    elif name == "stop_interior":
        wp[:, 2] = wp[:, 1]
        _refit(b, wp, N)
    elif name == "stop_first":
        wp[:, 1] = wp[:, 0]
        _refit(b, wp, N)
    elif name == "stop_last":
        wp[:, -1] = wp[:, -2]
        _refit(b, wp, N)
    elif name == "out_and_back":
        wp[:, 2] = wp[:, 0]
        _refit(b, wp, N)
    for k in ("vmax", "amax"):
        b[k] = np.ascontiguousarray(b[k])
    b["family"] = name
    return b


def with_starts(b, seed=0):
    """Give some paths a start velocity, a start parameter past 0 (which moves the horizon past
    the spline's end, into the end padding) or a nonzero start time. Path 0 is left alone."""
    B = b["control_points"].shape[0]
    rng = np.random.default_rng(seed + 17)
    pick = np.arange(B) % 4
    b["sd_start"] = np.where(pick == 1, rng.uniform(0.01, 0.05, B), 0.0)
    b["path_start"] = np.where(pick == 2, rng.uniform(0.05, 0.3, B) * b["knots"][:, -1], 0.0)
    b["time_start"] = np.where(pick >= 2, rng.uniform(0.5, 80.0, B), 0.0)
    for k in ("sd_start", "path_start", "time_start"):
        b[k] = np.ascontiguousarray(b[k])
    return b


def concat(batches):
    """Concatenate batches of one D and one control-point count along the path axis."""
    keys = ("control_points", "knots", "vmax", "amax", "path_start", "delta", "sd_start",
            "time_start")
    out = {k: np.ascontiguousarray(np.concatenate([x[k] for x in batches])) for k in keys}
    out["num_samples"] = batches[0]["num_samples"]
    out["safety"] = batches[0]["safety"]
    return out


def oracle_solve(tpo, b, N, nthreads=8):
    return tpo.time_joint_batch(b["knots"], b["control_points"], b["vmax"], b["amax"],
                                b["path_start"], b["delta"], N, sd_start=b["sd_start"],
                                time_start=b["time_start"], safety=b["safety"],
                                nthreads=nthreads)

"""The shapes the refinement tests share, and the oracle's reference for each, computed once per
process: synthetic.make_joint_batch(16, D, 33, 4) refined with max_samples 129, max_rounds 2 and
tolerance 0 into 16 slots."""
import functools
import importlib

import numpy as np

from conftest import PKG_NAME

import refine_reference as rr

DOFS = (1, 3, 6, 7, 8, 14, 16)
PATHS, SAMPLES, WAYPOINTS = 16, 33, 4
MAX_SAMPLES, MAX_ROUNDS = 129, 2


@functools.lru_cache(maxsize=None)
def joint_batch(D):
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    return syn.make_joint_batch(PATHS, D, SAMPLES, WAYPOINTS)


@functools.lru_cache(maxsize=None)
def joint_reference(D, max_rounds=MAX_ROUNDS, max_samples=MAX_SAMPLES, max_refined=PATHS, tolerance=0.0):
    from oracle import tpo
    tpo.build()
    base = joint_reference(D) if (max_rounds, max_samples, max_refined, tolerance) != (
        MAX_ROUNDS, MAX_SAMPLES, PATHS, 0.0) else None
    return rr.refine_joint_batch(tpo, joint_batch(D), max_rounds, max_samples, max_refined, tolerance,
                                 round0=base["round0"] if base else None)


def summary(ref):
    """(refined paths, paths that took two rounds, paths whose last solve still has violated rows,
    paths that were never refined)."""
    refined = [int(b) for b in ref["slot_path"] if b >= 0]
    two = [int(ref["slot_path"][k]) for k in range(len(ref["slot_path"])) if ref["rounds"][k] == 2]
    left = [int(ref["slot_path"][k]) for k, f in enumerate(ref["final"]) if f and f["record"][0] > 0]
    never = [b for b in range(len(ref["slot"])) if ref["slot"][b] < 0]
    return refined, two, left, never


WAYPOINT_COUNTS = (2, 5, 0, 5, 2, 5, 5, 2)


@functools.lru_cache(maxsize=None)
def waypoint_case(D):
    """A waypoint batch whose waypoint counts differ (one path has none), timed with 33 samples
    that cover each path exactly, and the oracle's reference on the oracle's own fits. Returns
    (the call's arrays, the batch in the joint form with a list entry per path, the reference).
    The waypoints come from the first of twenty seeds for which the oracle refines at least 2 paths."""
    from oracle import tpo
    tpo.build()
    best = None
    for seed in range(20):
        best = _waypoint_case(tpo, D, seed)
        if best[2]["num_refined"] >= 2:
            break
    return best


def _waypoint_case(tpo, D, seed):
    rng = np.random.default_rng(100 * D + seed)
    paths = [rng.uniform(-2.0, 2.0, size=(W, D)) for W in WAYPOINT_COUNTS]
    Bw = len(paths)
    offsets = np.zeros(Bw + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(p) for p in paths])
    vmax = 1.0 + rng.uniform(size=(Bw, D))
    amax = 2.0 + 2.0 * rng.uniform(size=(Bw, D))
    call = dict(waypoints=np.ascontiguousarray(np.concatenate(paths, axis=0)), offsets=offsets, vmax=vmax, amax=amax)
    fits = [tpo.joint_fit_spline(p, 0.2) if len(p) else None for p in paths]
    joint = dict(control_points=[f[0] if f else None for f in fits], knots=[f[1] if f else None for f in fits],
                 vmax=vmax, amax=amax, path_start=np.zeros(Bw), sd_start=np.zeros(Bw), time_start=np.zeros(Bw),
                 delta=np.array([np.float64(f[1][-1]) / np.float64(SAMPLES - 1) if f else 0.0 for f in fits]),
                 num_samples=SAMPLES, safety=0.8)
    ref = rr.refine_joint_batch(tpo, joint, MAX_ROUNDS, MAX_SAMPLES, Bw, 0.0)
    return call, joint, ref


def ragged_batch(D=7, stride=50, paths=PATHS):
    """A ragged batch: counts from {17, 33, 50}, delta = path_end / (n - 1), and one path (the last)
    with sd_start = -1, which fails with status 4. The counts rotate through the three values from
    the offset that gives the oracle the most refined paths (at least 2 are required)."""
    from oracle import tpo
    tpo.build()
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    best = None
    for shift in range(3):
        batch = dict(syn.make_joint_batch(paths, D, stride, WAYPOINTS))
        counts = np.array([(17, 33, 50)[(b + shift) % 3] for b in range(paths)], dtype=np.int32)
        batch["delta"] = batch["knots"][:, -1] / (counts - 1)
        batch["sd_start"] = batch["sd_start"].copy()
        batch["sd_start"][paths - 1] = -1.0
        batch["num_samples"] = stride
        ref = rr.refine_joint_batch(tpo, batch, MAX_ROUNDS, MAX_SAMPLES, paths, 0.0, counts=counts, stride=stride)
        if best is None or ref["num_refined"] > best[2]["num_refined"]:
            best = (batch, counts, ref)
    return best

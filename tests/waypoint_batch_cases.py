"""The waypoint batches of tests/test_gpu_waypoint_batch*.py and tests/test_waypoint_batch_cpu.py and
what the oracle makes of them: per path tpo.joint_fit_spline, then tpo.time_joint_batch on that one
spline with delta = path_end / (n - 1) (one numpy float64 division) unless the case gives deltas.

One batch has twelve paths with 0, 1, 2, 3, 5 and 11 waypoints -- 0, 4, 4, 7, 13 and 31 control
points, so the largest count is not the first path's and most paths use part of their slot -- two
roundings (0 included) and the sample counts 3 (the minimum), 63 / 64 / 65 (either side of the
64-thread blocks ragged batches use), 257 and the stride."""
import functools

import numpy as np

NUM_SAMPLES = 300
WAYPOINT_COUNTS = [2, 0, 11, 1, 3, 5, 5, 3, 11, 2, 1, 0]
SAMPLE_COUNTS = [3, 63, 64, 65, 257, NUM_SAMPLES, NUM_SAMPLES, 257, 65, 64, 63, 3]
ROUNDINGS = [0.2, 0.0] * 6
TIMING_DOFS = (1, 3, 6, 7, 8, 14, 16)
NO_WAYPOINTS = 11           # TPAMD_PATH_NO_WAYPOINTS
SENTINEL = -7.0


def fit_points(W):
    return 0 if W < 1 else (4 if W == 1 else 3 * W - 2)


def make_batch(D, reverse=False, seed=0):
    """waypoints [rows][D], offsets [B + 1], rounding [B], vmax / amax [B][D], ns [B]."""
    rng = np.random.default_rng(1000 * D + seed)
    counts = list(WAYPOINT_COUNTS)
    paths = [rng.uniform(-1.0, 1.0, size=(W, D)) for W in counts]
    vmax = rng.uniform(0.5, 2.0, size=(len(counts), D))
    amax = rng.uniform(0.5, 2.0, size=(len(counts), D))
    ns = np.array(SAMPLE_COUNTS, dtype=np.int32)
    rounding = np.array(ROUNDINGS)
    order = list(range(len(counts)))
    if reverse:
        order.reverse()
    paths = [paths[k] for k in order]
    offsets = np.zeros(len(order) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(p) for p in paths])
    return dict(D=D, B=len(order), waypoints=np.ascontiguousarray(np.concatenate(paths, axis=0)), offsets=offsets,
                paths=paths, rounding=np.ascontiguousarray(rounding[order]), vmax=np.ascontiguousarray(vmax[order]),
                amax=np.ascontiguousarray(amax[order]), ns=np.ascontiguousarray(ns[order]))


def without_empty(batch):
    """The batch without its paths that have no waypoints (and which paths of the batch are left)."""
    keep = [k for k in range(batch["B"]) if len(batch["paths"][k]) > 0]
    paths = [batch["paths"][k] for k in keep]
    offsets = np.zeros(len(keep) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([len(p) for p in paths])
    out = dict(D=batch["D"], B=len(keep), waypoints=np.ascontiguousarray(np.concatenate(paths, axis=0)),
               offsets=offsets, paths=paths)
    for k in ("rounding", "vmax", "amax", "ns"):
        out[k] = np.ascontiguousarray(batch[k][keep])
    return out, keep


def oracle_fits(tpo, batch):
    """Per path (control points [P][D], knots [P + 3]) or None without waypoints."""
    return [tpo.joint_fit_spline(p, r) if len(p) else None for p, r in zip(batch["paths"], batch["rounding"])]


def whole_path_delta(path_end, n):
    return np.float64(path_end) / np.float64(n - 1)


def given_deltas(fits, ns):
    """Deltas that stop short of the path's end (even paths) and run past it (odd paths)."""
    out = np.zeros(len(fits))
    for k, f in enumerate(fits):
        end = f[1][-1] if f is not None else 1.0
        out[k] = (0.6 if k % 2 == 0 else 1.3) * end / (int(ns[k]) - 1)
    return out


def oracle_expectation(tpo, batch, ns=None, delta=None, time_start=None, safety=0.8):
    """What every path of the batch must come out as: a list of dicts (None without waypoints) with
    P, knots, cps, path_end, delta, n and the oracle's timing of that one spline."""
    fits = oracle_fits(tpo, batch)
    out = []
    for k, f in enumerate(fits):
        if f is None:
            out.append(None)
            continue
        cps, knots = f
        n = int(ns[k]) if ns is not None else NUM_SAMPLES
        d = whole_path_delta(knots[-1], n) if delta is None else np.float64(delta[k])
        ref = tpo.time_joint_batch(knots[None], cps[None], batch["vmax"][k:k + 1], batch["amax"][k:k + 1], 0.0, d, n,
                                   time_start=None if time_start is None else time_start[k:k + 1], safety=safety)
        out.append(dict(P=cps.shape[0], knots=knots, cps=cps, path_end=knots[-1], delta=d, n=n, ref=ref))
    return out


@functools.lru_cache(maxsize=None)
def cached_case(D, reverse, mode):
    """(batch, expectation, kwargs of the call) of one case, computed once per session.
    mode: 'whole' (ragged counts, delta NULL), 'given' (ragged counts, given deltas, start times),
    'uniform' (no per-path counts, delta NULL)."""
    from oracle import tpo
    batch = make_batch(D, reverse)
    if mode == "whole":
        kw = dict(ns=batch["ns"], delta=None, time_start=None)
    elif mode == "given":
        kw = dict(ns=batch["ns"], delta=given_deltas(oracle_fits(tpo, batch), batch["ns"]),
                  time_start=np.linspace(0.25, 1.0, batch["B"]))
    else:
        kw = dict(ns=None, delta=None, time_start=None)
    return batch, oracle_expectation(tpo, batch, **kw), kw

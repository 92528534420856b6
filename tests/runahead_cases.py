"""Inputs of tests/test_gpu_sweep_runahead.py (test helper; tools/gpu_runahead_branches.py runs the
diagnostic library over the same batches to count the branches of the sweep's loop queue).

The forward wave of a sweep workgroup runs ahead of the backward wave through a queue of
switching-point loops (csrc/tpamd_sweep_joint.h, "loop queue"). What its protocol does depends on how
many loops a path has, how close successive switching points lie and which wave reaches a switching
point first, so the batches below have many loops on few samples: `make_joint_batch` with the
velocity limits at 0.2 and the acceleration limits at 0.05 of their drawn values (the oracle then
takes 9..18 loops at 130 samples and 20..27 at 600, and solves every path), and the families of
structured_paths.py with stationary stretches (switching points in runs of equal limit-curve
values) or without any contact with the limit curve (no loop at all: the first pair in order).
"""
import importlib

import numpy as np

import structured_paths as sp
from conftest import PKG_NAME

syn = importlib.import_module(PKG_NAME + ".synthetic")

DOFS = (3, 6, 7, 8, 14)
SAMPLES = (130, 257, 600)
PATHS = 32
VMAX_SCALE, AMAX_SCALE = 0.2, 0.05
# stationary stretches | no contact with the limit curve (velocity_bound, straight_*: zero loops)
FAMILIES = ("stop_interior", "stop_first", "stop_last", "out_and_back", "idle_most",
            "velocity_bound", "straight_linear", "straight_long")
FAMILY_SHAPES = ((7, 130), (7, 257), (3, 257))


def tight_batch(D, N, B=PATHS, first=0):
    b = syn.make_joint_batch(B, D, N, first_path_index=first)
    b["vmax"] = np.ascontiguousarray(b["vmax"] * VMAX_SCALE)
    b["amax"] = np.ascontiguousarray(b["amax"] * AMAX_SCALE)
    return b


def family_batch(name, D, N, B=16):
    return sp.make_family(name, B, D, N, seed=3)


def all_batches():
    """(label, D, N, batch) of every protocol-branch input of the test file."""
    for D in DOFS:
        for N in SAMPLES:
            yield "tight D=%d N=%d" % (D, N), D, N, tight_batch(D, N)
    for name in FAMILIES:
        for D, N in FAMILY_SHAPES:
            yield "%s D=%d N=%d" % (name, D, N), D, N, family_batch(name, D, N)


def oracle_with_loop_limit(tpo, b, i, N, limit):
    """Path i of batch b through the oracle's solver with `limit` switching-point loops (0: the
    default). Returns (status, dict of t, s, sd, sdd or None)."""
    D = b["control_points"].shape[2]
    s0 = float(b["path_start"][i])
    q, q1, q2 = tpo.joint_sample_path(b["knots"][i], b["control_points"][i], s0, b["delta"][i], N)
    rows = tpo.joint_constraint_setup(q1, q2, b["vmax"][i], b["amax"][i], safety=b["safety"])
    p = tpo.Profile(N, 2 * D)
    p.set_max_loops(limit if limit > 0 else max(100, 10 * N))
    rc = p.setup(*rows, s0, s0 + b["delta"][i] * (N - 1), float(b["sd_start"][i]), 0.0,
                 float(b["time_start"][i]))
    if rc != 0:
        return rc, None
    st = p.optimize()
    if st != 0:
        return st, None
    return 0, dict(t=p.time, s=p.s, sd=p.sd, sdd=p.sdd)

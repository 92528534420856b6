"""CPU search (oracle only, no GPU) for inputs of the joint sweep on which the solver ends with
"no connection" (7), "non-zero end" (9) or "critical index zero" (10) without a loop limit.

The joint sweep (csrc/tpamd_sweep_joint.h) takes joint-spline paths and Cartesian paths. Both kinds
are drawn here from every generator the tests have -- synthetic.make_joint_batch, every family of
tests/structured_paths.py, synthetic.make_cartesian_batch, every family of tests/cartesian_paths.py --
at 3..257 samples (very short paths included), with velocity and acceleration limits scaled by
1e-3..1e2 and 1e-4..1e3, start velocities, horizons that overshoot the spline's end, control points
scaled by 1e-6..1e3 and Cartesian limits scaled by 1e-3..1e2. Prints the count of every status met
and the first inputs of each status looked for, as one JSON line.

    python tools/search_failing_statuses.py [cases [seed]]        (default 4000 cases of 32 paths)

Result on record (profiles/sweep_runahead_status_search.json): no such input in 4000 cases."""
import importlib
import json
import os
import sys
from collections import Counter

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import tpo  # noqa: E402

tpo.build()
import cartesian_paths as cp  # noqa: E402
import structured_paths as sp  # noqa: E402

syn = sp.syn
WANTED = (7, 9, 10)
SAMPLES = (3, 4, 5, 9, 17, 33, 65, 130, 257)


def scaled(b, key, f):
    b[key] = np.ascontiguousarray(np.asarray(b[key]) * f)


def joint_case(rng):
    D = int(rng.choice([3, 6, 7, 8, 14]))
    N = int(rng.choice(SAMPLES))
    fam = str(rng.choice(sp.FAMILIES + ("plain",)))
    seed = int(rng.integers(0, 50))
    b = syn.make_joint_batch(32, D, N, first_path_index=1000 * seed) if fam == "plain" \
        else sp.make_family(fam, 32, D, N, seed=seed)
    mods = {}
    if rng.random() < 0.5: mods["vmax"] = float(10 ** rng.uniform(-3, 2)); scaled(b, "vmax", mods["vmax"])
    if rng.random() < 0.5: mods["amax"] = float(10 ** rng.uniform(-4, 3)); scaled(b, "amax", mods["amax"])
    if rng.random() < 0.3: mods["sd_start"] = float(10 ** rng.uniform(-2, 1)); b["sd_start"] = np.full(32, mods["sd_start"])
    if rng.random() < 0.3: mods["overshoot"] = float(rng.uniform(1.0, 3.0)); scaled(b, "delta", mods["overshoot"])
    if rng.random() < 0.3: mods["control_points"] = float(10 ** rng.uniform(-6, 3)); scaled(b, "control_points", mods["control_points"])
    ref = sp.oracle_solve(tpo, b, N)
    return dict(kind="joint", D=D, N=N, family=fam, seed=seed, mods=mods), ref["status"]


def cartesian_case(rng):
    D = int(rng.choice([6, 7]))
    N = int(rng.choice(SAMPLES))
    fam = str(rng.choice(cp.FAMILIES + ("plain",)))
    seed = int(rng.integers(0, 50))
    if fam == "plain":
        b = syn.make_cartesian_batch(16, D, N, first_path_index=1000 * seed)
        b.setdefault("sd_start", np.zeros(16))
        b.setdefault("time_start", np.zeros(16))
    else:
        b = cp.make_family(fam, 16, D, N, seed=seed)
        if rng.random() < 0.5:
            b = cp.with_starts(b, seed=seed)
    mods = {}
    for key, lo, hi in (("vmax", -3, 2), ("amax", -4, 3), ("vtrans", -3, 2), ("vrot", -3, 2)):
        if rng.random() < 0.4:
            mods[key] = float(10 ** rng.uniform(lo, hi))
            scaled(b, key, mods[key])
    if rng.random() < 0.3: mods["overshoot"] = float(rng.uniform(1.0, 3.0)); scaled(b, "delta", mods["overshoot"])
    ref = tpo.time_cartesian_batch(b["ik_positions"], b["jacobians"], b["vmax"], b["amax"], b["vtrans"], b["vrot"],
                                   b["path_start"], b["delta"], sd_start=b.get("sd_start"),
                                   time_start=b.get("time_start"), nthreads=8)
    return dict(kind="cartesian", D=D, N=N, family=fam, seed=seed, mods=mods), ref["status"]


def main():
    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 4000
    rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
    seen = {"joint": Counter(), "cartesian": Counter()}
    found = {}
    for it in range(cases):
        what, st = (cartesian_case if it % 3 == 2 else joint_case)(rng)
        c = Counter(int(s) for s in st)
        seen[what["kind"]].update(c)
        for s in WANTED:
            if c.get(s) and len(found.get(s, [])) < 5:
                found.setdefault(s, []).append(dict(what, paths=c[s]))
    print(json.dumps({"cases": cases, "statuses_joint": dict(sorted(seen["joint"].items())),
                      "statuses_cartesian": dict(sorted(seen["cartesian"].items())),
                      "found": {str(k): v for k, v in found.items()}}))


if __name__ == "__main__":
    main()

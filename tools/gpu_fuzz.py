"""Randomised parity fuzzing of the engine against the oracle (run on the GPU box):

    python tools/gpu_fuzz.py [--check] [seconds] [seed]

Random joint counts, sample counts, batch sizes, limit scales, start velocities, ragged
batches and Cartesian batches; every path of every case must match the oracle bit for bit
(status, last extremal index, t, s, sd, sdd, q, qd, qdd). Prints one JSON summary line.

--check: the uniform joint and the Cartesian cases also run the device check of the engine's own
solution (Engine.check_joint_paths / check_cartesian_paths) and compare its violations, path by path,
with the oracle's constraint_violations() of the same path (SolutionSatisfiesConstraints,
time_optimal_path_timing.cc:492-518; -1 where the path has no solution). The summary then also holds
checked_paths and ok_paths_with_violations, the number of status-OK paths with a non-zero count.
"""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import tpo  # noqa: E402

eng = importlib.import_module("x-edr-trajectory-planning_amd.engine")
syn = importlib.import_module("x-edr-trajectory-planning_amd.synthetic")
DEV = "cuda:0"
KEYS = ("time", "s", "sd", "sdd", "qd", "qdd")


def check(out, ref, counts=None):
    st = out["status"].cpu().numpy()
    if not np.array_equal(st, ref["status"]):
        return "status"
    ok = st == 0
    if not np.array_equal(out["last_extremal_index"].cpu().numpy()[ok], ref["last_extremal_index"][ok]):
        return "lei"
    for k in KEYS:
        g = out[k].cpu().numpy()
        r = ref["t" if k == "time" else k]
        if counts is None:
            if not np.array_equal(g[ok], r[ok], equal_nan=True):
                return k
        else:
            for i in np.nonzero(ok)[0]:
                if not np.array_equal(g[i, :counts[i]], r[i][:counts[i]], equal_nan=True):
                    return k
    return None


def oracle_violations(rows, s_start, s_end, sd_start, time_start):
    """constraint_violations() of the oracle's own solve of one path (-1: no solution)."""
    N, Cn = rows[0].shape
    p = tpo.Profile(N, Cn)
    p.set_max_loops(max(100, 10 * N))
    rc = p.setup(*rows, float(s_start), float(s_end), float(sd_start), 0.0, float(time_start))
    if rc == 0:
        rc = p.optimize()
    return p.constraint_violations() if rc == 0 else -1


def check_violations(got, want, status):
    """(field name or None, number of status-OK paths with violated rows)."""
    got = got["violations"].cpu().numpy()
    bad = None if np.array_equal(got, np.asarray(want, dtype=got.dtype)) else "violations"
    return bad, int(((status == 0) & (got > 0)).sum())


def main():
    argv = [a for a in sys.argv[1:] if a != "--check"]
    do_check = len(argv) != len(sys.argv) - 1
    budget = float(argv[0]) if len(argv) > 0 else 120.0
    seed = int(argv[1]) if len(argv) > 1 else 1
    checked = violated = 0
    rng = np.random.default_rng(seed)
    E = eng.Engine(0)
    t_end = time.time() + budget
    cases = paths = 0
    failures = []
    next_note = time.time() + 30.0
    while time.time() < t_end and len(failures) < 5:
        if time.time() >= next_note:      # a progress line every half minute
            print("[fuzz] %d cases, %d paths, %d failures" % (cases, paths, len(failures)), file=sys.stderr, flush=True)
            next_note += 30.0
        kind = rng.choice(["joint", "joint", "ragged", "cartesian", "groups"])
        D = int(rng.choice([1, 2, 3, 4, 5, 6, 7, 7, 7, 8, 9, 12, 14, 16]))
        N = int(rng.choice([3, 4, 17, 63, 64, 65, 128, 500, 1000, 2000, 2108, 2109, 2999, 4000, 4217, 6000]))
        B = int(rng.integers(1, 65))
        W = int(rng.choice([2, 3, 5, 10]))
        first = int(rng.integers(0, 1 << 30))
        desc = dict(kind=str(kind), D=D, N=N, B=B, W=W, first=first)
        if kind == "groups":
            # several batches of different shape side by side on the engine's lanes
            # (tpamd_time_joint_groups_device), some of them ragged: each against its own oracle run
            G = int(rng.integers(2, 6))
            groups, refs, cnts = [], [], []
            for g in range(G):
                Dg = int(rng.choice([3, 6, 7, 7, 14, 5, 9]))
                Ng = int(rng.choice([17, 128, 500, 1000, 2000, 2500, 4000]))
                Bg = int(rng.integers(1, 33))
                bg = syn.make_joint_batch(Bg, Dg, Ng, num_waypoints=W, first_path_index=first + 1000 * g)
                bg["vmax"] = bg["vmax"] * rng.uniform(0.3, 3.0, (Bg, 1))
                ragged = Ng >= 6 and rng.uniform() < 0.5
                counts = rng.integers(3, Ng + 1, size=Bg).astype(np.int32) if ragged else None
                if ragged:
                    bg["delta"] = bg["knots"][:, -1] / (counts - 1)
                ig = eng.upload_joint_batch(bg, DEV)
                if ragged:
                    ig["num_samples_per_path"] = torch.from_numpy(counts).to(DEV)
                groups.append(dict(inputs=ig, outputs=eng.alloc_joint_outputs(Bg, Ng, Dg, DEV), num_samples=Ng))
                if ragged:
                    ref = dict(status=np.zeros(Bg, np.int32), last_extremal_index=np.zeros(Bg, np.int32),
                               **{k: [None] * Bg for k in ("t", "s", "sd", "sdd", "qd", "qdd")})
                    for i in range(Bg):
                        one = {k: bg[k][i:i + 1] for k in ("knots", "control_points", "vmax", "amax", "path_start", "delta")}
                        r1 = tpo.time_joint_batch(one["knots"], one["control_points"], one["vmax"], one["amax"],
                                                  one["path_start"], one["delta"], int(counts[i]))
                        ref["status"][i] = r1["status"][0]
                        ref["last_extremal_index"][i] = r1["last_extremal_index"][0]
                        for k in ("t", "s", "sd", "sdd", "qd", "qdd"):
                            ref[k][i] = r1[k][0]
                else:
                    ref = tpo.time_joint_batch(bg["knots"], bg["control_points"], bg["vmax"], bg["amax"],
                                               bg["path_start"], bg["delta"], Ng, nthreads=16)
                refs.append(ref)
                cnts.append(counts)
                paths += Bg
            E.time_joint_groups(groups)
            torch.cuda.synchronize()
            bad = None
            for g in range(G):
                bad = bad or check(groups[g]["outputs"], refs[g], cnts[g])
            paths -= B
        elif kind == "cartesian":
            D = min(D, 9)
            N = max(N, 3)
            b = syn.make_cartesian_batch(B, D, N, num_waypoints=W, first_path_index=first)
            b["vtrans"] = b["vtrans"] * rng.uniform(0.2, 5.0, B)
            ref = tpo.time_cartesian_batch(b["ik_positions"], b["jacobians"], b["vmax"], b["amax"], b["vtrans"],
                                           b["vrot"], b["path_start"], b["delta"], nthreads=16)
            out = eng.alloc_joint_outputs(B, N, D, DEV)
            if do_check:
                out["sd2"] = torch.empty(B, N, dtype=torch.float64, device=DEV)
            inp = syn.upload_cartesian_batch(b, DEV)
            E.time_cartesian_paths(inp, out)
            torch.cuda.synchronize()
            bad = check(out, ref)
            if do_check and not bad:
                want = []
                for i in range(B):
                    q1, q2 = tpo.cartesian_path_derivatives(b["ik_positions"][i], b["delta"][i])
                    jq1 = np.zeros((N, 6))
                    for d in range(D):             # J q', the joints added in index order
                        jq1 = jq1 + b["jacobians"][i][:, :, d] * q1[:, d:d + 1]
                    rows = tpo.cartesian_constraint_setup(q1, q2, jq1, b["vmax"][i], b["amax"][i], b["vtrans"][i],
                                                          b["vrot"][i], b["safety"])
                    want.append(oracle_violations(rows, b["path_start"][i], b["path_start"][i] + b["delta"][i] * (N - 1),
                                                  0.0, 0.0))
                bad, nz = check_violations(E.check_cartesian_paths(inp, out, safety=b["safety"]), want, ref["status"])
                checked += B
                violated += nz
        else:
            b = syn.make_joint_batch(B, D, N, num_waypoints=W, first_path_index=first)
            b["vmax"] = b["vmax"] * rng.uniform(0.2, 4.0, (B, 1))
            b["amax"] = b["amax"] * rng.uniform(0.1, 8.0, (B, 1))
            b["sd_start"] = np.where(rng.uniform(size=B) < 0.3, rng.uniform(0.0, 0.3, B), 0.0)
            b["time_start"] = rng.uniform(-5.0, 50.0, B)
            inp = eng.upload_joint_batch(b, DEV)
            out = eng.alloc_joint_outputs(B, N, D, DEV)
            if kind == "ragged" and N >= 6:
                counts = rng.integers(3, N + 1, size=B).astype(np.int32)
                b["delta"] = b["knots"][:, -1] / (counts - 1)
                inp = eng.upload_joint_batch(b, DEV)
                inp["num_samples_per_path"] = torch.from_numpy(counts).to(DEV)
                E.time_joint_paths(inp, out, N)
                torch.cuda.synchronize()
                ref = dict(status=np.zeros(B, np.int32), last_extremal_index=np.zeros(B, np.int32),
                           **{k: [None] * B for k in ("t", "s", "sd", "sdd", "qd", "qdd")})
                for i in range(B):
                    one = {k: b[k][i:i + 1] for k in ("knots", "control_points", "vmax", "amax", "path_start",
                                                      "delta", "sd_start", "time_start")}
                    r1 = tpo.time_joint_batch(one["knots"], one["control_points"], one["vmax"], one["amax"],
                                              one["path_start"], one["delta"], int(counts[i]),
                                              sd_start=one["sd_start"], time_start=one["time_start"])
                    ref["status"][i] = r1["status"][0]
                    ref["last_extremal_index"][i] = r1["last_extremal_index"][0]
                    for k in ("t", "s", "sd", "sdd", "qd", "qdd"):
                        ref[k][i] = r1[k][0]
                bad = check(out, ref, counts)
            else:
                E.time_joint_paths(inp, out, N)
                torch.cuda.synchronize()
                ref = tpo.time_joint_batch(b["knots"], b["control_points"], b["vmax"], b["amax"], b["path_start"],
                                           b["delta"], N, sd_start=b["sd_start"], time_start=b["time_start"],
                                           nthreads=16)
                bad = check(out, ref)
                if do_check and not bad:
                    sd2 = torch.empty(B, N, dtype=torch.float64, device=DEV)
                    E.time_joint_paths(inp, dict(out, sd2=sd2), N)     # the same solve, asked for sd2 as well
                    want = []
                    for i in range(B):
                        _, q1, q2 = tpo.joint_sample_path(b["knots"][i], b["control_points"][i], b["path_start"][i],
                                                          b["delta"][i], N)
                        rows = tpo.joint_constraint_setup(q1, q2, b["vmax"][i], b["amax"][i], b["safety"])
                        want.append(oracle_violations(rows, b["path_start"][i],
                                                      b["path_start"][i] + b["delta"][i] * (N - 1), b["sd_start"][i],
                                                      b["time_start"][i]))
                    bad, nz = check_violations(E.check_joint_paths(inp, dict(out, sd2=sd2), N, safety=b["safety"]),
                                               want, ref["status"])
                    checked += B
                    violated += nz
        cases += 1
        paths += B
        if bad:
            failures.append(dict(desc, field=bad))
    summary = dict(seconds=budget, seed=seed, cases=cases, paths=paths, failures=failures)
    if do_check:
        summary.update(checked_paths=checked, ok_paths_with_violations=violated)
    print(json.dumps(summary))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())

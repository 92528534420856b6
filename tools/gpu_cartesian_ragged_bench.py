"""Ragged Cartesian batches on the GPU: the measurements of profiles/cartesian_ragged_ab.md.

  --mode ragged    1024 six-joint paths with 500..4000 samples: one ragged call (strided and packed)
                   against one uniform call per distinct sample count, same engine, same run;
                   wall time and the engine's own kernel timers (tpamd_profile_*).
  --mode uniform   4096 x 6 x 2000 (BASELINE.json configs[3]) through the uniform entry: the K1 and
                   sweep means of the library TPAMD_LIBRARY selects (for an A/B of two builds).

The paths are smooth synthetic IK solutions generated on the device (sums of a sine and a ramp per
joint; the Jacobian of synthetic.make_cartesian_batch). One JSON line per mode on stdout."""
import argparse
import importlib
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"


def make_paths(torch, dev, B, D, stride, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *shape: torch.rand(*shape, generator=g, dtype=torch.float64).to(dev)
    amp, freq, phase, slope = 0.2 + 0.5 * rnd(B, D), 0.5 + 1.5 * rnd(B, D), 6.28 * rnd(B, D), 0.6 * rnd(B, D) - 0.3
    delta = 0.004 + 0.002 * rnd(B)
    s = delta[:, None] * torch.arange(stride, dtype=torch.float64, device=dev)[None, :]
    q = amp[:, None, :] * torch.sin(freq[:, None, :] * s[:, :, None] + phase[:, None, :]) + slope[:, None, :] * s[:, :, None]
    r = torch.arange(6, device=dev)[None, None, :, None]
    d = torch.arange(D, device=dev)[None, None, None, :]
    J = 0.25 * torch.sin(q[:, :, None, :] * (r + 1.0) + 0.37 * d) + (r == d % 6)
    zeros = torch.zeros(B, dtype=torch.float64, device=dev)
    return dict(ik_positions=q.contiguous(), jacobians=J.contiguous(), max_velocity=1.0 + rnd(B, D),
                max_acceleration=2.0 + 2.0 * rnd(B, D), max_translational_velocity=0.6 + 0.9 * rnd(B),
                max_rotational_velocity=0.8 + 1.2 * rnd(B), path_start=zeros, delta=delta, sd_start=zeros.clone(),
                time_start=zeros.clone())


def timed(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return dict(min_ms=min(ms), mean_ms=sum(ms) / len(ms), runs=[round(x, 3) for x in ms])


def kernel_ms(torch, E, fn):
    """Kernel time of one fn() by the engine's own event timers: total and per kernel."""
    E.profile_enable(True)
    E.profile_reset()
    fn()
    torch.cuda.synchronize()
    summary = E.profile_summary()
    E.profile_enable(False)
    per = {k: round(ms * n, 4) for k, (ms, n) in summary.items() if n}
    return dict(total_ms=round(sum(per.values()), 4), per_kernel_ms=per, launches={k: n for k, (ms, n) in summary.items() if n})


def mode_ragged(args, torch, eng):
    dev, B, D, stride = "cuda:0", args.paths, 6, 4000
    counts = np.random.default_rng(7).integers(500, stride + 1, B).astype(np.int32)
    full = make_paths(torch, dev, B, D, stride, 11)
    ns = torch.from_numpy(counts).to(dev)
    first_np = np.concatenate([[0], np.cumsum(counts[:-1])]).astype(np.int32)
    first = torch.from_numpy(first_np).to(dev)
    packed = dict(full)
    packed["ik_positions"] = torch.cat([full["ik_positions"][b, :n] for b, n in enumerate(counts)]).contiguous()
    packed["jacobians"] = torch.cat([full["jacobians"][b, :n] for b, n in enumerate(counts)]).contiguous()
    out = eng.alloc_joint_outputs(B, stride, D, dev)
    groups = []
    for n in sorted(set(counts.tolist())):
        ids = torch.from_numpy(np.nonzero(counts == n)[0]).to(dev)
        inp = {k: (v[ids, :n] if k in ("ik_positions", "jacobians") else v[ids]).contiguous() for k, v in full.items()}
        groups.append((inp, eng.alloc_joint_outputs(len(ids), n, D, dev), ids, n))
    E = eng.Engine(0)
    ragged_strided = lambda E=E: E.time_cartesian_paths(full, out, num_samples_per_path=ns)
    ragged_packed = lambda E=E: E.time_cartesian_paths(packed, out, num_samples_per_path=ns, first_row=first)

    def per_count():
        for inp, o, _, _ in groups:
            E.time_cartesian_paths(inp, o)

    res = dict(mode="ragged", paths=B, dofs=D, stride=stride, samples=int(counts.sum()),
               distinct_counts=len(groups), library=os.path.basename(eng._SO))
    for name, fn in (("per_count_loop", per_count), ("ragged_strided", ragged_strided), ("ragged_packed", ragged_packed)):
        r = timed(torch, fn, args.reps)
        r["paths_per_s"] = round(B / (r["min_ms"] * 1e-3))
        r["kernels"] = kernel_ms(torch, E, fn)
        res[name] = r
    # the three give the same bits
    ragged_packed()
    torch.cuda.synchronize()
    solved = int((out["status"] == 0).sum())
    same = True
    for inp, o, ids, n in groups:
        E.time_cartesian_paths(inp, o)
        torch.cuda.synchronize()
        for k in ("time", "sd", "sdd", "qd", "qdd"):
            same = same and bool(torch.equal(out[k][ids, :n], o[k]))
    res["solved"], res["bit_equal_to_per_count_loop"] = solved, same
    print(json.dumps(res))


def mode_uniform(args, torch, eng):
    dev, B, D, N = "cuda:0", 4096, 6, 2000
    inp = make_paths(torch, dev, B, D, N, 13)
    out = eng.alloc_joint_outputs(B, N, D, dev)
    E = eng.Engine(0)
    fn = lambda: E.time_cartesian_paths(inp, out)
    fn()
    torch.cuda.synchronize()
    E.profile_enable(True)
    E.profile_reset()
    for _ in range(args.steps):
        fn()
    torch.cuda.synchronize()
    summary = E.profile_summary()
    E.profile_enable(False)
    wall = timed(torch, fn, 10)
    print(json.dumps(dict(mode="uniform", library=os.path.basename(eng._SO), steps=args.steps,
                          solved=int((out["status"] == 0).sum()),
                          mean_ms={k: round(ms, 5) for k, (ms, n) in summary.items() if n},
                          wall_min_ms=round(wall["min_ms"], 4), wall_mean_ms=round(wall["mean_ms"], 4))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("ragged", "uniform"), default="ragged")
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--engine-module", default=None,
                    help="load the binding from this file: an older engine.py for an older library (TPAMD_LIBRARY)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    if args.engine_module:
        spec = importlib.util.spec_from_file_location("tpamd_engine_binding", args.engine_module)
        eng = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(eng)
    else:
        eng = importlib.import_module(PKG + ".engine")
    (mode_ragged if args.mode == "ragged" else mode_uniform)(args, torch, eng)


if __name__ == "__main__":
    main()

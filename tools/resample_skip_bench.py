"""Times the skip-method resampler (k_resample_skip) on the GPU.

  python tools/resample_skip_bench.py [--long]
      one library (TPAMD_LIBRARY, else the built libtpamd.so), one JSON line:
      (a) tpamd_resample_skip_device for 1024 paths x 7 joints at 2000, 8000 and 32000 samples, with a
          time step that keeps about every second sample ("half") and one that skips none ("all");
          --long adds 65536 samples, which only a library without the 32768-sample limit accepts;
      (b) steady replans of a 1024 x 7 x 1000 skip-method planner set.
  python tools/resample_skip_bench.py --ab PREVIOUS.so [--rounds 3] [--out profiles/resample_skip_ab.md]
      A/B against another build of the library, in the scheme of tools/ab_two_libraries.sh (which is
      tied to bench.py): fresh child processes, TPAMD_LIBRARY selects the .so, the two alternate.
      Writes a markdown table: per case the median of the rounds' medians and their range, so the
      range of PREVIOUS against itself is the run-to-run spread to judge a difference by.

(a) is timed with device events around each call (5 warm-up calls, 20 timed), (b) with the host clock
around plan(), which ends in a device synchronise (5 warm-up replans, 40 timed). Inputs are seeded."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
B, D = 1024, 7
SIZES = (2000, 8000, 32000)
LONG = 65536
DT = 0.004


def _stats(ms):
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def measure_resample(eng, E, torch, N, keep, warmup=5, reps=20):
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev)
    g.manual_seed(1000 + N)
    f = dict(dtype=torch.float64, device=dev)
    gaps = 0.002 + 0.002 * torch.rand(B, N, generator=g, **f)      # 2 .. 4 ms: 0.95 * DT keeps about every second
    sol = dict(time=100.0 + torch.cumsum(gaps, dim=1))
    for k in ("s", "sd", "sdd"):
        sol[k] = torch.rand(B, N, generator=g, **f)
    for k in ("q", "qd", "qdd"):
        sol[k] = torch.rand(B, N, D, generator=g, **f)
    amax = torch.ones(B, D, **f)
    start = sol["time"][:, 0].contiguous() - 0.1
    cap = N + 1
    out = {k: torch.zeros(B, cap, **f) for k in ("out_time", "out_s", "out_sd", "out_sdd")}
    out.update({k: torch.zeros(B, cap, D, **f) for k in ("out_q", "out_qd", "out_qdd")})
    out["count"] = torch.zeros(B, dtype=torch.int32, device=dev)
    dt = DT if keep == "half" else 1e-6
    ms = []
    for i in range(warmup + reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        E.resample_uniform(sol, amax, start, dt, out, skip=True)
        b.record()
        b.synchronize()
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    kept = float(out["count"].double().mean()) - 1.0
    r = _stats(ms)
    r.update(samples=N, keep=keep, kept_fraction=kept / N,
             # the time stamps once, every kept sample's 4 + 3 D doubles in and out
             gbytes=B * (N * 8 + kept * (4 + 3 * D) * 16) / 1e9)
    return r


def measure_replan(eng, E, torch, warmup=5, reps=40):
    import numpy as np
    N, W, MS = 1000, 6, 1_000_000
    rng = np.random.default_rng(20261019)
    wps = rng.uniform(-2.5, 2.5, size=(B * W, D))
    offsets = (W * np.arange(B + 1)).astype(np.int32)
    vmax, amax = rng.uniform(1.0, 2.0, size=(B, D)), rng.uniform(2.0, 4.0, size=(B, D))
    ms = []
    with eng.PlannerSet(E, B, D, N, num_points=3 * W - 2, time_step_ns=4 * MS, sampling_method=1) as ps:
        status, _ = ps.set_waypoints(wps, offsets, vmax, amax, np.full(B, 0.005))
        assert (status == 0).all()
        start = 1000 * MS
        ps.plan(start, 500 * MS)
        ok = 0
        for i in range(warmup + reps):
            start += 20 * MS
            t0 = time.perf_counter()
            summary = ps.plan(start, 500 * MS)
            t1 = time.perf_counter()
            if i >= warmup:
                ms.append(1e3 * (t1 - t0))
                ok += int((summary["status"] == 0).sum())
        r = _stats(ms)
        r.update(planners_ok=ok / reps, history=float(summary["history_count"].double().mean()),
                 trajectory=float(summary["num_samples"].double().mean()))
    return r


def child(args):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("resample_skip_bench needs a GPU")
    eng = importlib.import_module(PKG + ".engine")
    E = eng.Engine(0)
    res = dict(library=os.path.basename(eng._SO), resample=[], replan=None)
    for N in ((LONG,) if args.long else SIZES):
        for keep in ("half", "all"):
            res["resample"].append(measure_resample(eng, E, torch, N, keep))
            torch.cuda.empty_cache()
    if not args.long:
        res["replan"] = measure_replan(eng, E, torch)
    print(json.dumps(res))


def _run(lib, extra=()):
    env = dict(os.environ, TPAMD_LIBRARY=lib)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(extra), env=env, capture_output=True,
                         text=True, timeout=900)
    if out.returncode != 0:
        sys.stderr.write(out.stderr[-3000:])
        raise SystemExit("child failed for " + lib)
    return json.loads(out.stdout.strip().splitlines()[-1])


def ab(args):
    this = os.environ.get("TPAMD_LIBRARY") or os.path.join(ROOT, PKG, "csrc", "libtpamd.so")
    prev = os.path.abspath(args.ab)
    runs = {"this": [], "previous": []}
    for _ in range(args.rounds):
        for name, lib in (("this", this), ("previous", prev)):
            runs[name].append(_run(lib))
            print(name, json.dumps(runs[name][-1]), flush=True)
    long_run = _run(this, ["--long"])
    print("this --long", json.dumps(long_run), flush=True)

    def cell(values):
        return "%.3f (%.3f .. %.3f)" % (statistics.median(values), min(values), max(values))

    lines = ["| case | kept | this build, ms | previous build, ms | previous / this |", "|---|---|---|---|---|"]
    for i, c in enumerate(runs["this"][0]["resample"]):
        t = [r["resample"][i]["median"] for r in runs["this"]]
        p = [r["resample"][i]["median"] for r in runs["previous"]]
        lines.append("| resample %d x %d x %d, %s | %.2f | %s | %s | %.2f |" % (
            B, D, c["samples"], c["keep"], c["kept_fraction"], cell(t), cell(p),
            statistics.median(p) / statistics.median(t)))
    t = [r["replan"]["median"] for r in runs["this"]]
    p = [r["replan"]["median"] for r in runs["previous"]]
    lines.append("| replan of a %d x %d x 1000 set | - | %s | %s | %.2f |" % (
        B, D, cell(t), cell(p), statistics.median(p) / statistics.median(t)))
    for c in long_run["resample"]:
        lines.append("| resample %d x %d x %d, %s | %.2f | %.3f (%.3f .. %.3f) | not accepted | - |" % (
            B, D, c["samples"], c["keep"], c["kept_fraction"], c["median"], c["min"], c["max"]))
    lines.append("")
    lines.append("Memory traffic of the resample cases (time stamps once, kept samples in and out), GB per call: " +
                 ", ".join("%d %s %.2f" % (c["samples"], c["keep"], c["gbytes"])
                           for c in runs["this"][0]["resample"] + long_run["resample"]) + ".")
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--long", action="store_true")
    ap.add_argument("--ab", metavar="PREVIOUS.so")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    ab(a) if a.ab else child(a)

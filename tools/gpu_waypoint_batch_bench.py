"""Waypoint batches on the GPU: the measurements of profiles/waypoint_batch_ab.md.

1024 seven-joint paths, 2..12 waypoints each (fixed seed), 2000 samples each, every path sampled over
its whole length. Same build, same process, same engine:

  A  the way without the waypoint entries: every path fitted on the host (the oracle's fit, one call
     per path), delta = path_end / (N - 1) on the host, the batch bucketed by control-point count and
     all groups timed by one tpamd_time_joint_groups_host call;
  B  tpamd_time_waypoint_paths_host on the waypoints, and tpamd_time_waypoint_paths_device with the
     waypoints and limits already resident.

Every path's outputs are compared bit for bit between A and both forms of B before a number is
printed. Wall time is a host clock around calls that end in a synchronise, warm-up first, A and B
alternating; medians with min and max. Kernel time is the engine's own event timers
(tpamd_profile_*: set-up, sampling/LP and sweep spans), taken in passes of their own, plus the fit
call timed by events around Engine.fit_joint_waypoints on resident waypoints (it allocates its zeroed
outputs, copies the offsets up and runs the kernel, so it bounds the kernel from above). Launches and
PCIe bytes are counted from the shapes. One JSON line on stdout; --markdown PATH also writes the table."""
import argparse
import datetime
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
ROWS = ("time", "s", "sd", "sdd", "q", "qd", "qdd")


def make_batch(B, D, seed):
    rng = np.random.default_rng(seed)
    counts = rng.integers(2, 13, B)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(counts=counts, offsets=offsets, waypoints=rng.uniform(-1.0, 1.0, size=(int(offsets[-1]), D)),
                vmax=rng.uniform(0.5, 2.0, size=(B, D)), amax=rng.uniform(0.5, 2.0, size=(B, D)))


def host_outputs(B, N, D):
    out = {k: np.zeros((B, N)) for k in ("time", "s", "sd", "sdd")}
    out.update({k: np.zeros((B, N, D)) for k in ("q", "qd", "qdd")})
    out.update(status=np.full(B, -1, dtype=np.int32), last_extremal_index=np.zeros(B, dtype=np.int32))
    return out


class RunA:
    """Host fit, bucket by control-point count, one groups call. The group arrays are allocated once."""

    def __init__(self, tpo, E, b, N, D):
        self.tpo, self.E, self.b, self.N, self.D = tpo, E, b, N, D
        npts = 3 * b["counts"] - 2
        self.ids = {int(P): np.flatnonzero(npts == P) for P in sorted(set(npts.tolist()))}
        self.groups = []
        for P, ids in self.ids.items():
            n = len(ids)
            inp = dict(knots=np.zeros((n, P + 3)), control_points=np.zeros((n, P, D)),
                       max_velocity=np.ascontiguousarray(b["vmax"][ids]), max_acceleration=np.ascontiguousarray(b["amax"][ids]),
                       path_start=np.zeros(n), delta=np.zeros(n), sd_start=np.zeros(n), time_start=np.zeros(n))
            self.groups.append(dict(inputs=inp, outputs=host_outputs(n, N, D), num_samples=N))
        self.fit_ms = self.call_ms = 0.0

    def __call__(self):
        t0 = time.perf_counter()
        b, off = self.b, self.b["offsets"]
        for g, ids in zip(self.groups, self.ids.values()):
            for i, k in enumerate(ids):
                cps, knots = self.tpo.joint_fit_spline(b["waypoints"][off[k]:off[k + 1]], 0.2)
                g["inputs"]["knots"][i], g["inputs"]["control_points"][i] = knots, cps
                g["inputs"]["delta"][i] = knots[-1] / np.float64(self.N - 1)
        t1 = time.perf_counter()
        self.E.time_joint_groups(self.groups, host=True)
        t2 = time.perf_counter()
        self.fit_ms, self.call_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3

    def gathered(self):
        B = len(self.b["counts"])
        out = host_outputs(B, self.N, self.D)
        for g, ids in zip(self.groups, self.ids.values()):
            for k, v in g["outputs"].items():
                out[k][ids] = v
        return out

    def pcie_bytes(self):
        up = sum(sum(v.nbytes for v in g["inputs"].values()) for g in self.groups)
        down = sum(sum(v.nbytes for v in g["outputs"].values()) for g in self.groups)
        return up, down


def stats(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4))


def kernel_spans(torch, E, fn):
    E.profile_enable(True)
    E.profile_reset()
    fn()
    torch.cuda.synchronize()
    summary = E.profile_summary()
    E.profile_enable(False)
    per = {k: round(ms * n, 4) for k, (ms, n) in summary.items() if n}
    return round(sum(per.values()), 4), int(sum(n for _, n in summary.values())), per


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--markdown", default=None)
    ap.add_argument("--commit", default="(working tree)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("needs a GPU")
    eng = importlib.import_module(PKG + ".engine")
    from oracle import tpo
    tpo.build()
    dev, B, D, N = torch.device("cuda", 0), args.paths, 7, args.samples
    b = make_batch(B, D, 2025)
    E = eng.Engine(0)
    run_a = RunA(tpo, E, b, N, D)
    out_h = host_outputs(B, N, D)
    out_h.update(num_points=np.zeros(B, dtype=np.int32), path_end=np.zeros(B), delta_used=np.zeros(B))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    w_d, vm_d, am_d = up(b["waypoints"]), up(b["vmax"]), up(b["amax"])
    out_d = {k: up(v) for k, v in out_h.items()}
    b_host = lambda: E.time_waypoint_paths(b["waypoints"], b["offsets"], b["vmax"], b["amax"], N, outputs=out_h, host=True)

    def b_device():
        E.time_waypoint_paths(w_d, b["offsets"], vm_d, am_d, N, outputs=out_d)
        torch.cuda.synchronize()

    # the same bits first
    run_a(); b_host(); b_device()
    ref = run_a.gathered()
    solved = int((ref["status"] == 0).sum())
    same = dict(host=True, device=True)
    for k in ROWS + ("status", "last_extremal_index"):
        same["host"] = same["host"] and ref[k].tobytes() == out_h[k].tobytes()
        same["device"] = same["device"] and ref[k].tobytes() == out_d[k].cpu().numpy().tobytes()
    if not (same["host"] and same["device"]):
        raise SystemExit("A and B differ: %s" % same)

    runs = dict(A=run_a, B_host=b_host, B_device=b_device)
    wall = {k: [] for k in runs}
    a_fit, a_call = [], []
    for step in range(args.warmup + args.steps):
        for name, fn in runs.items():            # alternating
            t0 = time.perf_counter()
            fn()
            ms = (time.perf_counter() - t0) * 1e3
            if step >= args.warmup:
                wall[name].append(ms)
                if name == "A":
                    a_fit.append(run_a.fit_ms)
                    a_call.append(run_a.call_ms)
    # kernel time: the engine's event timers, and the fit kernel by events of its own
    kern = {name: kernel_spans(torch, E, fn) for name, fn in runs.items()}
    fit_ms = []
    for _ in range(args.warmup + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        E.fit_joint_waypoints(w_d, b["offsets"])
        e1.record()
        torch.cuda.synchronize()
        fit_ms.append(e0.elapsed_time(e1))
    fit_kernel_ms = round(statistics.median(fit_ms[args.warmup:]), 4)
    out_bytes = sum(out_h[k].nbytes for k in ROWS + ("status", "last_extremal_index"))
    fit_out = sum(out_h[k].nbytes for k in ("num_points", "path_end", "delta_used"))
    a_up, a_down = run_a.pcie_bytes()
    pcie = dict(A=dict(h2d=a_up, d2h=a_down),
                B_host=dict(h2d=b["waypoints"].nbytes + b["vmax"].nbytes + b["amax"].nbytes + b["offsets"].nbytes,
                            d2h=out_bytes + fit_out),
                B_device=dict(h2d=b["offsets"].nbytes, d2h=0))
    G = len(run_a.groups)
    # per solve at 7 joints: set-up, sampling/LP, sweep (which runs the boundary passes and the epilogue)
    launches = dict(A=3 * G, B_host=4, B_device=4)
    res = dict(paths=B, dofs=D, samples=N, waypoints="2..12", groups_in_A=G, solved=solved, bit_equal=same,
               steps=args.steps, warmup=args.warmup, wall={k: stats(v) for k, v in wall.items()},
               A_host_fit=stats(a_fit), A_engine_call=stats(a_call),
               kernel_ms={k: dict(solve_spans_ms=v[0], timed_spans=v[1], per_kernel=v[2]) for k, v in kern.items()},
               fit_kernel_ms=fit_kernel_ms, launches=launches, pcie_bytes=pcie)
    print(json.dumps(res))
    if args.markdown:
        with open(args.markdown, "w") as f:
            f.write("# Waypoint batches: host fit + one group per control-point count (A) against one call (B)\n\n")
            f.write("Commit %s, %s, MI355X, `tools/gpu_waypoint_batch_bench.py --paths %d --samples %d --warmup %d "
                    "--steps %d`.\n\n" % (args.commit, datetime.date.today().isoformat(), B, N, args.warmup, args.steps))
            f.write("%d seven-joint paths, 2..12 waypoints (seed 2025), %d samples each over the whole path; %d solved; "
                    "outputs of A, B host and B device bit-equal: %s. A needs %d groups. Wall time: host clock around "
                    "calls that end in a synchronise, A and B alternating, median [min .. max] of %d steps after %d "
                    "warm-up steps. Kernel time: the engine's event timers over one call (solve kernels); the fit call "
                    "by events around Engine.fit_joint_waypoints on resident waypoints (median; output allocation, "
                    "offsets copy and kernel: an upper bound of the kernel). Launches and PCIe bytes are counted from "
                    "the shapes.\n\n" % (B, N, solved, same["host"] and same["device"], G, args.steps, args.warmup))
            f.write("| run | wall per batch (ms) | solve kernels (ms) | fit call (ms) | launches | PCIe up (bytes) | PCIe down (bytes) |\n")
            f.write("|---|---|---|---|---|---|---|\n")
            names = dict(A="A: host fit + groups_host", B_host="B: time_waypoint_paths_host",
                         B_device="B: time_waypoint_paths_device, inputs resident")
            for k in ("A", "B_host", "B_device"):
                w = res["wall"][k]
                f.write("| %s | %.3f [%.3f .. %.3f] | %.3f | %s | %d | %d | %d |\n" % (
                    names[k], w["median_ms"], w["min_ms"], w["max_ms"], kern[k][0],
                    "host" if k == "A" else "%.4f" % fit_kernel_ms, launches[k], pcie[k]["h2d"], pcie[k]["d2h"]))
            f.write("\nOf A's wall time the host fit (oracle, one call per path from Python) takes %.3f ms [%.3f .. %.3f] "
                    "and the engine call %.3f ms [%.3f .. %.3f].\n" % (
                        res["A_host_fit"]["median_ms"], res["A_host_fit"]["min_ms"], res["A_host_fit"]["max_ms"],
                        res["A_engine_call"]["median_ms"], res["A_engine_call"]["min_ms"], res["A_engine_call"]["max_ms"]))


if __name__ == "__main__":
    main()

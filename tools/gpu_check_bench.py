"""Measures the solution check on the GPU and writes profiles/check_solutions_ab.md:

    python tools/gpu_check_bench.py [--paths 1024] [--repeats 31] [--out profiles/check_solutions_ab.md]

  joint check   1024 x 7 x 2000 after a solve: device time (HIP events) of Engine.check_joint_paths
                next to the sampling/LP kernel's time for the same batch (tpamd_profile_mean_ms), and
                next to what it replaces: downloading the solution and counting on the host with the
                oracle's rows, on one thread and on 16 (timed on a slice of the batch, scaled)
  rows check    1024 x 2000 x 14: bytes read over device time, with a device-to-device copy of the
                same number of bytes timed in the same run as the yardstick
Every device figure is the median of `repeats` event-timed calls after 5 warm-up calls, all in one
process. The counts of the device check are compared with the host's on the timed slice."""
import argparse
import datetime
import importlib
import os
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from oracle import tpo  # noqa: E402

eng = importlib.import_module("x-edr-trajectory-planning_amd.engine")
syn = importlib.import_module("x-edr-trajectory-planning_amd.synthetic")
DEV = "cuda:0"
KT = 2.220446049250313e-16 * 1e5
KI_SAMPLE_LP = 1


def device_ms(fn, repeats, warmup=5):
    """Median, min and max of the event-timed durations of fn() in milliseconds."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), float(np.min(ms)), float(np.max(ms))


def host_count(batch, i, N, sd2, sdd):
    _, q1, q2 = tpo.joint_sample_path(batch["knots"][i], batch["control_points"][i], batch["path_start"][i],
                                      batch["delta"][i], N)
    A, B, lo, hi = tpo.joint_constraint_setup(q1, q2, batch["vmax"][i], batch["amax"][i], batch["safety"])
    v = A * sdd[:, None] + B * sd2[:, None]
    return int(((v + KT < lo) | (v - KT > hi)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=31)
    ap.add_argument("--host-paths", type=int, default=128)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "check_solutions_ab.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gpu_check_bench needs a GPU")
    if args.repeats < 15:
        raise SystemExit("at least 15 repeats")
    B, D, N = args.paths, 7, 2000
    E = eng.Engine(0)
    lines = []

    # ---- joint check
    batch = syn.make_joint_batch(B, D, N)
    inp = eng.upload_joint_batch(batch, DEV)
    out = eng.alloc_joint_outputs(B, N, D, DEV)
    out["sd2"] = torch.empty(B, N, dtype=torch.float64, device=DEV)
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    E.profile_enable(True)
    E.profile_reset()
    for _ in range(args.repeats):
        E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    lp_ms, lp_n = E.profile_mean_ms(KI_SAMPLE_LP)
    E.profile_enable(False)
    rec = {k: torch.empty(B, dtype=torch.float64 if k == "worst_excess" else torch.int32, device=DEV)
           for k in ("violations", "worst_excess", "worst_sample", "worst_row", "first_sample")}
    joint = device_ms(lambda: E.check_joint_paths(inp, out, N, outputs=rec), args.repeats)
    viol = rec["violations"].cpu().numpy()
    status = out["status"].cpu().numpy()
    # what the check replaces: the solution comes down, the host forms the rows and counts
    H = min(args.host_paths, B)
    t0 = time.perf_counter()
    sd2, sdd = out["sd2"].cpu().numpy(), out["sdd"].cpu().numpy()
    t_down = time.perf_counter() - t0
    t0 = time.perf_counter()
    one = [host_count(batch, i, N, sd2[i], sdd[i]) for i in range(H)]
    t_one = (time.perf_counter() - t0) * B / H
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=16) as pool:
        many = list(pool.map(lambda i: host_count(batch, i, N, sd2[i], sdd[i]), range(H)))
    t_many = (time.perf_counter() - t0) * B / H
    agree = all(status[i] != 0 or viol[i] == one[i] == many[i] for i in range(H))
    lines += [
        "## Joint check, %d x %d x %d, after a solve" % (B, D, N), "",
        "| what | time |", "|---|---|",
        "| `check_joint_paths`, device (median of %d; min, max) | %.4f ms (%.4f, %.4f) |" % ((args.repeats,) + joint),
        "| sampling/LP kernel of the solve of the same batch (`tpamd_profile_mean_ms`, %d launches) | %.4f ms |" % (lp_n, lp_ms),
        "| download of sd2 and sdd, %.1f MB | %.1f ms |" % (2 * B * N * 8 / 1e6, 1e3 * t_down),
        "| host count with the oracle's rows, 1 thread (%d paths timed, scaled to %d) | %.0f ms |" % (H, B, 1e3 * t_one),
        "| the same on 16 threads | %.0f ms |" % (1e3 * t_many), "",
        "Status-OK paths: %d of %d; of them with violated rows: %d. Device and host counts agree on the %d timed "
        "paths: %s." % (int((status == 0).sum()), B, int(((status == 0) & (viol > 0)).sum()), H, "yes" if agree else "NO"),
        "",
    ]
    lines += ["Check over sampling/LP kernel: %.2f." % (joint[0] / lp_ms), ""]

    # ---- rows check
    Cn = 14
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    rows = {k: torch.rand(B, N, Cn, dtype=torch.float64, device=DEV, generator=g) for k in ("a", "b")}
    rows["lower"] = -torch.rand(B, N, Cn, dtype=torch.float64, device=DEV, generator=g) - 3.0
    rows["upper"] = torch.rand(B, N, Cn, dtype=torch.float64, device=DEV, generator=g) + 3.0
    sol = dict(sd2=torch.rand(B, N, dtype=torch.float64, device=DEV, generator=g),
               sdd=torch.rand(B, N, dtype=torch.float64, device=DEV, generator=g))
    nbytes = 4 * B * N * Cn * 8
    rows_ms = device_ms(lambda: E.check_rows(rows, sol, outputs=rec), args.repeats)
    src = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    copy_ms = device_ms(lambda: dst.copy_(src), args.repeats)
    lines += [
        "## Rows check, %d x %d x %d" % (B, N, Cn), "",
        "| what | time | rate |", "|---|---|---|",
        "| `check_rows`, device: %.3f GB of rows read (median of %d; min, max) | %.4f ms (%.4f, %.4f) | %.0f GB/s read |"
        % ((nbytes / 1e9, args.repeats) + rows_ms + (nbytes / 1e6 / rows_ms[0],)),
        "| device-to-device copy of %.3f GB, same run (reads and writes that many bytes) | %.4f ms (%.4f, %.4f) | "
        "%.0f GB/s read + %.0f GB/s written |"
        % ((nbytes / 1e9,) + copy_ms + (nbytes / 1e6 / copy_ms[0], nbytes / 1e6 / copy_ms[0])), "",
        "sd2 and sdd add %.1f MB (1 / %d of the rows) and are not counted." % (2 * B * N * 8 / 1e6, 2 * Cn), "",
    ]

    try:
        commit = args.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], text=True,
                                         stderr=subprocess.DEVNULL).strip()
    except Exception:
        commit = "unknown (not a git checkout)"
    head = ["# Solution check: measurements", "",
            "%s, %s, commit %s plus the working tree, one process, one build; `tools/gpu_check_bench.py --paths %d --repeats %d`. "
            "The joint kernel is the runtime-D one (no D-templated instances were written)."
            % (datetime.date.today().isoformat(), torch.cuda.get_device_name(0), commit, B, args.repeats), ""]
    text = "\n".join(head + lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

"""Cartesian goals on the device against the per-path host loop ("Cartesian goals").

  python3 tools/gpu_ik_targets_bench.py [--out profiles/ik_targets_bench.json] [--paths 1024]

The README's Cartesian-set shape: 1024 paths, D = 7, N = 1000, six pose waypoints per path, delta
chosen per path so that its IK table has 4 250 rows (round(path_end / delta) = 3 249).
  1. device fit (Engine.fit_pose_waypoints on CUDA tensors): HIP events around the call;
  2. device targets (Engine.sample_ik_targets into CUDA tensors): HIP events around the call, and
     the bytes the kernel has to store, (7 + D) * 8 per row, over that time;
  3. both end to end into device memory: fit, path_end down, row counts on the host, targets; host
     clock around work that ends in a device synchronise;
  4. the comparison: tools/ik_targets_host_loop.cc, the unchanged mirror's way of getting the same
     arrays -- per path TimeableCartesianSplinePath::SetWaypoints and the target part of
     ExtendIkSolution (pose sampler with num_paths = 1 plus the host EvalCurve loop), in a loop over
     the paths on one thread.
Every stage is warmed up first; the device stages repeat 50 times (median, min and max reported), the
host loop three times. Needs a GPU: there is no fallback.
"""
import argparse
import importlib
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
HBM_PEAK_GBS = 8000.0           # MI355X HBM3E


def make_goals(B, D, W, seed=1024):
    rng = np.random.default_rng(seed)
    t = np.cumsum(rng.uniform(-0.3, 0.3, (B, W, 3)), axis=1) + rng.uniform(-0.5, 0.5, (B, 1, 3))
    q = rng.standard_normal((B, W, 4))
    q /= np.linalg.norm(q, axis=2, keepdims=True)
    joints = np.cumsum(rng.uniform(-0.5, 0.5, (B, W, D)), axis=1)
    return np.ascontiguousarray(np.concatenate([t, q], axis=2)), np.ascontiguousarray(joints)


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(np.min(ms)), max_ms=float(np.max(ms)), repeats=len(ms))


def device_stages(B, D, N, W, rows_per_path, reps=50, warmup=5):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError("gpu_ik_targets_bench needs a GPU")
    eng = importlib.import_module(PKG + ".engine")
    eng.build_library()
    E = eng.Engine(0)
    dev = torch.device("cuda", 0)
    pose, joints = make_goals(B, D, W)
    off = (np.arange(B + 1) * W).astype(np.int32)
    d_pose, d_joints = torch.from_numpy(pose.reshape(-1, 7)).to(dev), torch.from_numpy(joints.reshape(-1, D)).to(dev)
    tr = torch.full((B,), 0.05, dtype=torch.float64, device=dev)
    rr = torch.full((B,), 0.2, dtype=torch.float64, device=dev)
    fit = E.fit_pose_waypoints(d_pose, d_joints, off, tr, rr)
    path_end = fit["path_end"].cpu().numpy()
    assert (fit["status"].cpu().numpy() == 0).all()
    delta = path_end / (rows_per_path - N - 1)
    d_delta = torch.from_numpy(delta).to(dev)

    def row_offsets_of(pe):
        rows = [E.ik_table_rows(pe[k], delta[k], N) for k in range(B)]
        return np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)

    ro = row_offsets_of(path_end)
    total = int(ro[-1])
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        for _ in range(warmup):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(reps):
            ev[0].record()
            fn()
            ev[1].record()
            ev[1].synchronize()
            out.append(ev[0].elapsed_time(ev[1]))
        return out

    fit_ms = timed(lambda: E.fit_pose_waypoints(d_pose, d_joints, off, tr, rr))
    tgt_ms = timed(lambda: E.sample_ik_targets(fit, d_delta, ro))

    def chain():
        f = E.fit_pose_waypoints(d_pose, d_joints, off, tr, rr)
        r = row_offsets_of(f["path_end"].cpu().numpy())
        out = E.sample_ik_targets(f, d_delta, r)
        torch.cuda.synchronize()
        return out

    for _ in range(warmup):
        chain()
    chain_ms = []
    for _ in range(reps):
        t0 = time.perf_counter()
        chain()
        chain_ms.append(1e3 * (time.perf_counter() - t0))
    store_bytes = total * (7 + D) * 8
    res = dict(paths=B, dofs=D, num_samples=N, waypoints_per_path=W, rows=total, rows_per_path=float(total) / B,
               control_points_per_path=3 * W - 2, fit=stats(fit_ms), targets=stats(tgt_ms), end_to_end=stats(chain_ms),
               target_store_bytes=store_bytes)
    res["targets"]["store_gb_per_s"] = store_bytes / (res["targets"]["median_ms"] * 1e-3) / 1e9
    res["targets"]["share_of_hbm_peak"] = res["targets"]["store_gb_per_s"] / HBM_PEAK_GBS
    return res, (pose, joints, delta)


def host_loop(B, D, N, W, goals, repeats=3):
    pose, joints, delta = goals
    host = os.path.join(ROOT, PKG, "host")
    csrc = os.path.join(ROOT, PKG, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    with tempfile.TemporaryDirectory() as tmp:
        exe, inp = os.path.join(tmp, "ik_targets_host_loop"), os.path.join(tmp, "goals.bin")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
                               os.path.join(ROOT, "tools", "ik_targets_host_loop.cc"), "-L" + host, "-ltp_host",
                               "-L" + csrc, "-ltpamd", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc])
        with open(inp, "wb") as f:
            f.write(struct.pack("<iiii", B, D, N, W))
            for b in range(B):
                f.write(struct.pack("<d", float(delta[b])))
                f.write(pose[b].astype("<f8").tobytes())
                f.write(joints[b].astype("<f8").tobytes())
        out = subprocess.run([exe, inp, str(repeats)], capture_output=True, text=True, timeout=1500)
        sys.stderr.write(out.stderr[-2000:])
        if out.returncode != 0:
            raise RuntimeError("ik_targets_host_loop failed: %s" % out.stdout[-2000:])
        return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--paths", type=int, default=1024)
    ap.add_argument("--device-only", action="store_true")
    a = ap.parse_args()
    B, D, N, W, rows = a.paths, 7, 1000, 6, 4250
    res, goals = device_stages(B, D, N, W, rows)
    if not a.device_only:
        res["host_loop"] = host_loop(B, D, N, W, goals)
        res["host_loop"]["same_rows"] = res["host_loop"]["rows"] == res["rows"]
        res["speedup_end_to_end"] = res["host_loop"]["loop_ms_median"] / res["end_to_end"]["median_ms"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

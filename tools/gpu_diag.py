"""Diagnostic build run: where do the sweep kernel's cycles go? (not a timing run)
Slots: csrc/tpamd_sweep_joint.h JointSweep::diag / diagx; 0..31 backward wave, 32..63 forward wave.
DIAG_SO names another library of csrc/ (the light form: -DTPAMD_DIAG -DTPAMD_DIAG_LIGHT)."""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
eng = importlib.import_module("x-edr-trajectory-planning_amd.engine")
syn = importlib.import_module("x-edr-trajectory-planning_amd.synthetic")
eng._SO = os.path.join(ROOT, "x-edr-trajectory-planning_amd", "csrc", os.environ.get("DIAG_SO", "libtpamd_diag.so"))
B, D, N = int(os.environ.get("DIAG_B", 1024)), int(os.environ.get("DIAG_D", 7)), int(os.environ.get("DIAG_N", 2000))
E = eng.Engine(0)
b = syn.make_joint_batch(B, D, N)
inp = eng.upload_joint_batch(b, "cuda:0")
out = eng.alloc_joint_outputs(B, N, D, "cuda:0")
for _ in range(3):
    E.time_joint_paths(inp, out, N)
torch.cuda.synchronize()
d = E.debug_diag(B).astype(np.float64)
names = ["extremal cycles (loop)", None, "crit search", "tail", "chain-block cycles",
         "first pair + loop", "chain blocks", "crit mismatches (must be 0)", "boundary-follow blocks",
         "first pair cycles", "scalar FindSdd steps", "loops", "tile fills", "fills w/o prefetch",
         "chain steps accepted", "whole kernel after set-up", "tail: sd/dt pass",
         "tail: time integral | lei+remaining qd/qdd", "literal crit walk (diag only)",
         "boundary: flags loaded (cum.)", "boundary: +zfit (cum.)", "boundary: +detect (cum.)", "boundary: +final (cum.)", "boundary: final re-fit cycles", "scalar-step cycles", "boundary-follow cycles", "init_carry cycles", "tile fills", "tile-fill cycles", "init_carry calls", "blocks from a guessed constraint"]
names[12] = "qd/qdd inside the loop"
names[13] = "tail: up to the sd/dt pass"
print("%-30s %38s | %38s" % ("B=%d D=%d N=%d" % (B, D, N), "backward wave (mean/min/max)", "forward wave (mean/min/max)"))
for k, n in enumerate(names):
    if n is None:
        continue
    a, f = d[:, k], d[:, 32 + k]
    print("%-30s %12.0f %12.0f %12.0f | %12.0f %12.0f %12.0f" % (n, a.mean(), a.min(), a.max(), f.mean(), f.min(), f.max()))
# (the literal walk of the diagnostic build runs in the forward wave since the search moved there)
net = d[:, 32 + 15] - d[:, 32 + 18]
print("whole kernel minus the literal walk (forward wave): mean %.0f min %.0f max %.0f" % (net.mean(), net.min(), net.max()))

# The loop queue (JointSweep::diagx): what the forward wave waited for, by cause, how deep the queue was
# when the backward wave took an entry, and who was first at (sd2[icrit+1], sdd[icrit]).
xx = E.debug_diag_ext(B).astype(np.float64)
x, f = xx[:, :16], xx[:, 16:32]
for k, n in enumerate(("a rare branch reads next to the switching point (hazards 1 and 2)",
                       "marks in an earlier first-step footprint (hazard 3)", "ring full")):
    print("forward wave waits, %-66s %9.0f cycles per path (max %9.0f), %7.3f waits per path, paths with one %d"
          % (n, f[:, k].mean(), f[:, k].max(), f[:, 9 + k].mean(), int((f[:, 9 + k] > 0).sum())))
print("forward wave at the final join %.0f cycles per path (max %.0f); backward wave %.0f (max %.0f)"
      % (f[:, 4].mean(), f[:, 4].max(), x[:, 7].mean(), x[:, 7].max()))
print("backward wave waiting for an entry %.0f cycles per path (max %.0f), %.1f waits per path"
      % (x[:, 0].mean(), x[:, 0].max(), x[:, 9].mean()))
taken = np.maximum(x[:, 1:5].sum(axis=1), 1)
print("entries taken per path %.1f; queue depth at the take 1: %.2f  2: %.2f  3: %.2f  4: %.2f per path (totals %s)"
      % (taken.mean(), x[:, 1].mean(), x[:, 2].mean(), x[:, 3].mean(), x[:, 4].mean(), [int(v) for v in x[:, 1:5].sum(axis=0)]))
print("entries found forward first at the end of the backward first step %.2f per path (total %d; the forward wave counted %d), backward first %.2f (total %d)"
      % (x[:, 5].mean(), int(x[:, 5].sum()), int(f[:, 5].sum()), x[:, 6].mean(), int(x[:, 6].sum())))
print("emit_range trips started inside loops %.1f" % x[:, 8].mean())
st = out["status"].cpu().numpy()
print("statuses:", {int(k): int((st == k).sum()) for k in np.unique(st)})

# per-path cycles of the whole kernel (the launch lasts as long as its slowest path): histogram for
# profiles/ (DIAG_HIST=path.json)
if os.environ.get("DIAG_HIST"):
    import json
    edges = np.linspace(net.min(), net.max(), 25)
    hist, _ = np.histogram(net, bins=edges)
    loops = d[:, 32 + 11]
    json.dump({"paths": B, "dofs": D, "samples": N, "cycles_per_path": {"mean": float(net.mean()), "min": float(net.min()),
               "p50": float(np.percentile(net, 50)), "p90": float(np.percentile(net, 90)), "p99": float(np.percentile(net, 99)),
               "max": float(net.max())}, "histogram_edges": [float(x) for x in edges], "histogram_counts": [int(x) for x in hist],
               "switching_point_loops": {"mean": float(loops.mean()), "min": float(loops.min()), "max": float(loops.max())},
               "correlation_cycles_vs_loops": float(np.corrcoef(net, loops)[0, 1]),
               "idle_share_of_a_one_round_launch": float(1.0 - net.mean() / net.max())},
              open(os.environ["DIAG_HIST"], "w"), indent=1)

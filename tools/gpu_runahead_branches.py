"""Which branches of the sweep's loop queue do the inputs of tests/test_gpu_sweep_runahead.py take?
Runs the diagnostic library (DIAG_SO, default the light form libtpamd_diaglight.so: -DTPAMD_DIAG
-DTPAMD_DIAG_LIGHT) over tests/runahead_cases.py and sums the queue counters (JointSweep::diagx)
per batch and over all of them. Counts, not timings; which wave is first differs from run to run.
    python tools/gpu_runahead_branches.py [repeats]"""
import importlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
eng = importlib.import_module("x-edr-trajectory-planning_amd.engine")
eng._SO = os.path.join(ROOT, "x-edr-trajectory-planning_amd", "csrc", os.environ.get("DIAG_SO", "libtpamd_diaglight.so"))
import runahead_cases as rc

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 3
E = eng.Engine(0)
NAMES = ("forward first", "backward first", "pair via run", "rare-branch waits", "mark waits", "ring full waits",
         "takes at depth 1", "depth 2", "depth 3", "depth 4", "poll expired")
total = np.zeros(len(NAMES))
print("%-28s" % "batch" + "".join("%16s" % n for n in NAMES))
batches = list(rc.all_batches()) + [("tight D=7 N=2000 (64)", 7, 2000, rc.tight_batch(7, 2000, B=64, first=500))]
for label, D, N, b in batches:
    B = b["control_points"].shape[0]
    inp = eng.upload_joint_batch(b, "cuda:0")
    out = eng.alloc_joint_outputs(B, N, D, "cuda:0")
    row = np.zeros(len(NAMES))
    for _ in range(repeats):
        E.time_joint_paths(inp, out, N)
        torch.cuda.synchronize()
        xx = E.debug_diag_ext(B).astype(np.float64)
        x, f = xx[:, :16], xx[:, 16:32]
        st = out["status"].cpu().numpy()
        row += np.array([x[:, 5].sum(), x[:, 6].sum(), f[:, 6].sum(), f[:, 9].sum(), f[:, 10].sum(), f[:, 11].sum(),
                         x[:, 1].sum(), x[:, 2].sum(), x[:, 3].sum(), x[:, 4].sum(), (st == 12).sum()])
    total += row
    print("%-28s" % label + "".join("%16d" % v for v in row), flush=True)
print("%-28s" % ("all, %d solves each" % repeats) + "".join("%16d" % v for v in total))

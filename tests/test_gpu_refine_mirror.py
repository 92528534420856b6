"""RefineSolutions on BatchPathTiming and BatchWaypointTiming (tests/cpp/test_batch_refine_gpu.cc): 16
paths of the shapes (7, 33, 4) and (16, 33, 4), two rounds. Off is bit-equal to never set; on, every
path is held against tpamd_time_joint_paths_refined_host on the same arrays (a cured path carries
2 n - 1 or 4 n - 3 samples, violations == 0 and the slot's arrays; a path refinement does not improve
keeps its coarse arrays), the offsets follow the sample counts, and the waypoint batch equals the path
batch."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_refine_solutions_option_of_the_batch_classes(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    importlib.import_module(PKG_NAME + ".engine").build_library()
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    host = os.path.join(ROOT, PKG_NAME, "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_batch_refine_gpu")
    subprocess.check_call(
        ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w",
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_batch_refine_gpu.cc"),
         "-L" + host, "-ltp_host", "-Wl,-rpath," + host,
         "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "FAIL" not in out.stdout
    for cls in ("BatchPathTiming", "BatchWaypointTiming"):
        for shape in ("(7, 33, 4)", "(16, 33, 4)"):
            assert "%s %s: " % (cls, shape) in out.stdout

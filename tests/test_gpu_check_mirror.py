"""CheckSolutions on BatchPathTiming, BatchWaypointTiming and BatchCartesianTiming
(tests/cpp/test_check_solutions_gpu.cc): 16 paths of the shapes (7, 65, 4) and (16, 33, 3); violations
== 0 exactly where the mirror's own TimeOptimalPathProfile::SolutionSatisfiesConstraints() is ok, and
timing results bit-equal with the option off and on."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_check_solutions_option_of_the_batch_classes(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    importlib.import_module(PKG_NAME + ".engine").build_library()
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    host = os.path.join(ROOT, PKG_NAME, "host")
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", host, "-s"])
    subprocess.check_call(["make", "-C", oracle, "-s", "libtp_oracle.so"])
    exe = str(tmp_path / "test_check_solutions_gpu")
    subprocess.check_call(
        ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w",
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_check_solutions_gpu.cc"),
         "-L" + host, "-ltp_host", "-Wl,-rpath," + host, "-L" + oracle, "-ltp_oracle", "-Wl,-rpath," + oracle,
         "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "FAIL" not in out.stdout
    for cls in ("BatchPathTiming", "BatchWaypointTiming", "BatchCartesianTiming"):
        for shape in ("(7, 65, 4)", "(16, 33, 3)"):
            assert "%s %s: " % (cls, shape) in out.stdout

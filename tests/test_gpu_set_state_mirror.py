"""Moving planners between sets through the C++ mirror (PathTimingTrajectorySet::ExportPlanners /
ImportPlanners / CopyPlanners): tests/cpp/test_set_state_gpu.cc holds every moved planner against a
host PathTimingTrajectory that was given the same waypoints and Plans and continues on the host --
getters at once after the move, then three more Plans, bit for bit -- for export + import into a set
of other capacities in reversed order, CopyPlanners into a third set and a rotation in place, at
D = 3 and 7 with both sampling methods; refused calls change nothing. The bridge from the
reference-named class: the bytes PlannerStateFromHost builds from a host planner equal the device
export of a set planner that was given the same calls, AdoptPlanner takes the host planner into a set
that continues bit-equal to a twin host planner, and ReleasePlanner hands it to a fresh host planner
that continues bit-equal as well."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_mirror_moves_planners_against_host_planners(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_state_gpu")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_state_gpu.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "FAIL" not in out.stdout
    assert out.stdout.count("set state vs host planners") == 4
    assert out.stdout.count("equal to the device export, 6 of 6 continued Plans bit-equal") == 4

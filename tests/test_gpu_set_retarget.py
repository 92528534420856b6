"""Retargeting moving planner-set planners on the GPU (tpamd_planner_set_retarget*,
PathTimingTrajectorySet::RetargetWaypointPaths): tests/cpp/test_set_retarget.cc holds 70-planner sets
at D = 3 and 7 with both sampling methods bit-equal to one mirror planner each, driven through
TrajectoryBuffer::GetPositionAtTime / GetVelocityAtTime, ComputeStoppingPoint, SetWaypoints and
SetPath (shuffled subsets, planners at rest, W = 0, refused planners against an untouched twin,
capacity growth, three Plans after the retarget), the _device entry on a non-blocking stream to
the host entry, and checks the call-level errors."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_retarget_against_mirrors(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_retarget")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_retarget.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[:4000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("retarget vs mirrors") == 4
    assert out.stdout.count("retarget C-ABI") == 4

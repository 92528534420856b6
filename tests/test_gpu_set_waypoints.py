"""New waypoint paths for planner-set planners, fitted on the GPU (tpamd_planner_set_set_waypoints*,
PathTimingTrajectorySet::SetWaypointPaths): tests/cpp/test_set_waypoints.cc holds 260-planner sets at
D = 3 and 7 with both sampling methods bit-equal to sets loaded with host-fitted paths and to one
mirror planner each (refits mid-motion with an initial velocity, capacity growth included), the
_device variant on a non-blocking stream to the host variant, and checks the call-level errors."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_waypoints_against_host_fit_and_mirrors(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_waypoints")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_waypoints.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(out.stdout[:4000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("device fit vs host fit and mirrors") == 4
    assert out.stdout.count("set_waypoints C-ABI") == 4

"""BatchWaypointTiming against BatchPathTiming (tests/cpp/test_batch_waypoint_timing.cc): 14 paths with
6 and 7 joints, 1 .. 9 waypoints and three sample counts; every packed result array bit-equal with the
options' delta_parameter and with CoverWholePath; AddPath's refusals; the path without waypoints."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_waypoint_mirror_equals_batch_path_timing(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    importlib.import_module(PKG_NAME + ".engine").build_library()
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    host = os.path.join(ROOT, PKG_NAME, "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_batch_waypoint_timing")
    subprocess.check_call(
        ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w",
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_batch_waypoint_timing.cc"),
         "-L" + host, "-ltp_host", "-Wl,-rpath," + host, "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64",
         "-lm", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "FAIL" not in out.stdout
    assert "delta_parameter: " in out.stdout and "whole path: " in out.stdout

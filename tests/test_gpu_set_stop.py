"""Stopping trajectories on the GPU (tpamd_planner_set_stop_trajectories*, tpamd_stop_trajectories_*;
PathTimingTrajectorySet::StopTrajectoriesBeforeTime): tests/cpp/test_set_stop.cc holds 260-planner
sets at D = 3 and 7 with both sampling methods byte-equal to the mirror's TrajectoryBuffer::StopBeforeTime
on each planner's GetTrajectory, checks that a stop leaves the next Plan unchanged, runs the _device
variant on a non-blocking stream with a Plan right after it, runs the batch form on solver and
resampler outputs (D = 3, 7, 14, ragged counts, by time and by index) against the mirror, and checks
the calls' errors."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_stop_against_mirror(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_stop")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_stop.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(out.stdout[:4000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("stop vs mirror (D") == 4
    assert out.stdout.count("stop C-ABI") == 4
    assert "batch stop vs mirror" in out.stdout

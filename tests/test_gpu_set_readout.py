"""Bulk readout of a planner set on the GPU (tpamd_planner_set_download_trajectories*,
tpamd_planner_set_sample_at_ticks*; PathTimingTrajectorySet::GetTrajectories / GetSetpoints):
tests/cpp/test_set_readout.cc holds 260-planner sets at D = 3 and 7 with both sampling methods
byte-equal to GetTrajectory of every planner and to one mirror planner's Get*AtTime each, follows a
few planners with the oracle's planner, checks that reading out does not change the next Plan, runs
the _device variants on a non-blocking stream with a Plan right after them, and checks the calls'
errors."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_readout_against_mirrors(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", host, "-s"])
    subprocess.check_call(["make", "-C", oracle, "-s", "libtp_oracle.so"])
    exe = str(tmp_path / "test_set_readout")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_readout.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L" + oracle, "-ltp_oracle",
           "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc, "-Wl,-rpath," + oracle]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=1200)
    print(out.stdout[:4000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("readout vs mirrors") == 4
    assert out.stdout.count("readout C-ABI") == 4

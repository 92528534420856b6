"""Planner-set checking over many windows on the GPU (tpamd_planner_set_set_checking / _check_results /
_check_results_device, PathTimingTrajectorySet::SetChecking / CheckResults / CheckResultsDevice):
tests/cpp/test_set_check_gpu.cc drives sets of 24 planners at D = 1, 7, 16, N = 64, 200 and both
sampling methods through Plan and through PlanDevice + CheckResultsDevice on one non-blocking stream,
over a first Plan and three replans, and holds every record bit-equal to one host
PathTimingTrajectory per planner with SetCheckSolutions(true); a twin set with checking off must plan
the same, bit for bit, and report "nothing checked"; call-level errors must write nothing. Cartesian
sets go through PlanStreaming, where planners wait for IK rows between two windows and are resumed."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_check_against_mirror_planners(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_check_gpu")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_check_gpu.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[:6000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("set check joint") == 12
    assert out.stdout.count("set check Cartesian streaming") == 2
    assert out.stdout.count("set check totals") == 1

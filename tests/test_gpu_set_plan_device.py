"""The enqueued-only Plan of planner sets on the GPU (tpamd_planner_set_plan_device / _reserve /
_capacity, PathTimingTrajectorySet::PlanDevice / FinishPlanDevice): tests/cpp/test_set_plan_device.cc
drives 70-planner sets (one of 130) at D = 3 and 7 with both sampling methods through plan_device on
a non-blocking stream with max_windows 1, 2 and 4 and holds every planner bit-equal to a twin set
driven through tpamd_planner_set_plan with max_planning_iterations = max_windows - 1 (mixed planner
kinds, three replans), does the same for Cartesian sets with resident tables, checks the
per-planner RESOURCE_EXHAUSTED outcomes and their recovery through reserve, the ordering against
other calls of the same engine without synchronisation by the caller, the four-call control cycle
on one stream, that the call does not wait for the stream, and the call-level errors."""
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_set_plan_device_against_twins(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    import importlib
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_set_plan_device")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_set_plan_device.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[:6000])
    print(out.stdout[-3000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("plan_device twins") == 13
    assert out.stdout.count("plan_device Cartesian") == 2
    assert out.stdout.count("plan_device capacity") == 2
    assert out.stdout.count("plan_device ordering") == 1
    assert out.stdout.count("plan_device cycle") == 1
    assert out.stdout.count("plan_device does not wait") == 1
    assert out.stdout.count("plan_device call-level errors") == 1
    assert out.stdout.count("plan_device mirror") == 1

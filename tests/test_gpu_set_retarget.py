"""Retargeting moving planner-set planners on the GPU (tpamd_planner_set_retarget*,
PathTimingTrajectorySet::RetargetWaypointPaths): tests/cpp/test_set_retarget.cc holds 70-planner sets
at D = 3 and 7 with both sampling methods bit-equal to one mirror planner each, driven through
TrajectoryBuffer::GetPositionAtTime / GetVelocityAtTime, ComputeStoppingPoint, SetWaypoints and
SetPath (shuffled subsets, planners at rest, W = 0, refused planners against an untouched twin,
capacity growth, three Plans after the retarget), the _device entry on a non-blocking stream to
the host entry, and checks the call-level errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_retarget_against_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_set_retarget.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=600, head=4000, tail=3000)
    assert out.count("retarget vs mirrors") == 4
    assert out.count("retarget C-ABI") == 4

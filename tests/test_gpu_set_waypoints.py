"""New waypoint paths for planner-set planners, fitted on the GPU (tpamd_planner_set_set_waypoints*,
PathTimingTrajectorySet::SetWaypointPaths): tests/cpp/test_set_waypoints.cc holds 260-planner sets at
D = 3 and 7 with both sampling methods bit-equal to sets loaded with host-fitted paths and to one
mirror planner each (refits mid-motion with an initial velocity, capacity growth included), the
_device variant on a non-blocking stream to the host variant, and checks the call-level errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_waypoints_against_host_fit_and_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_set_waypoints.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=1200, head=4000, tail=3000)
    assert out.count("device fit vs host fit and mirrors") == 4
    assert out.count("set_waypoints C-ABI") == 4

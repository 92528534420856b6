"""The online path switch of a planner set on the GPU (tpamd_planner_set_switch_paths,
PathTimingTrajectorySet::SwitchToWaypointPaths): tests/cpp/test_set_switch.cc holds 260-planner
sets at D = 3 and 7 with both sampling methods bit-equal to one mirror planner each running
GetPathStopParameter -> SwitchToWaypointPath -> SetInitialVelocity -> Plan, follows a few of them
with the oracle's planner, and checks the call's errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_switch_against_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_set_switch.cc", tmp_path, libs=("host", "engine", "oracle", "m"))
    out = run_driver(exe, timeout=1200, head=4000, tail=3000)
    assert out.count("switch vs mirrors") == 4

"""The enqueued-only Plan of planner sets on the GPU (tpamd_planner_set_plan_device / _reserve /
_capacity, PathTimingTrajectorySet::PlanDevice / FinishPlanDevice): tests/cpp/test_set_plan_device.cc
drives 70-planner sets (one of 130) at D = 3 and 7 with both sampling methods through plan_device on
a non-blocking stream with max_windows 1, 2 and 4 and holds every planner bit-equal to a twin set
driven through tpamd_planner_set_plan with max_planning_iterations = max_windows - 1 (mixed planner
kinds, three replans), does the same for Cartesian sets with resident tables, checks the
per-planner RESOURCE_EXHAUSTED outcomes and their recovery through reserve, the ordering against
other calls of the same engine without synchronisation by the caller, the four-call control cycle
on one stream, that the call does not wait for the stream, and the call-level errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_plan_device_against_twins(tmp_path):
    require_gpu()
    exe = build_driver("test_set_plan_device.cc", tmp_path, libs=("host", "engine", "hip", "m"), flags=("-pthread",))
    out = run_driver(exe, timeout=600, head=6000, tail=3000)
    assert out.count("plan_device twins") == 13
    assert out.count("plan_device Cartesian") == 2
    assert out.count("plan_device capacity") == 2
    assert out.count("plan_device ordering") == 1
    assert out.count("plan_device cycle") == 1
    assert out.count("plan_device does not wait") == 1
    assert out.count("plan_device call-level errors") == 1
    assert out.count("plan_device mirror") == 1

"""Planner-set checking over many windows on the GPU (tpamd_planner_set_set_checking / _check_results /
_check_results_device, PathTimingTrajectorySet::SetChecking / CheckResults / CheckResultsDevice):
tests/cpp/test_set_check_gpu.cc drives sets of 24 planners at D = 1, 7, 16, N = 64, 200 and both
sampling methods through Plan and through PlanDevice + CheckResultsDevice on one non-blocking stream,
over a first Plan and three replans, and holds every record bit-equal to one host
PathTimingTrajectory per planner with SetCheckSolutions(true); a twin set with checking off must plan
the same, bit for bit, and report "nothing checked"; call-level errors must write nothing. Cartesian
sets go through PlanStreaming, where planners wait for IK rows between two windows and are resumed."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_check_against_mirror_planners(tmp_path):
    require_gpu()
    exe = build_driver("test_set_check_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m"), flags=("-pthread",))
    out = run_driver(exe, timeout=600, head=6000, tail=3000)
    assert out.count("set check joint") == 12
    assert out.count("set check Cartesian streaming") == 2
    assert out.count("set check totals") == 1

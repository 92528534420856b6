"""Stopping trajectories on the GPU (tpamd_planner_set_stop_trajectories*, tpamd_stop_trajectories_*;
PathTimingTrajectorySet::StopTrajectoriesBeforeTime): tests/cpp/test_set_stop.cc holds 260-planner
sets at D = 3 and 7 with both sampling methods byte-equal to the mirror's TrajectoryBuffer::StopBeforeTime
on each planner's GetTrajectory, checks that a stop leaves the next Plan unchanged, runs the _device
variant on a non-blocking stream with a Plan right after it, runs the batch form on solver and
resampler outputs (D = 3, 7, 14, ragged counts, by time and by index) against the mirror, and checks
the calls' errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_stop_against_mirror(tmp_path):
    require_gpu()
    exe = build_driver("test_set_stop.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=1200, head=4000, tail=3000)
    assert out.count("stop vs mirror (D") == 4
    assert out.count("stop C-ABI") == 4
    assert "batch stop vs mirror" in out

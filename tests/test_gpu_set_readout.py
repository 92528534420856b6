"""Bulk readout of a planner set on the GPU (tpamd_planner_set_download_trajectories*,
tpamd_planner_set_sample_at_ticks*; PathTimingTrajectorySet::GetTrajectories / GetSetpoints):
tests/cpp/test_set_readout.cc holds 260-planner sets at D = 3 and 7 with both sampling methods
byte-equal to GetTrajectory of every planner and to one mirror planner's Get*AtTime each, follows a
few planners with the oracle's planner, checks that reading out does not change the next Plan, runs
the _device variants on a non-blocking stream with a Plan right after them, and checks the calls'
errors."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_set_readout_against_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_set_readout.cc", tmp_path, libs=("host", "engine", "oracle", "hip", "m"))
    out = run_driver(exe, timeout=1200, head=4000, tail=3000)
    assert out.count("readout vs mirrors") == 4
    assert out.count("readout C-ABI") == 4

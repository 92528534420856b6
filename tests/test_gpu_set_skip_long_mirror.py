"""The host mirror's PathTimingTrajectorySet with the skip method at a history capacity above 32768
samples (tests/cpp/test_set_skip_long.cc): every Plan equals one mirror PathTimingTrajectory per
planner, bit for bit."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_skip_method_set_above_32768_against_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_set_skip_long.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=300, tail=3000)
    assert "9 plans bit-equal to the mirrors" in out

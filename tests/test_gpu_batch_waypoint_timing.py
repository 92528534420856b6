"""BatchWaypointTiming against BatchPathTiming (tests/cpp/test_batch_waypoint_timing.cc): 14 paths with
6 and 7 joints, 1 .. 9 waypoints and three sample counts; every packed result array bit-equal with the
options' delta_parameter and with CoverWholePath; AddPath's refusals; the path without waypoints."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_waypoint_mirror_equals_batch_path_timing(tmp_path):
    require_gpu()
    exe = build_driver("test_batch_waypoint_timing.cc", tmp_path, libs=("host", "engine", "hip", "m"), flags=("-w",))
    out = run_driver(exe, timeout=300, forbid_fail=True)
    assert "delta_parameter: " in out and "whole path: " in out

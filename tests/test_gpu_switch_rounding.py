"""The rounding radius of the online path switch on the GPU (tpamd_planner_set_switch_paths_rounded,
PathTimingTrajectorySet::SwitchToWaypointPaths with `rounding`): tests/cpp/test_switch_rounding.cc
holds 70-planner sets at D = 3 and 7 with rounding 0, 0.05 and 1.0 bit-equal to mirror paths whose
PathOptions::rounding has that value, and the entry without the argument to rounding 0.2.
PlannerSet.switch_paths(rounding=...) is held to the same entry."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_switch_rounding_against_mirrors(tmp_path):
    require_gpu()
    exe = build_driver("test_switch_rounding.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=600)
    assert out.count("switch rounding") == 6
    assert out.count("switch without the argument") == 2


def test_python_switch_paths_takes_the_rounding():
    """PlannerSet.switch_paths: the default equals rounding=0.2 bit for bit, another radius gives
    another control polygon with the same knots."""
    require_gpu()
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    E = eng.Engine(0)
    B, D, N, MS = 5, 3, 100, 1_000_000
    rng = np.random.default_rng(5)
    wps = rng.uniform(-1.5, 1.5, size=(B * 3, D))
    off = np.arange(B + 1, dtype=np.int32) * 3
    new = rng.uniform(-1.5, 1.5, size=(B * 2, D))
    noff = np.arange(B + 1, dtype=np.int32) * 2
    splines = {}
    for name, kwargs in (("default", {}), ("0.2", dict(rounding=0.2)), ("0.05", dict(rounding=0.05))):
        with eng.PlannerSet(E, B, D, N, time_step_ns=MS) as ps:
            ps.set_waypoints(wps, off, np.full((B, D), 1.5), np.full((B, D), 3.0), 0.005)
            assert (ps.plan(1000 * MS, 400 * MS)["status"].numpy() == 0).all()
            got = ps.switch_paths(np.full(B, 1100 * MS, dtype=np.int64), new, noff, **kwargs)
            assert (got["status"].numpy() == 0).all(), got["status"]
            splines[name] = [ps.download_path(b) for b in range(B)]
    differ = 0
    for b in range(B):
        assert splines["default"][b][0].tobytes() == splines["0.2"][b][0].tobytes()
        assert splines["default"][b][1].tobytes() == splines["0.2"][b][1].tobytes()
        assert splines["default"][b][1].shape == splines["0.05"][b][1].shape
        differ += splines["default"][b][1].tobytes() != splines["0.05"][b][1].tobytes()
    assert differ >= 1      # (a switch position that projects onto the last waypoint has no corner to round)

"""The rounding radius of the online path switch on the GPU (tpamd_planner_set_switch_paths_rounded,
PathTimingTrajectorySet::SwitchToWaypointPaths with `rounding`): tests/cpp/test_switch_rounding.cc
holds 70-planner sets at D = 3 and 7 with rounding 0, 0.05 and 1.0 bit-equal to mirror paths whose
PathOptions::rounding has that value, and the entry without the argument to rounding 0.2.
PlannerSet.switch_paths(rounding=...) is held to the same entry."""
import importlib
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_switch_rounding_against_mirrors(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_switch_rounding")
    cmd = ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_switch_rounding.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm",
           "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    assert out.stdout.count("switch rounding") == 6
    assert out.stdout.count("switch without the argument") == 2


def test_python_switch_paths_takes_the_rounding():
    """PlannerSet.switch_paths: the default equals rounding=0.2 bit for bit, another radius gives
    another control polygon with the same knots."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
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

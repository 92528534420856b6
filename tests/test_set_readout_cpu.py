"""The planner-set readout's bracket and interpolation on the CPU: csrc/tpamd_readout.h (host/device
functions) compiled for the host and compared bit for bit with the mirror's
TrajectoryPlanner::Get{Position,Velocity,Acceleration}AtTime, and the switch's sw_velocity_at_time,
which takes the same bracket, with GetVelocityAtTime (tests/cpp/test_readout_interp.cc). No GPU
needed."""
import os

from conftest import ROOT, PKG_NAME
from native_driver import build_driver, run_driver


def test_readout_interpolation_matches_mirror_bit_for_bit(tmp_path):
    exe = build_driver("test_readout_interp.cc", tmp_path, opt="-O2")
    out = run_driver(exe, timeout=600, tail=3000)
    counts = {}
    for line in out.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
        if line.startswith("interpolation cases:"):
            assert int(line.split(":")[1]) >= 20000
    # every edge of the bracket is reached
    for cat in ("on a sample/ok", "between samples/ok", "first sample/ok", "last sample/ok", "inside/ok",
                "1 ns before the first/status 2", "1 ns after the last/status 2", "on a repeated stamp/ok",
                "one sample/ok", "one sample/status 2", "empty/status 1"):
        assert counts.get(cat, 0) > 0, (cat, counts)
    assert "tick times: ok" in out


def test_readout_exports_are_declared():
    """The four readout entry points are in the header and registered with the binding."""
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    for name in ("tpamd_planner_set_sample_at_ticks", "tpamd_planner_set_sample_at_ticks_device",
                 "tpamd_planner_set_download_trajectories", "tpamd_planner_set_download_trajectories_device"):
        assert "int %s(" % name in hdr, name
        assert name in eng.ABI_SYMBOLS and len(getattr(lib, name).argtypes) >= 10, name
    assert os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_readout.h") in eng._abi.library_sources()

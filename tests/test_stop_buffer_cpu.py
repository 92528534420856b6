"""Stopping trajectories on the CPU: the mirror's TrajectoryBuffer::StopAtIndex / StopBeforeTime
and RescaleTrajectoryBackwardToStop (host/trajectory_buffer.cc, host/rescale_to_stop.cc) on the
reference's test cases, and the host/device core of csrc/tpamd_rescale.h, compiled for the host,
bit-equal to the mirror on seeded trajectories (tests/cpp/test_stop_buffer.cc). No GPU needed."""
import os

from conftest import ROOT, PKG_NAME
from native_driver import build_driver, run_driver


def test_stop_core_matches_mirror_bit_for_bit(tmp_path):
    exe = build_driver("test_stop_buffer.cc", tmp_path, opt="-O2",
                       extra_sources=("host/rescale_to_stop.cc", "host/trajectory_buffer.cc"))
    out = run_driver(exe, timeout=600, tail=3000)
    assert "reference cases: done" in out
    counts = {}
    for line in out.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
        if line.startswith("stop cases:"):
            assert int(line.split(":")[1]) >= 20000
    for cat in ("broke at rate >= 1", "used all samples and matched", "NotFound", "last-sample early return",
                "at-rest mid (Internal)", "before the front", "clamped beyond the end",
                "kept count decremented", "kept count not decremented", "empty", "one sample",
                "bad max_acceleration", "bad time_step", "non-increasing times"):
        assert counts.get(cat, 0) > 0, (cat, counts)


def test_stop_exports_are_declared():
    """The stop entry points are in the header and registered with the binding."""
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    for name in ("tpamd_stop_trajectories_device", "tpamd_stop_trajectories_host",
                 "tpamd_planner_set_stop_trajectories", "tpamd_planner_set_stop_trajectories_device"):
        assert "int %s(" % name in hdr, name
        assert name in eng.ABI_SYMBOLS and len(getattr(lib, name).argtypes) >= 2, name
    assert "#define TPAMD_PLAN_NOT_FOUND 6" in hdr
    assert os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_rescale.h") in eng._abi.library_sources()
    mk = open(os.path.join(ROOT, PKG_NAME, "host", "Makefile")).read()
    assert "rescale_to_stop.cc" in mk and "trajectory_buffer.cc" in mk

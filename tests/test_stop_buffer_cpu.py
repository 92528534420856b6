"""Stopping trajectories on the CPU: the mirror's TrajectoryBuffer::StopAtIndex / StopBeforeTime
and RescaleTrajectoryBackwardToStop (host/trajectory_buffer.cc, host/rescale_to_stop.cc) on the
reference's test cases, and the host/device core of csrc/tpamd_rescale.h, compiled for the host,
bit-equal to the mirror on seeded trajectories (tests/cpp/test_stop_buffer.cc). No GPU needed."""
import os
import subprocess

from conftest import ROOT, PKG_NAME


def _build_driver(tmp_path):
    exe = str(tmp_path / "test_stop_buffer")
    host = os.path.join(ROOT, PKG_NAME, "host")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_stop_buffer.cc"),
           os.path.join(host, "rescale_to_stop.cc"), os.path.join(host, "trajectory_buffer.cc")]
    subprocess.check_call(cmd)
    return exe


def test_stop_core_matches_mirror_bit_for_bit(tmp_path):
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "reference cases: done" in out.stdout
    counts = {}
    for line in out.stdout.splitlines():
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
    src = open(os.path.join(ROOT, PKG_NAME, "engine.py")).read()
    for name in ("tpamd_stop_trajectories_device", "tpamd_stop_trajectories_host",
                 "tpamd_planner_set_stop_trajectories", "tpamd_planner_set_stop_trajectories_device"):
        assert "int %s(" % name in hdr, name
        assert '"%s"' % name in src, name
    assert "#define TPAMD_PLAN_NOT_FOUND 6" in hdr
    assert '"tpamd_rescale.h"' in src
    mk = open(os.path.join(ROOT, PKG_NAME, "host", "Makefile")).read()
    assert "rescale_to_stop.cc" in mk and "trajectory_buffer.cc" in mk

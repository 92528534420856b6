"""The planner-set path switch's edit routines on the CPU: csrc/tpamd_switch.h (host/device
functions) compiled for the host and compared bit for bit with the mirror's
TimeableJointSplinePath::SwitchToWaypointPath and TrajectoryPlanner::GetVelocityAtTime
(tests/cpp/test_switch_edit.cc). No GPU needed."""
import importlib
import os
import subprocess

from conftest import ROOT, PKG_NAME


def _build_driver(tmp_path):
    importlib.import_module(PKG_NAME + ".engine").build_library()
    host = os.path.join(ROOT, PKG_NAME, "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    exe = str(tmp_path / "test_switch_edit")
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    cmd = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "test_switch_edit.cc"),
           "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc]
    subprocess.check_call(cmd)
    return exe


def test_switch_edit_matches_mirror_bit_for_bit(tmp_path):
    exe = _build_driver(tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    counts = {}
    for line in out.stdout.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
        if line.startswith("edit cases:"):
            assert int(line.split(":")[1]) >= 4000
    # every edge the switch has is reached, and each of them succeeds somewhere
    for cat in ("inside a span/ok", "keep >= umax/ok", "keep >= umax/status 2", "keep <= umin/status 2",
                "projection within 1e-3/ok", "line parameter < 0/ok", "repeated waypoints/ok",
                "three in a row (3)/ok"):
        assert counts.get(cat, 0) > 0, (cat, counts)
    assert any(k.startswith("on a knot/") for k in counts), counts
    assert "velocity bracket:" in out.stdout

"""The planner-set path switch's edit routines on the CPU: csrc/tpamd_switch.h (host/device
functions) compiled for the host and compared bit for bit with the mirror's
TimeableJointSplinePath::SwitchToWaypointPath and TrajectoryPlanner::GetVelocityAtTime
(tests/cpp/test_switch_edit.cc). No GPU needed."""
from native_driver import build_driver, run_driver


def test_switch_edit_matches_mirror_bit_for_bit(tmp_path):
    exe = build_driver("test_switch_edit.cc", tmp_path, libs=("host", "engine"), opt="-O2")
    out = run_driver(exe, timeout=600, tail=3000)
    counts = {}
    for line in out.splitlines():
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
    assert "velocity bracket:" in out

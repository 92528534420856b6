"""path_tools on the CPU: csrc/tpamd_retarget.h (host/device functions) compiled for the host and
compared bit for bit with the mirror's ComputeStoppingPoint and ProjectPointOnPath for every
D = 1..16 (tests/cpp/test_path_tools.cc), both held against the long-double restatement of
tests/path_tools_reference.py, and the literal cases of the reference's path_tools_test.cc
(tests/golden/path_tools_golden.json). No GPU needed."""
import json
import os
import subprocess

import numpy as np
import pytest

import native_driver
import path_tools_reference as ref

# The mirror's largest relative error against the long-double restatement over the 768 moving rows
# of the dump (3.2 epsilon, at D = 2), measured on the build this was written on, and the bound held
# here: 8 x that, for a different libm or compiler (DESIGN.md "What holds path_tools").
MEASURED_STOP_ERROR = 7.1e-16
STOP_ERROR_BOUND = 8 * MEASURED_STOP_ERROR


def build_driver(dirname):
    return native_driver.build_driver("test_path_tools.cc", dirname, libs=("m",), opt="-O2",
                                      extra_sources=("host/path_tools.cc", "host/spline_edit.cc"))


def read_dump(path):
    """The cases of a test_path_tools dump: (stops, projs), each a list of dicts."""
    stops, projs = [], []
    for line in open(path):
        f = line.split()
        val = lambda a: np.array([float.fromhex(x) for x in a])
        if f[0] == "stop":
            D = int(f[1])
            v = val(f[4:])
            assert len(v) == 1 + 4 * D
            stops.append(dict(D=D, category=int(f[2]), status=int(f[3]), rounding=v[0], pos=v[1:1 + D],
                              vel=v[1 + D:1 + 2 * D], acc=v[1 + 2 * D:1 + 3 * D], out=v[1 + 3 * D:]))
        else:
            D, W = int(f[1]), int(f[2])
            v = val(f[5:])
            assert len(v) == D + W * D + 2 + D
            projs.append(dict(D=D, W=W, status=int(f[3]), index=int(f[4]), point=v[:D],
                              wps=v[D:D + W * D].reshape(W, D), distance=v[D + W * D], parameter=v[D + W * D + 1],
                              proj=v[D + W * D + 2:]))
    return stops, projs


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("path_tools")
    exe = build_driver(d)
    dump = os.path.join(str(d), "cases.txt")
    out = subprocess.run([exe, dump], capture_output=True, text=True, timeout=600)
    return exe, dump, out


def test_routines_match_the_mirror_bit_for_bit(driver):
    _, dump, out = driver
    print(out.stdout[-4000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    counts = {}
    for line in out.stdout.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
    for kind in ("random", "rest", "below 100 eps", "one moving joint",
                 "velocity along the axis of the smallest limit", "equal limits"):
        for r in ("rounding 0", "rounding 0.2", "large rounding"):
            assert counts.get("stop: %s, %s" % (kind, r), 0) >= 48, (kind, r, counts)
    assert sum(n for k, n in counts.items() if k.startswith("stop: non-positive limit")) == 64, counts
    for kind in ("no waypoints", "one waypoint", "random point", "point on a waypoint", "point on a segment",
                 "point beyond the end", "point before the start", "repeated waypoints"):
        assert counts.get("proj: " + kind, 0) >= 32, (kind, counts)
    stops, projs = read_dump(dump)
    for D in range(1, 17):
        assert sum(c["D"] == D for c in stops) == 70 and sum(c["D"] == D for c in projs) == 70


def test_stopping_points_against_the_long_double_reference(driver):
    _, dump, out = driver
    assert out.returncode == 0
    stops, _ = read_dump(dump)
    worst, large = 0.0, 0
    for c in stops:
        status, point, parts = ref.compute_stopping_point(c["pos"], c["vel"], c["acc"], c["rounding"])
        assert status == c["status"], c
        if status != ref.OK:
            continue
        if parts is None:                        # at rest: the position itself
            assert c["out"].tobytes() == c["pos"].tobytes()
            continue
        ref.check_stopping_parts(parts, c["vel"], c["acc"], c["rounding"])
        worst = max(worst, ref.stopping_point_error(c["out"], c["pos"], c["vel"], c["acc"], c["rounding"]))
        ref.check_stopping_point(c["out"], c["pos"], c["vel"], c["acc"], c["rounding"], rel=STOP_ERROR_BOUND)
        delta = float(np.sqrt(np.sum(parts["delta"] ** 2)))
        large += c["rounding"] > delta / 4
    print("largest relative error of the mirror against the long-double reference: %.3e (bound %.3e)"
          % (worst, STOP_ERROR_BOUND))
    assert large >= 16 * 10                      # the large roundings do exceed |delta| / 4
    assert worst <= STOP_ERROR_BOUND


def test_projections_against_the_long_double_reference(driver):
    _, dump, out = driver
    assert out.returncode == 0
    _, projs = read_dump(dump)
    eps = float(np.finfo(np.float64).eps)
    for c in projs:
        status, index, dist, t, proj = ref.project_point_on_path(c["wps"], c["point"])
        assert status == c["status"], c
        if status != ref.OK:
            continue
        # the least distance is what a projection means; index and parameter may differ between
        # two segments that are equally close (a point on a shared waypoint)
        rel = 64 * eps
        scale = max(np.abs(c["wps"]).max(), np.abs(c["point"]).max(), 1.0)
        assert abs(c["distance"] - float(dist)) <= rel * scale, c
        ref.check_projection(c["wps"], c["point"], c["distance"], rel)
        if index == c["index"] and c["W"] > 1:
            a, b = c["wps"][c["index"]], c["wps"][c["index"] + 1]
            length = float(np.sqrt(np.sum((b - a) ** 2)))
            if length > 1e-3:
                assert abs(c["parameter"] - float(t)) * length <= rel * scale * 4, c
                assert np.abs(c["proj"] - np.asarray(proj, dtype=np.float64)).max() <= rel * scale * 4, c
        # the projected point lies where the parameter says
        if c["W"] > 1:
            a, b = c["wps"][c["index"]], c["wps"][c["index"] + 1]
            assert np.abs(c["proj"] - (a + c["parameter"] * (b - a))).max() <= rel * scale
            assert c["parameter"] <= 1.0


def _evaluate(exe, tmp_path, lines):
    src = tmp_path / "eval.txt"
    src.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, "--eval", str(src)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
    rows = []
    for line in out.stdout.splitlines():
        f = line.split()
        if f and f[0] == "stop":
            rows.append((int(f[1]), np.array([float.fromhex(x) for x in f[2:]])))
        elif f and f[0] == "proj":
            v = [float.fromhex(x) for x in f[3:]]
            rows.append((int(f[1]), int(f[2]), v[0], v[1], np.array(v[2:])))
    return rows


def test_golden_cases_of_the_reference(driver, tmp_path, golden_dir):
    exe = driver[0]
    g = json.load(open(os.path.join(golden_dir, "path_tools_golden.json")))
    fmt = lambda v: " ".join(float(x).hex() for x in np.ravel(v))
    lines, expect = [], []
    for c in g["project"]:
        wps = np.array(c["waypoints"])
        if "point" in c:
            point, proj = np.array(c["point"]), np.array(c["projected_point"])
            want = (c["waypoint_index"], c["distance_to_path"], c["line_parameter"], proj)
        else:                                    # built as the test builds it
            t = c["line_parameter_of_projected_point"]
            proj = wps[1] + t * (wps[2] - wps[1])
            point = proj + np.array(c["point_offset"])
            want = (c["waypoint_index"], float(np.linalg.norm(proj - point)), t, proj)
        lines.append("proj %d %d %s %s" % (wps.shape[1], wps.shape[0], fmt(point), fmt(wps)))
        expect.append(want)
    lines.append("proj 2 0 0x0p+0 0x0p+0")
    for c in g["stopping_point"]:
        D = len(c["position"])
        lines.append("stop %d %s %s %s %s" % (D, float(c["corner_rounding"]).hex(), fmt(c["position"]),
                                              fmt(c["velocity"]), fmt(c["acceleration_limit"])))
    rows = _evaluate(exe, tmp_path, lines)
    assert len(rows) == len(lines)
    ulp4 = lambda a, b: abs(a - b) <= 4 * np.finfo(np.float64).eps * max(abs(a), abs(b))     # EXPECT_DOUBLE_EQ
    for (status, index, dist, t, proj), (w_index, w_dist, w_t, w_proj) in zip(rows, expect):
        assert status == ref.OK and index == w_index
        assert ulp4(dist, w_dist) and ulp4(t, w_t)
        assert np.abs(proj - w_proj).max() <= g["epsilon"]
    assert rows[len(expect)][0] == ref.INVALID_ARGUMENT                   # "No waypoints."
    for c, (status, out) in zip(g["stopping_point"], rows[len(expect) + 1:]):
        pos, vel = np.array(c["position"]), np.array(c["velocity"])
        if "status" in c:
            assert status == ref.INVALID_ARGUMENT
        elif c["expect"] == "equals_position":
            assert status == ref.OK and np.array_equal(out, pos)
        else:
            assert status == ref.OK and not np.array_equal(out, pos)
            directions = np.stack([vel, out - pos], axis=1)
            assert np.linalg.matrix_rank(directions) == 1
            assert np.dot(out - pos, vel) > 0

"""The planner-set waypoint fit on the CPU: csrc/tpamd_fit.h (host/device functions) compiled for the
host and compared bit for bit with the mirror's TimeableJointSplinePath::SetWaypoints and the oracle's
joint fit (tests/cpp/test_fit_waypoints.cc), and a sample of its cases with tpo.joint_fit_spline.
No GPU needed."""
import subprocess

import numpy as np

from native_driver import build_driver


def _build_driver(tmp_path):
    return build_driver("test_fit_waypoints.cc", tmp_path, libs=("host", "engine", "oracle", "m"), opt="-O2")


def _read_cases(path):
    raw = open(path, "rb").read()
    pos, cases = 0, []
    while pos < len(raw):
        W, D = np.frombuffer(raw, dtype=np.int32, count=2, offset=pos)
        pos += 8
        rounding = float(np.frombuffer(raw, dtype=np.float64, count=1, offset=pos)[0])
        pos += 8
        P = 4 if W == 1 else 3 * W - 2
        take = lambda n: np.frombuffer(raw, dtype=np.float64, count=n, offset=pos)
        wps = take(W * D).reshape(W, D)
        pos += 8 * W * D
        knots = take(P + 3)
        pos += 8 * (P + 3)
        cps = take(P * D).reshape(P, D)
        pos += 8 * P * D
        cases.append((int(W), int(D), rounding, wps, knots, cps))
    return cases


def test_fit_matches_mirror_and_oracle_bit_for_bit(tmp_path):
    exe = _build_driver(tmp_path)
    dump = str(tmp_path / "fit_cases.bin")
    out = subprocess.run([exe, dump], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    counts = {}
    for line in out.stdout.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
        if line.startswith("fit cases:"):
            assert int(line.split(":")[1]) >= 5000
    for kind in ("random", "repeated waypoints", "collinear runs", "polygon shorter than 0.1"):
        for r in ("rounding 0", "rounding 0.2", "large rounding"):
            assert counts.get(kind + ", " + r, 0) >= 200, (kind, r, counts)
    assert counts.get("final knot 0.1 (polygon shorter than 0.1)", 0) > 0, counts
    assert counts.get("no waypoints / wrong dimension", 0) == 5, counts

    # the same fits through the oracle's Python entry
    from oracle import tpo
    tpo.build()
    cases = _read_cases(dump)
    assert len(cases) >= 200
    for W, D, rounding, wps, knots, cps in cases:
        ocps, oknots = tpo.joint_fit_spline(wps, rounding)
        assert ocps.shape == cps.shape and oknots.shape == knots.shape, (W, D)
        assert ocps.tobytes() == cps.tobytes() and oknots.tobytes() == knots.tobytes(), (W, D, rounding)

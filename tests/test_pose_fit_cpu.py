"""The Cartesian waypoint fit on the CPU: csrc/tpamd_pose_fit.h (host/device functions) compiled for the
host. tests/cpp/test_pose_fit.cc holds fit_pose_waypoints bit-equal to the mirror's
TimeableCartesianSplinePath::SetWaypoints on the seeded case list of tests/pose_fit_reference.py; the
same fits are compared with that module's long-double restatement and with the reference's literal
corner-rounding poses; the driver runs once more as a stand-alone program under
-fsanitize=address,undefined; tpamd_ik_table_rows is checked against the mirror's formula. No GPU
needed."""
import importlib
import json
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, PKG_NAME
from native_driver import build_driver
import pose_fit_reference as pfr

DRIVER = "test_pose_fit.cc"


def _golden_cases():
    """The reference's corner-rounding tests (splines/spline_utils_test.cc:31-146, as data in
    tests/golden/spline_utils_golden.json) as fit cases: rotations about (1, 2, 3) / |(1, 2, 3)|."""
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "spline_utils_golden.json")))
    axis = np.array(fx["rotation_axis"]) / np.linalg.norm(fx["rotation_axis"])
    quat = lambda angle: np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])
    cases = []
    for c in fx["cases"]:
        pose = np.array([np.concatenate([p["translation"], quat(p["angle"])]) for p in c["corners"]])
        cases.append(dict(family="golden", W=len(pose), D=1, tr=c["translation_radius"], rr=c["rotation_radius"],
                          pose=pose, joints=np.zeros((len(pose), 1)), golden=c, quat=quat))
    return cases


@pytest.fixture(scope="module")
def fits(tmp_path_factory):
    """The case list, and fit_pose_waypoints' result on every case as the mirror-linked driver dumps
    it (the driver's bit-for-bit comparison with the mirror runs in the same pass)."""
    tmp = tmp_path_factory.mktemp("pose_fit")
    exe = build_driver(DRIVER, tmp, libs=("host", "engine", "m"), opt="-O2")
    cases = pfr.all_cases() + _golden_cases()
    case_file, dump = str(tmp / "cases.bin"), str(tmp / "fits.bin")
    pfr.write_cases(case_file, cases)
    out = subprocess.run([exe, case_file, dump], capture_output=True, text=True, timeout=600)
    return dict(cases=cases, case_file=case_file, out=out, fits=pfr.read_fits(dump, cases) if out.returncode == 0 else None)


def test_fit_matches_mirror_bit_for_bit(fits):
    out = fits["out"]
    print(out.stdout[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-2000:]
    assert "standalone" not in out.stdout
    counts = {}
    for line in out.stdout.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
    assert sum(counts[f] for f in pfr.FAMILIES) >= 3000, counts
    for fam in pfr.FAMILIES:
        assert counts.get(fam, 0) >= 200, (fam, counts)
    assert counts.get("empty", 0) == 4, counts
    floor = [int(l.split(":")[1]) for l in out.stdout.splitlines() if l.startswith("final knot at the floor")]
    assert floor and floor[0] >= 200, floor                 # the "short" family ends on 0.1 * 10
    cases = fits["cases"]
    assert {c["W"] for c in cases} >= set(range(0, 7)) and {c["D"] for c in cases} >= set(pfr.DOFS)
    assert {(c["tr"], c["rr"]) for c in cases} >= set(pfr.ROUNDINGS)
    for c, f in zip(cases, fits["fits"]):
        assert f["P"] == (0 if c["W"] < 1 else max(3 * c["W"] - 2, 4))
        if c["family"] == "short":
            assert f["knots"][-1] == 0.1 * 10.0


def test_fit_against_long_double_reference(fits):
    """Every control-point component and the last knot within 4e-15 max(1, |x|) of the long-double
    restatement (pose_fit_reference.fit). Prints the worst values."""
    assert fits["fits"] is not None, fits["out"].stdout[-2000:]
    worst = dict(translation=0.0, rotation=0.0, joints=0.0, last_knot=0.0)
    n = 0
    for c, f in zip(fits["cases"], fits["fits"]):
        if c["W"] < 1 or c["family"] == "golden":
            continue
        ref = pfr.fit(c["pose"], c["joints"], c["tr"], c["rr"])
        for key in ("translation", "rotation", "joints"):
            worst[key] = max(worst[key], pfr.deviation(f[key], ref[key]))
        worst["last_knot"] = max(worst["last_knot"], pfr.deviation(f["knots"][-1:], ref["knots"][-1:]))
        # the whole knot vector is the last knot times exact fractions: a looser sanity check of the shape
        assert pfr.deviation(f["knots"], ref["knots"]) < 1e-13
        n += 1
    print("pose fit against long double over %d cases: worst deviation / max(1, |x|): %r" % (n, worst))
    assert n >= 3000
    for key, value in worst.items():
        assert value <= pfr.BOUND, (key, value)


def test_reference_corner_rounding_fixtures(fits):
    """The literal control poses of the reference's own corner-rounding tests, through
    fit_pose_waypoints (1e-9 on translations, rotations equal up to sign: eigenmath IsApprox)."""
    assert fits["fits"] is not None
    checked = used = 0
    for c, f in zip(fits["cases"], fits["fits"]):
        if c["family"] != "golden":
            continue
        g = c["golden"]
        assert f["P"] == g["num_control_points"], g["name"]
        if c["W"] == 1:
            assert (f["translation"] == c["pose"][0, :3]).all() and (f["rotation"] == c["pose"][0, 3:]).all()
        else:
            assert (f["translation"][0::3] == c["pose"][:, :3]).all() and (f["rotation"][0::3] == c["pose"][:, 3:]).all()
        for idx, pose in g["expected"].items():
            np.testing.assert_allclose(f["translation"][int(idx)], pose["translation"], atol=1e-9, err_msg=g["name"])
            dot = abs(float(np.dot(f["rotation"][int(idx)], c["quat"](pose["angle"]))))
            assert abs(dot - 1.0) < 1e-12, (g["name"], idx, dot)
            checked += 1
        if g["name"] == "ZeroRadius":
            assert (f["translation"][1] == c["pose"][0, :3]).all() and (f["translation"][2] == c["pose"][1, :3]).all()
        used += 1
    assert used == 5 and checked == 10


def test_sanitized_standalone_driver(fits, tmp_path):
    """The same driver as a stand-alone program (own main, header only, no mirror) built with
    -fsanitize=address,undefined, on the same case list. No Python process loads sanitized code."""
    exe = build_driver(DRIVER, tmp_path, libs=("m",), name="test_pose_fit_san",
                       flags=("-g", "-DPOSE_FIT_STANDALONE", "-fsanitize=address,undefined",
                              "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"))
    out = subprocess.run([exe, fits["case_file"]], capture_output=True, text=True, timeout=600)
    print(out.stdout[-1500:], out.stderr[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "standalone: mirror not linked" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr


def test_ik_table_rows_against_the_mirror_formula():
    """tpamd_ik_table_rows = PathIkIndex(knots.back()) + N + 1 with PathIkIndex = std::round(x / delta)
    (half away from zero), on values that include exact halves; -1 for a bad delta or sample count."""
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    table = [  # path_end, delta, N, rows
        (1.0, 0.25, 3, 4 + 3 + 1), (1.0, 0.4, 3, 3 + 3 + 1),      # 2.5 rounds away from zero
        (0.5, 1.0, 64, 1 + 64 + 1), (1.5, 1.0, 64, 2 + 64 + 1), (2.5, 1.0, 64, 3 + 64 + 1),
        (0.125, 0.25, 10, 1 + 10 + 1), (0.375, 0.25, 10, 2 + 10 + 1), (0.49, 1.0, 5, 0 + 5 + 1),
        (0.0, 0.1, 3, 0 + 3 + 1), (17.3, 0.004, 1000, 4325 + 1000 + 1), (1.0, 0.1, 1, 10 + 1 + 1),
        (3.0, 2.0, 7, 2 + 7 + 1), (5.0, 2.0, 7, 3 + 7 + 1), (7.0, 2.0, 7, 4 + 7 + 1),
    ]
    for path_end, delta, N, rows in table:
        x = path_end / delta
        mirror = int(np.floor(abs(x) + 0.5) * np.sign(x)) + N + 1          # std::round
        assert rows == mirror, (path_end, delta, N)
        assert lib.tpamd_ik_table_rows(path_end, delta, N) == rows, (path_end, delta, N)
    rng = np.random.default_rng(5)
    for _ in range(300):
        path_end, delta, N = rng.uniform(0.0, 40.0), rng.uniform(1e-3, 0.5), int(rng.integers(1, 2000))
        x = path_end / delta
        assert lib.tpamd_ik_table_rows(path_end, delta, N) == int(np.floor(x + 0.5)) + N + 1
    for path_end, delta, N in ((1.0, 0.0, 3), (1.0, -0.1, 3), (1.0, float("nan"), 3), (1.0, 0.1, 0), (1.0, 0.1, -2)):
        assert lib.tpamd_ik_table_rows(path_end, delta, N) == -1

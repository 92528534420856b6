"""CPU-only part of the C++ host mirror: online path edits (knot insertion, truncation,
extension, SwitchToWaypointPath, ProjectPointOnPath) against the reference's own tests restated
as data, and the mirror's brute-force LP against the oracle's (tests/cpp/test_host_cpu.cc)."""
import os

from conftest import ROOT
from native_driver import CPP, build_driver, run_driver


def test_host_path_edits_and_brute_force_lp():
    exe = build_driver("test_host_cpu.cc", CPP, libs=("host", "engine", "oracle", "m"))
    # the reference's corner-rounding fixtures (data) as a flat list of numbers for the C++ reader
    import json
    fx = json.load(open(os.path.join(ROOT, "tests", "golden", "spline_utils_golden.json")))
    flat = os.path.join(ROOT, "tests", "cpp", "spline_utils_cases.txt")
    with open(flat, "w") as f:
        f.write("%d\n" % len(fx["cases"]))
        for c in fx["cases"]:
            f.write("%d %r %r %d\n" % (len(c["corners"]), c["translation_radius"], c["rotation_radius"],
                                      c["num_control_points"]))
            for p in c["corners"]:
                f.write("%r %r %r %r\n" % (*p["translation"], p["angle"]))
            f.write("%d\n" % len(c["expected"]))
            for idx, p in sorted(c["expected"].items()):
                f.write("%s %r %r %r %r\n" % (idx, *p["translation"], p["angle"]))
    run_driver(exe, flat, timeout=300, tail=3000, err_tail=1000)

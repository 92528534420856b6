"""Cartesian planner sets on the CPU: the window rule of csrc/tpamd_cartesian_window.h (which table
rows a window reads, whether the table holds them, and the per-sample arithmetic that follows)
compiled for the host and held against the oracle bit for bit (tests/cpp/test_cartesian_window.cc);
the new entry points are declared, defined, bound and reachable from the mirror; the library
cross-compiles for gfx950 and the resource-usage record of the touched kernels is present. No GPU
needed."""
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME
from native_driver import build_driver, run_driver

ENTRIES = ("tpamd_planner_set_create_cartesian", "tpamd_planner_set_upload_ik_tables",
           "tpamd_planner_set_upload_ik_tables_device", "tpamd_planner_set_download_ik_table")


def test_window_rule_matches_the_oracle_bit_for_bit(tmp_path):
    exe = build_driver("test_cartesian_window.cc", tmp_path, libs=("oracle", "m"), opt="-O2")
    out = run_driver(exe, timeout=600, tail=3000)
    counts = {}
    for line in out.splitlines():
        if ":" in line and line.rsplit(":", 1)[1].strip().isdigit():
            counts[line.rsplit(":", 1)[0]] = int(line.rsplit(":", 1)[1])
    assert counts["in range"] > 1000 and counts["out of range"] > 100 and counts["samples"] > 50000
    for name in ("window ends on the last row", "one row before", "one row past"):
        assert counts[name] > 0, counts


def test_synthetic_family_keeps_every_oracle_planner_ok(tmp_path):
    """The condition the GPU parity test rests on, checked without a GPU: over the synthetic families
    of tests/cpp/test_cartesian_set_gpu.cc (its --cpu-check mode: the oracle planners alone, no GPU
    call) every oracle planner returns OK at every Plan and ends with target_reached, the
    modified-state re-upload included."""
    exe = build_driver("test_cartesian_set_gpu.cc", tmp_path, libs=("engine", "oracle", "hip", "m"), flags=("-pthread",))
    out = run_driver(exe, "--cpu-check", timeout=900, tail=3000)
    assert out.count("family: D") == 6 and out.count("256 at the end") == 6
    assert out.count("modified") == 3 and "FAILURES" not in out


def test_cartesian_set_exports_are_declared():
    """The Cartesian-set entry points are in the header, defined in the C-ABI, registered with the
    binding and reachable from the mirror."""
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    src = open(os.path.join(ROOT, PKG_NAME, "engine.py")).read()
    capi = open(os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_capi.hip")).read()
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    for name in ENTRIES:
        assert "int %s(" % name in hdr, name
        assert re.search(r"^int %s\(" % name, capi, re.M), name
        assert name in eng.ABI_SYMBOLS, name                  # the export list, read from the header
        assert len(getattr(lib, name).argtypes) >= 4, name    # and the prototype, set from its declaration
    assert os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_cartesian_window.h") in eng._abi.library_sources()
    for method in ("def set_ik_tables(", "def download_ik_table(", "cartesian=False", "table_capacity="):
        assert method in src, method
    cls = open(os.path.join(ROOT, PKG_NAME, "host", "path_timing_trajectory_set.h")).read()
    for method in ("SetCartesianPath(", "SetCartesianPaths(", "SetIkTables(", "GetIkTable(", "CartesianTableCapacity"):
        assert method in cls, method
    impl = open(os.path.join(ROOT, PKG_NAME, "host", "path_timing_trajectory_set.cc")).read()
    for name in ("tpamd_planner_set_create_cartesian", "tpamd_planner_set_upload_ik_tables",
                 "tpamd_planner_set_download_ik_table"):
        assert name + "(" in impl, name
    path = open(os.path.join(ROOT, PKG_NAME, "host", "timeable_path_cartesian_spline.h")).read()
    assert "BuildIkTable(" in path
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_kernels.h")).read()
    assert "cw_window(" in kernels and "cw_rows_at(" in kernels      # the kernels call the tested functions


def test_library_cross_compiles_and_resource_usage_is_recorded():
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    so = eng.build_library()
    assert os.path.exists(so)
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, re.M), name
    usage = open(os.path.join(ROOT, "profiles", "cartesian_set_resource_usage.txt")).read()
    for kernel in ("k_cartesian_lp<1, 6>", "k_cartesian_lp<1, 7>", "k_cartesian_rows", "k_plan_begin", "k_plan_end",
                   "k_plan_project", "k_pset_prologue"):
        block = usage[usage.index(kernel):]
        assert "before:" in block and "after:" in block, kernel
    # no touched kernel spills or loses occupancy
    for m in re.finditer(r"before: (.*)\n\s+after:\s+(.*)", usage):
        b = dict(re.findall(r"(\S+(?: Spill)?) (\d+)", m.group(1)))
        a = dict(re.findall(r"(\S+(?: Spill)?) (\d+)", m.group(2)))
        if not b:
            continue
        assert int(a["Occupancy"]) >= int(b["Occupancy"]), m.group(0)
        assert int(a["ScratchSize"]) == 0 and int(a["VGPRs Spill"]) == 0 and int(a["SGPRs Spill"]) == 0, m.group(0)

"""Discarding consumed IK rows on the CPU: cw_window_need_from, cw_discard_floor and the compaction
schedule cw_compact_* (csrc/tpamd_cartesian_window.h), compiled for the host
(tests/cpp/test_cartesian_discard_window.cc); the same driver stand-alone under AddressSanitizer and
UndefinedBehaviorSanitizer; the built library exports the new entry points and the binding loads
them. No GPU needed."""
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME
from native_driver import build_driver

ENTRIES = ("tpamd_planner_set_discard_ik_rows", "tpamd_planner_set_ik_table_info",
           "tpamd_planner_set_download_ik_rows", "tpamd_planner_set_ik_table_device_pointers")
SRC = os.path.join(ROOT, "tests", "cpp", "test_cartesian_discard_window.cc")


def _run(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    print(out.stderr[-3000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    counts = {}
    for line in out.stdout.splitlines():
        if ":" in line and line.rsplit(":", 1)[1].strip().isdigit():
            counts[line.rsplit(":", 1)[0]] = int(line.rsplit(":", 1)[1])
    return counts, out


def _check_counts(counts):
    assert counts["need_from equal at first_row 0"] == 6000 and counts["rounding ties"] >= 1000
    assert counts["below first_row"] > 1000 and counts["at or above first_row"] > 1000
    assert counts["malformed either way"] > 100
    assert counts["floor attained"] > 5000 and counts["later starts"] == 20 * counts["floor attained"]
    assert counts["floor zero by rule"] > 3000 and counts["floor positive"] > 1000
    # lengths 1..40 x every (threads, unroll) with threads * unroll in 1..8 x every shift 0..len-1
    assert counts["compaction schedules"] == 20 * sum(range(1, 41)) and counts["overlapping moves"] > 1000


def test_need_from_floor_and_compaction_schedule(tmp_path):
    exe = build_driver(SRC, tmp_path, libs=("m",), opt="-O2")
    counts, _ = _run(exe)
    _check_counts(counts)


def test_driver_is_clean_under_sanitizers(tmp_path):
    """The same driver as a stand-alone program with its own main, built with
    -fsanitize=address,undefined: host code only, nothing preloaded."""
    exe = build_driver(SRC, tmp_path, libs=("m",), name="test_cartesian_discard_window_san",
                       flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    counts, out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    _check_counts(counts)


def test_library_exports_the_discard_entries_and_binds_them():
    """The built library defines every new entry point, the header declares it and the ctypes
    binding loads with it."""
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    so = eng.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert name in eng.ABI_SYMBOLS, name
        assert "int %s(" % name in hdr, name
    L = eng.load_library()
    for name in ENTRIES:
        assert getattr(L, name).argtypes, name
    for name in ("discard_ik_rows", "ik_table_info", "download_ik_rows"):
        assert callable(getattr(eng.PlannerSet, name)), name

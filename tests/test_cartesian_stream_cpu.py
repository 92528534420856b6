"""Streaming IK tables on the CPU: cw_window_need (csrc/tpamd_cartesian_window.h), the three-way
window rule behind tpamd_planner_set_plan_streaming / _plan_resume, compiled for the host and held
against a restatement of TimeableCartesianSplinePath::SamplePath's index arithmetic; the host
simulation of suspend / append / resume (tests/cpp/test_cartesian_stream_window.cc); the same driver
stand-alone under AddressSanitizer and UndefinedBehaviorSanitizer; the built library exports the new
entry points and the binding loads them. No GPU needed."""
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME
from native_driver import build_driver

ENTRIES = ("tpamd_planner_set_append_ik_rows", "tpamd_planner_set_append_ik_rows_device",
           "tpamd_planner_set_plan_streaming", "tpamd_planner_set_plan_resume",
           "tpamd_sample_ik_target_rows_host", "tpamd_sample_ik_target_rows_device")
SRC = os.path.join(ROOT, "tests", "cpp", "test_cartesian_stream_window.cc")


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


def test_window_need_matches_the_reference_rule_and_the_state_machine(tmp_path):
    exe = build_driver(SRC, tmp_path, libs=("m",), opt="-O2")
    counts, _ = _run(exe)
    assert counts["resident"] > 1000 and counts["needs rows"] > 1000 and counts["malformed"] > 100
    for name in ("rounding ties", "negative starts", "rows = last", "rows = last + 1", "rows = last + 2"):
        assert counts[name] > 0, counts
    assert counts["state machines"] == 200 and counts["suspensions"] > counts["state machines"]


def test_window_need_driver_is_clean_under_sanitizers(tmp_path):
    """The same driver as a stand-alone program with its own main, built with
    -fsanitize=address,undefined: host code only, nothing preloaded."""
    exe = build_driver(SRC, tmp_path, libs=("m",), name="test_cartesian_stream_window_san",
                       flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"))
    counts, out = _run(exe)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    assert counts["needs rows"] > 1000


def test_library_exports_the_streaming_entries_and_binds_them():
    """The built library defines every new entry point and the ctypes binding loads with them."""
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    so = eng.build_library()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    for name in ENTRIES:
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert name in eng.ABI_SYMBOLS, name
    L = eng.load_library()
    for name in ENTRIES:
        assert getattr(L, name).argtypes, name

"""Ragged Cartesian batches on the CPU: the per-path row arithmetic of csrc/tpamd_cartesian_window.h
compiled for the host against the oracle's set-up of every path alone (tests/cpp/
test_cartesian_ragged_rows.cc), the mirror's bucketing on length lists with known buckets
(tests/cpp/test_cartesian_buckets.cc), and the new entry points declared, defined, exported and
bound. No GPU needed."""
import importlib
import inspect
import os
import re
import subprocess

from conftest import ROOT, PKG_NAME
from native_driver import build_driver, run_driver

ENTRIES = ("tpamd_time_cartesian_paths_ragged_device", "tpamd_time_cartesian_paths_ragged_host",
           "tpamd_optimize_rows_ragged_device", "tpamd_optimize_rows_ragged_host")


def _run(exe):
    return run_driver(exe, timeout=300, tail=3000)


def test_ragged_row_arithmetic_matches_the_oracle_per_path(tmp_path):
    out = _run(build_driver("test_cartesian_ragged_rows.cc", tmp_path, libs=("oracle", "m"), opt="-O2"))
    # five joint counts, two layouts, two paths of each count in {3, 4, 5, 64}
    assert "samples: %d" % (5 * 2 * 2 * (3 + 4 + 5 + 64)) in out
    assert "refused: %d" % (5 * 4 * 70) in out


def test_mirror_buckets_on_known_length_lists(tmp_path):
    _run(build_driver("test_cartesian_buckets.cc", tmp_path, fp_contract_off=False,
                      flags=("-I" + os.path.join(ROOT, "include"),)))


def test_ragged_entry_points_are_declared_exported_and_bound():
    eng = importlib.import_module(PKG_NAME + ".engine")
    so = eng.build_library()
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    capi = open(os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_capi.hip")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    lib = eng.load_library()
    for name in ENTRIES:
        assert "int %s(" % name in hdr, name
        assert re.search(r"^int %s\(" % name, capi, re.M), name
        assert re.search(r" T %s$" % name, syms, re.M), name
        assert name in eng.ABI_SYMBOLS and getattr(lib, name).argtypes, name
    # the ragged kernels are instances of their own: the uniform ones are still there
    kern = subprocess.run(["strings", so], capture_output=True, text=True, check=True).stdout
    for k in ("k_setup_cartesian_ragged", "k_cartesian_rows_ragged", "k_setup_rows_ragged"):
        assert k in kern, k
    sig = inspect.signature(eng.Engine.time_cartesian_paths).parameters
    assert sig["num_samples_per_path"].default is None and sig["first_row"].default is None
    assert inspect.signature(eng.Engine.optimize_rows).parameters["num_samples_per_path"].default is None
    mirror = open(os.path.join(ROOT, PKG_NAME, "host", "batch_cartesian_timing.h")).read()
    assert "EngineCallsOfLastCompute()" in mirror and "CartesianTimingBuckets(" in mirror
    impl = open(os.path.join(ROOT, PKG_NAME, "host", "batch_cartesian_timing.cc")).read()
    assert "tpamd_time_cartesian_paths_ragged_host(" in impl
    kernels = open(os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_kernels.h")).read()
    assert "cw_rows_ragged_at(" in kernels and "cw_ragged_count(" in kernels   # the kernels call the tested functions

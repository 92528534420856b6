"""CPU-side checks of the enqueued-only Plan (tpamd_planner_set_plan_device): the library builds
for gfx950 and exports the new symbols, the structs and constants of the Python binding match
include/tpamd.h, and the host mirror's new methods compile. No compute here."""
import ctypes
import importlib
import os
import re
import subprocess

import pytest

from conftest import PKG_NAME, ROOT

NEW_SYMBOLS = ("tpamd_planner_set_reserve", "tpamd_planner_set_capacity", "tpamd_planner_set_plan_device")


@pytest.fixture(scope="module")
def eng():
    m = importlib.import_module(PKG_NAME + ".engine")
    m.build_library()
    return m


def _header():
    return open(os.path.join(ROOT, "include", "tpamd.h")).read()


def test_library_exports_the_new_symbols(eng):
    lib = eng.load_library()
    for name in NEW_SYMBOLS:
        assert name in eng.ABI_SYMBOLS
        assert hasattr(lib, name), name
    assert lib.tpamd_version() == 200
    assert "--offload-arch=gfx950" in eng.HIPCC_FLAGS


def test_info_struct_is_32_bytes_and_matches_the_header(eng):
    assert ctypes.sizeof(eng._PlanDeviceInfo) == 32
    body = re.search(r"typedef struct tpamd_plan_device_info \{(.*?)\} tpamd_plan_device_info;", _header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        assert decl.startswith("int32_t "), decl
        fields += [f.strip() for f in decl[len("int32_t "):].split(",")]
    assert fields == list(eng.PLAN_DEVICE_INFO_FIELDS) + ["reserved[2]"]
    assert [n for n, _ in eng._PlanDeviceInfo._fields_] == list(eng.PLAN_DEVICE_INFO_FIELDS) + ["reserved"]


def test_resource_exhausted_is_8_and_distinct(eng):
    codes = dict((m.group(1), int(m.group(2)))
                 for m in re.finditer(r"#define (TPAMD_PLAN_[A-Z_]+) (\d+)", _header()))
    assert codes["TPAMD_PLAN_RESOURCE_EXHAUSTED"] == 8 == eng.PLAN_RESOURCE_EXHAUSTED
    assert len(set(codes.values())) == len(codes) and len(codes) >= 9
    # the TPAMD_PLAN_* codes have no string table in the C-ABI (tpamd_error_string names the
    # TPAMD_E_* call-level errors); the mirror maps the new code to a Status of its own
    host = open(os.path.join(ROOT, PKG_NAME, "host", "path_timing_trajectory_set.cc")).read()
    assert "case TPAMD_PLAN_RESOURCE_EXHAUSTED:" in host and "ResourceExhaustedError(" in host


def test_header_declares_the_entry_as_specified():
    hdr = re.sub(r"\s+", " ", _header())
    assert ("int tpamd_planner_set_plan_device(tpamd_planner_set *set, const int64_t *start_ns, "
            "const int64_t *horizon_ns, int max_windows, tpamd_planner_summary *summary, "
            "tpamd_plan_device_info *info, void *hip_stream);") in hdr
    assert "int tpamd_planner_set_reserve(tpamd_planner_set *set, int history_capacity, int trajectory_capacity);" in hdr
    assert "int tpamd_planner_set_capacity(const tpamd_planner_set *set, int32_t *history, int32_t *trajectory);" in hdr


def test_host_mirror_compiles_with_the_new_methods(eng):
    host = os.path.join(ROOT, PKG_NAME, "host")
    subprocess.check_call(["make", "-C", host, "-s"])
    hdr = open(os.path.join(host, "path_timing_trajectory_set.h")).read()
    for decl in ("Status Reserve(int history, int trajectory);",
                 "Status PlanDevice(const int64_t *start_ns_dev, const int64_t *horizon_ns_dev, int max_windows, "
                 "void *hip_stream);",
                 "std::vector<Status> FinishPlanDevice();"):
        assert decl in hdr, decl
    lib = ctypes.CDLL(os.path.join(host, "libtp_host.so"))
    syms = subprocess.run(["nm", "-D", "--defined-only", lib._name], capture_output=True, text=True).stdout
    for name in ("PlanDevice", "FinishPlanDevice", "Reserve"):
        assert re.search(r"PathTimingTrajectorySet\d+%s" % name, syms), name


def test_python_class_has_the_new_methods(eng):
    for name in ("reserve", "capacity", "plan_async"):
        assert callable(getattr(eng.PlannerSet, name))
    assert callable(eng.PlanHandle.result)

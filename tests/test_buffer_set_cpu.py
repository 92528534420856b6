"""Trajectory buffers on the CPU: the mirror's TrajectoryBuffer (host/trajectory_buffer.cc) on the
reference's test cases for InsertSegment, AppendSample, DiscardSegmentBefore, GetPositionsUpToTime,
AddOffsetToTimestamps and the sequence number, and the host/device core of csrc/tpamd_buffer.h,
compiled for the host, bit-equal to a mirror buffer after every operation of seeded random
operation sequences (tests/cpp/test_buffer_core.cc). No GPU needed."""
import os
import re

from conftest import ROOT, PKG_NAME
from native_driver import build_driver, run_driver

CATEGORIES = (
    "insert: empty segment", "insert: into an empty buffer", "insert: at or before the front (sequence back to 0)",
    "insert: exactly at the last sample", "insert: within tolerance just after a sample (replaced)",
    "insert: just outside tolerance (kept)", "insert: strictly inside",
    "discard: empty buffer", "discard: at or before the front", "discard: after the back (cleared)",
    "discard: on a sample", "discard: within tolerance of the sample before", "discard: interpolated new first sample",
    "stop: NotFound", "stop: at-rest mid (Internal)", "stop: before the front (OutOfRange)", "stop: index out of range",
    "stop: clamped beyond the end", "stop: empty (OK)", "stop: bad max_acceleration", "stop: bad time_step",
    "stop: non-increasing times", "stop: sequence moved", "stop: sequence unchanged (at-rest last sample)",
    "append: behind the last sample", "append: not behind the last sample (InvalidArgument)", "offset", "clear",
    "capacity: compaction taken", "capacity: TPAMD_PLAN_MORE, buffer unchanged",
)


def test_buffer_core_matches_mirror_bit_for_bit(tmp_path):
    exe = build_driver("test_buffer_core.cc", tmp_path, opt="-O2",
                       extra_sources=("host/rescale_to_stop.cc", "host/trajectory_buffer.cc"))
    out = run_driver(exe, timeout=600, tail=5000)
    assert "reference cases: done" in out
    counts = {}
    for line in out.splitlines():
        if line.startswith("category "):
            name, n = line[len("category "):].rsplit(":", 1)
            counts[name.strip()] = int(n)
        if line.startswith("operations:"):
            assert int(line.split(":")[1]) >= 20000
    for cat in CATEGORIES:
        assert counts.get(cat, 0) > 0, (cat, counts)
    assert not any(name.startswith("stop: other") for name in counts), counts


def test_buffer_set_exports_are_declared():
    """The buffer-set entry points are in the header, registered with the binding and built into
    the host library; every operation has a host-pointer and a _device entry."""
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    src = open(os.path.join(ROOT, PKG_NAME, "engine.py")).read()
    capi = open(os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_capi.hip")).read()
    ops = ("insert", "insert_from_planner_set", "append_sample", "discard_before", "stop_before_time",
           "sample_at_ticks", "add_offset", "clear", "info", "download")
    names = ["tpamd_buffer_set_create", "tpamd_buffer_set_reserve"]
    for op in ops:
        names += ["tpamd_buffer_set_" + op, "tpamd_buffer_set_" + op + "_device"]
    import importlib
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    for name in names:
        assert "int %s(" % name in hdr, name
        assert re.search(r"^int %s\(" % name, capi, re.M), name
        assert name in eng.ABI_SYMBOLS and len(getattr(lib, name).argtypes) >= 2, name
    assert "void tpamd_buffer_set_destroy(" in hdr and "size_t tpamd_buffer_set_device_bytes(" in hdr
    assert "typedef struct tpamd_buffer_set tpamd_buffer_set;" in hdr
    assert os.path.join(ROOT, PKG_NAME, "csrc", "tpamd_buffer.h") in eng._abi.library_sources()
    assert "class BufferSet" in src
    mk = open(os.path.join(ROOT, PKG_NAME, "host", "Makefile")).read()
    assert "trajectory_buffer_set.cc" in mk
    cls = open(os.path.join(ROOT, PKG_NAME, "host", "trajectory_buffer_set.h")).read()
    for method in ("InsertSegments", "InsertFromPlannerSet", "AppendSamples", "DiscardSegmentsBefore", "StopBeforeTimes",
                   "GetSetpoints", "AddOffsetsToTimestamps", "Clear", "GetInfo", "GetSamples", "Reserve"):
        assert method + "(" in cls, method
    mirror = open(os.path.join(ROOT, PKG_NAME, "host", "trajectory_buffer.h")).read()
    for method in ("Reserve", "GetStartTime", "GetEndTime", "GetSequenceNumber", "AppendSample", "DiscardSegmentBefore",
                   "GetPositionsUpToTime", "AddOffsetToTimestamps"):
        assert method + "(" in mirror, method

"""CPU-side checks of the drop-in boundary: the C-ABI library builds for gfx950,
loads, exports every symbol include/tpamd.h declares, and refuses to run
without a GPU (no CPU fallback). No compute calls here."""
import ctypes
import importlib
import os
import re

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT


@pytest.fixture(scope="module")
def eng():
    m = importlib.import_module(PKG_NAME + ".engine")
    m.build_library()
    return m


def test_header_symbols_are_all_exported(eng):
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tpamd_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 26
    assert declared == set(eng.ABI_SYMBOLS)
    lib = eng.load_library()
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.tpamd_version() == 200
    assert lib.tpamd_error_string(7).decode().startswith("could not connect")
    # every function carries the restype and argtypes of its declaration; a struct mirror goes to
    # its parameters by value (ctypes passes the reference) or by byref
    protos = eng._abi.parse_prototypes(open(os.path.join(ROOT, "include", "tpamd.h")).read())
    assert list(protos) == eng.ABI_SYMBOLS and len(protos) == 147
    for name, (restype, argtypes) in protos.items():
        f = getattr(lib, name)
        assert f.restype == restype and list(f.argtypes) == argtypes, name
    assert lib.tpamd_planner_set_sample_at_ticks.argtypes[4] is ctypes.c_int64
    assert lib.tpamd_rebuild_time_device.argtypes[4] is ctypes.c_size_t
    assert lib.tpamd_engine_destroy.restype is None and lib.tpamd_profile_mean_ms.restype is ctypes.c_double
    # NULL engine: refused before anything is read, whichever way the struct goes in
    bt = eng._JointBatch(1, 7, 100, 4, 0, 0, 0.8)
    ji, po = eng._JointInputs.from_dict({}), eng._PathOutputs.from_dict({})
    assert lib.tpamd_time_joint_paths_host(None, bt, ji, po) == lib.tpamd_time_joint_paths_host(
        None, ctypes.byref(bt), ctypes.byref(ji), ctypes.byref(po)) != 0


def test_multi_device_header_symbols_are_all_exported(eng):
    """include/tpamd_multi.h against libtpamd_multi.so (loads RCCL; no device call)."""
    hdr = open(os.path.join(ROOT, "include", "tpamd_multi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(tpamd_[a-z0-9_]+)\s*\(", hdr))
    assert declared == {"tpamd_multi_create", "tpamd_multi_destroy", "tpamd_multi_num_devices", "tpamd_multi_device",
                        "tpamd_multi_engine", "tpamd_multi_uses_rccl", "tpamd_gather_bytes_per_path",
                        "tpamd_multi_time_joint_paths_host", "tpamd_multi_time_joint_groups_host"}
    eng.load_library()
    lib = ctypes.CDLL(eng.build_multi_library())
    for name in sorted(declared):
        assert hasattr(lib, name), name
    lib.tpamd_gather_bytes_per_path.restype = ctypes.c_size_t
    assert lib.tpamd_gather_bytes_per_path(0, 2000, 7) == 32016      # compact: 16 N + 16
    assert lib.tpamd_gather_bytes_per_path(2, 2000, 7) == 160000     # full: north_star's t, sd, sdd... + q


def test_planner_set_struct_layouts_match_header(eng):
    class Cfg(ctypes.Structure):
        _fields_ = [(n, ctypes.c_int32) for n in ("a", "b", "c", "d", "e", "f", "g", "h")] + \
                   [("x", ctypes.c_double), ("y", ctypes.c_double), ("z", ctypes.c_int64)]
    assert ctypes.sizeof(Cfg) == 56                                   # tpamd_planner_set_config
    # tpamd_planner_summary: 3 x int64 + 8 x int32 (the device-side record has the same layout)
    assert 3 * 8 + 8 * 4 == 56


def test_struct_layouts_match_header(eng):
    # sizes implied by the C declarations (LP64): 6 int32 + double; 9 / 10 pointers; ...
    assert ctypes.sizeof(eng._JointBatch) == 32
    assert ctypes.sizeof(eng._JointInputs) == 80
    assert ctypes.sizeof(eng._PathOutputs) == 88
    assert ctypes.sizeof(eng._RowsBatch) == 16
    assert ctypes.sizeof(eng._RowsInputs) == 72
    assert ctypes.sizeof(eng._ResampleArgs) == 16 + 9 * 8 + 8 + 8 + 8 * 8


def _mirrors(eng):
    """Every ctypes mirror the binding exports, by the name of its C struct."""
    found = {}
    for value in vars(eng).values():
        if isinstance(value, type) and issubclass(value, ctypes.Structure) and getattr(value, "_c_name_", None):
            found[value._c_name_] = value
    return found


def test_every_mirror_has_the_layout_the_compiler_gives_its_struct(eng, tmp_path):
    """sizeof and every field's offsetof of each mirrored struct, printed by a C++ program that
    includes include/tpamd.h and names the fields as the mirror does (a field the header lacks
    does not compile), against ctypes.sizeof and the ctypes field offsets."""
    from native_driver import build_driver, run_driver
    mirrors = _mirrors(eng)
    assert len(mirrors) == 20
    lines = ['#include <cstddef>', '#include <cstdio>', '#include "tpamd.h"', 'int main() {']
    for c_name, mirror in sorted(mirrors.items()):
        lines.append('  std::printf("%s sizeof %%zu\\n", sizeof(%s));' % (c_name, c_name))
        for field, _ in mirror._fields_:
            lines.append('  std::printf("%s %s %%zu\\n", offsetof(%s, %s));' % (c_name, field, c_name, field))
    lines += ['  std::printf("ALL OK\\n");', '  return 0;', '}']
    source = tmp_path / "struct_layouts.cc"
    source.write_text("\n".join(lines) + "\n")
    exe = build_driver(str(source), tmp_path, flags=("-I" + os.path.join(ROOT, "include"),))
    compiled = {}
    for line in run_driver(exe, tail=0).splitlines()[:-1]:
        c_name, what, value = line.split()
        compiled[c_name, what] = int(value)
    expected = {}
    for c_name, mirror in mirrors.items():
        expected[c_name, "sizeof"] = ctypes.sizeof(mirror)
        for field, _ in mirror._fields_:
            expected[c_name, field] = getattr(mirror, field).offset
    assert compiled == expected
    assert len(expected) > 150          # 20 structs, every field


def test_prototype_parser_on_literal_declarations(eng):
    from ctypes import POINTER, c_char_p, c_double, c_int, c_int64, c_size_t, c_void_p
    text = """
    /* int tpamd_in_a_comment(int x); */
    int tpamd_version(void);
    const char *tpamd_error_string(int code);
    size_t tpamd_engine_workspace_bytes(const tpamd_engine *engine);
    void tpamd_engine_destroy(tpamd_engine *engine);
    int tpamd_time_joint_paths_device(tpamd_engine *engine, const tpamd_joint_batch *batch,
                                      const tpamd_joint_inputs *in,
                                      const tpamd_path_outputs *out, void *hip_stream);
    int tpamd_some_readout(tpamd_planner_set *set, int count, const int32_t *ids, const int64_t *start_ns,
                           int64_t step_ns, int32_t num_ticks, double time_step, double *q, size_t bytes,
                           tpamd_planner_check *records, tpamd_engine **out);
    """
    got = eng._abi.parse_prototypes(text)
    assert got == {
        "tpamd_version": (c_int, []),
        "tpamd_error_string": (c_char_p, [c_int]),
        "tpamd_engine_workspace_bytes": (c_size_t, [c_void_p]),
        "tpamd_engine_destroy": (None, [c_void_p]),
        "tpamd_time_joint_paths_device": (c_int, [c_void_p, POINTER(eng._JointBatch), POINTER(eng._JointInputs),
                                                  POINTER(eng._PathOutputs), c_void_p]),
        # a record array the call writes is an address like any other array, mirrored or not
        "tpamd_some_readout": (c_int, [c_void_p, c_int, c_void_p, c_void_p, c_int64, c_int, c_double, c_void_p,
                                       c_size_t, c_void_p, c_void_p]),
    }
    for bad in ("int tpamd_x(float gain);", "float tpamd_x(int a);", "int tpamd_x(tpamd_joint_batch by_value);",
                "char *tpamd_x(void);", "int tpamd_x(unsigned n);"):
        with pytest.raises(eng.TpamdError, match="no ctypes type"):
            eng._abi.parse_prototypes(bad)


def test_no_gpu_means_loud_failure(eng):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(eng.TpamdError):
        eng.Engine(0)


def test_product_does_not_touch_the_oracle():
    """The shipped package must never import, link or call anything under oracle/."""
    pkg_dir = os.path.join(ROOT, PKG_NAME)
    for dirpath, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".cc", ".cpp", ".hpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "tp_oracle" not in text and "oracle." not in text.replace("oracle's", ""), f
                assert "from oracle" not in text and "import oracle" not in text, f


def test_environment_switches_are_the_documented_ones():
    """Every TPAMD_* variable the native code reads is in the table of INTEGRATION.md section 4, and
    the table lists nothing else (TPAMD_LIBRARY is read by the ctypes binding). Text only."""
    read = set()
    for sub in ("csrc", "host"):
        for dirpath, _, files in os.walk(os.path.join(ROOT, PKG_NAME, sub)):
            for f in files:
                if f.endswith((".h", ".hip", ".cc", ".cpp", ".hpp")):
                    text = open(os.path.join(dirpath, f)).read()
                    read |= set(re.findall(r'getenv\(\s*"(TPAMD_[A-Z0-9_]+)"', text))
                    assert len(re.findall(r"getenv\(", text)) == len(re.findall(r'getenv\(\s*"TPAMD_', text)), f
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    section = doc[doc.index("## 4. Environment switches"):]
    section = section.split("\n## ", 1)[0]
    rows = [ln for ln in section.splitlines() if ln.startswith("| `TPAMD_")]
    documented = set()
    for ln in rows:
        documented |= set(re.findall(r"`(TPAMD_[A-Z0-9_]+)`", ln.split("|")[1]))
    assert read == documented - {"TPAMD_LIBRARY"}
    assert read == {"TPAMD_FORCE_GENERIC", "TPAMD_ORDER_RAGGED", "TPAMD_FRONT_DELAY_US", "TPAMD_DEVICE"}


def test_synthetic_generator_is_deterministic_and_matches_spec():
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    from oracle import tpo
    a = syn.make_joint_batch(5, 7, 500)
    b = syn.make_joint_batch(3, 7, 500, first_path_index=2)
    np.testing.assert_array_equal(a["control_points"][2:], b["control_points"])
    np.testing.assert_array_equal(a["knots"][2:], b["knots"])
    assert a["control_points"].shape == (5, 28, 7) and a["knots"].shape == (5, 31)
    assert np.all((a["vmax"] >= 1) & (a["vmax"] < 2)) and np.all((a["amax"] >= 2) & (a["amax"] < 4))
    assert np.all(np.abs(a["waypoints"]) <= 2)
    np.testing.assert_allclose(a["delta"] * 499, a["knots"][:, -1], rtol=1e-15)
    # first splitmix64 output for seed 0x5EEDC0DE00000000 (path 0), checked independently
    x = (0x5EEDC0DE00000000 + 0x9E3779B97F4A7C15) & (2**64 - 1)
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2**64 - 1)
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2**64 - 1)
    z ^= z >> 31
    assert a["waypoints"][0, 0, 0] == (z >> 11) * 2.0 ** -53 * 4.0 - 2.0
    # the host-side fit restates the same rule as the oracle's restatement of the reference
    for i in range(5):
        cps, knots = tpo.joint_fit_spline(a["waypoints"][i], 0.2)
        np.testing.assert_array_equal(cps, a["control_points"][i])
        np.testing.assert_array_equal(knots, a["knots"][i])

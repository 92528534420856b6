"""CPU side of the waypoint batches: the four exports and their prototypes, and joint_fit_path (the body
of k_fit_joint_waypoints, csrc/tpamd_joint_fit.h) run on the host by a stand-alone program built with
the address and undefined-behaviour sanitizers (tests/cpp/test_joint_fit_layout.cc). Its packed and
strided outputs are held bit-equal to tpo.joint_fit_spline at D = 1, 7, 16 and W = 0, 1, 2, 11; the
offsets of both layouts are restated in numpy here and every value outside a path's own slots must
still be the sentinel."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from native_driver import build_driver

NEW_EXPORTS = ("tpamd_fit_joint_waypoints_host", "tpamd_fit_joint_waypoints_device",
               "tpamd_time_waypoint_paths_host", "tpamd_time_waypoint_paths_device")
WAYPOINT_COUNTS = [2, 0, 11, 1, 2, 11, 0, 1]
SAMPLES = [3, 63, 64, 65, 257, 300, 17, 300]
N = 300


def test_exports_and_prototypes():
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    lib = eng.load_library()
    hdr = open(os.path.join(ROOT, "include", "tpamd.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_EXPORTS:
        assert hasattr(lib, name), name
        assert name in eng.ABI_SYMBOLS
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, code)
        assert m, "no prototype of %s in include/tpamd.h" % name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[0] == "tpamd_engine *engine"
        assert (params[-1] == "void *hip_stream") == name.endswith("_device")
        assert len(getattr(lib, name).argtypes) == len(params)
    assert re.search(r"#define\s+TPAMD_PATH_NO_WAYPOINTS\s+11\b", code)
    assert lib.tpamd_error_string(11).decode() == "path without waypoints"
    assert eng.PATH_STATUS[11] == "no_waypoints"
    for struct, fields in (("tpamd_waypoint_batch", 5), ("tpamd_waypoint_inputs", 9),
                           ("tpamd_waypoint_fit_outputs", 5)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        assert body.count(";") == fields
    assert len(eng._WaypointBatch._fields_) == 5 and len(eng._WaypointInputs._fields_) == 9
    assert len(eng._WaypointFitOutputs._fields_) == 5


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_driver("test_joint_fit_layout.cc", tmp_path_factory.mktemp("joint_fit"),
                        flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _fit_points(W):
    return np.where(W < 1, 0, np.where(W == 1, 4, 3 * W - 2))


def _run(program, D, paths, rounding, delta_in):
    B = len(paths)
    W = np.array([len(p) for p in paths])
    P = _fit_points(W)
    offsets = np.concatenate([[0], np.cumsum(W)])
    # the packed layout, restated: points behind each other, knots too, three more per path with points
    point_offsets = np.concatenate([[0], np.cumsum(P)])
    knot_offsets = np.concatenate([[0], np.cumsum(P + 3 * (P > 0))])
    S = max(4, int(P.max()))
    hx = lambda a: " ".join(float(x).hex() for x in np.asarray(a, dtype=np.float64).reshape(-1))
    it = lambda a: " ".join(str(int(x)) for x in a)
    text = "\n".join(["%d %d %d %d" % (D, B, S, N), it(offsets), it(point_offsets[:-1]), it(knot_offsets[:-1]),
                      "%d %d" % (point_offsets[-1], knot_offsets[-1]), it(SAMPLES), hx(rounding), hx(delta_in),
                      hx(np.concatenate([p.reshape(-1) for p in paths]))]) + "\n"
    out = subprocess.run([program], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    got = {}
    for line in out.stdout.splitlines():
        name, n, *vals = line.split()
        assert len(vals) == int(n)
        integer = name.split("_")[1] in ("np", "status", "samples")
        got[name] = np.array([int(v) if integer else float.fromhex(v) for v in vals],
                             dtype=np.int32 if integer else np.float64)
    return got, P, point_offsets, knot_offsets, S


@pytest.mark.parametrize("D", [1, 7, 16])
def test_host_fit_in_both_layouts_is_the_oracles(program, D):
    from oracle import tpo
    tpo.build()
    rng = np.random.default_rng(40 + D)
    paths = [rng.uniform(-1, 1, size=(W, D)) for W in WAYPOINT_COUNTS]
    B = len(paths)
    rounding = np.array([0.2, 0.0, 0.05, 0.0, 0.3, 0.0, 0.2, 0.1])
    delta_in = rng.uniform(0.001, 0.01, size=B)
    got, P, po, ko, S = _run(program, D, paths, rounding, delta_in)
    same = lambda a, b, what: (a.shape == b.shape and a.tobytes() == b.tobytes()) or pytest.fail(str(what))
    assert (got["packed_np"] == P).all() and (got["whole_np"] == P).all() and (got["given_np"] == P).all()
    np.testing.assert_array_equal(got["packed_status"], np.where(P == 0, 3, 0))
    for tag in ("whole", "given"):
        np.testing.assert_array_equal(got[tag + "_status"], np.where(P == 0, 11, -7))   # the sweep writes the others
        assert not got[tag + "_zero"].any()
    np.testing.assert_array_equal(got["whole_samples"], np.where(P == 0, 0, N))
    np.testing.assert_array_equal(got["given_samples"], np.where(P == 0, 0, SAMPLES))
    same(got["given_delta"], delta_in, "given deltas pass through")
    packed_k, packed_c = got["packed_knots"].copy(), got["packed_cps"].reshape(-1, D).copy()
    for tag, rnd in (("packed", rounding), ("given", rounding), ("whole", np.full(B, 0.2))):
        for k in range(B):
            Pk = int(P[k])
            if tag != "packed":
                kn = got[tag + "_knots"].reshape(B, S + 3)[k]
                cp = got[tag + "_cps"].reshape(B, S, D)[k]
                assert (kn[Pk + 3 if Pk else 0:] == -7.0).all() and (cp[Pk:] == -7.0).all(), (tag, k)
                kn, cp = kn[:Pk + 3], cp[:Pk]
            else:
                kn = got["packed_knots"][ko[k]:ko[k + 1]]
                cp = got["packed_cps"].reshape(-1, D)[po[k]:po[k + 1]]
            if Pk == 0:
                assert kn[:0].size == 0 and got[tag + "_end"][k] == 0.0
                continue
            ocp, okn = tpo.joint_fit_spline(paths[k], rnd[k])
            assert ocp.shape == (Pk, D) and okn.shape == (Pk + 3,)
            same(cp, ocp, (tag, "control points", k))
            same(kn, okn, (tag, "knots", k))
            same(got[tag + "_end"][k:k + 1], okn[-1:], (tag, "path_end", k))
            if tag == "whole":
                same(got["whole_delta"][k:k + 1], np.array([okn[-1] / np.float64(N - 1)]), "delta of the whole path")
    # the packed arrays are exactly as long as the restated offsets say and were written everywhere
    assert packed_k.shape == (ko[-1],) and packed_c.shape == (po[-1], D)
    assert not (packed_k == -7.0).any() and not (packed_c == -7.0).any()

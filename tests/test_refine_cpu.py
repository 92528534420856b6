"""CPU side of the refined batch calls (include/tpamd.h tpamd_time_*_paths_refined_*): the four
exports and their prototypes; the decisions of csrc/tpamd_refine.h run on the host by a stand-alone
program built with the address and undefined-behaviour sanitizers (tests/cpp/test_refine_logic.cc),
held equal to a numpy restatement; and the oracle's statement of the whole loop
(tests/refine_reference.py) on the shapes the GPU tests use, with the conditions that keep those
tests from becoming vacuous."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import PKG_NAME, ROOT
from native_driver import build_driver

import refine_cases as cases
import refine_reference as rr

NEW_EXPORTS = ("tpamd_time_joint_paths_refined_device", "tpamd_time_joint_paths_refined_host",
               "tpamd_time_waypoint_paths_refined_device", "tpamd_time_waypoint_paths_refined_host")


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
        assert "const tpamd_refine_options *opt" in params and "const tpamd_refine_outputs *ref" in params
        assert len(getattr(lib, name).argtypes) == len(params)
    for struct, fields in (("tpamd_refine_options", 5), ("tpamd_refine_outputs", 9)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), code, flags=re.S).group(1)
        assert body.count(";") == fields
    assert len(eng._RefineOptions._fields_) == 5 and len(eng._RefineOutputs._fields_) == 9
    assert (eng.REFINE_NOTHING, eng.REFINE_NO_SLOT, eng.REFINE_TOO_LONG) == (rr.NOTHING, rr.NO_SLOT, rr.TOO_LONG)


# ------------------------------------------------------------------ the decisions, on the host
@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_driver("test_refine_logic.cc", tmp_path_factory.mktemp("refine_logic"),
                        flags=("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _records(B, max_samples, max_rounds, tolerance, seed):
    """Hand-made round-0 records, one kind after the other: clean, violating, not checked, and an
    excess exactly equal to the tolerance; sample counts around the limit 2 n - 1 == max_samples; and
    for every round a record of the same kinds."""
    rng = np.random.default_rng(seed)
    fits = (max_samples + 1) // 2                  # the largest n with 2 n - 1 <= max_samples
    kinds = [(0, -0.25), (3, tolerance + 0.5), (-1, np.nan), (2, tolerance), (1, np.nextafter(tolerance, np.inf))]
    counts = [fits, fits + 1, 17, 33, (fits + 1) // 2, (fits + 1) // 2 + 1]
    paths = []
    for b in range(B):
        v, x = kinds[b % len(kinds)] if b < 2 * len(kinds) else kinds[rng.integers(len(kinds))]
        n = counts[(b // len(kinds)) % len(counts)] if b < 30 else counts[rng.integers(len(counts))]
        made = [kinds[rng.integers(len(kinds))] for _ in range(max_rounds)]
        paths.append((v, x, int(n), float(rng.uniform(0.01, 0.2)), made))
    return paths


def _restate(paths, M, max_samples, max_rounds, tolerance):
    slot, slot_path, used = rr.slot_map([(p[0], p[1]) for p in paths], [p[2] for p in paths], max_samples, M, tolerance)
    first_samples, first_delta = np.zeros(M, dtype=np.int64), np.zeros(M)
    rounds, num_samples, delta = np.zeros(M, dtype=np.int64), np.zeros(M, dtype=np.int64), np.zeros(M)
    nxt = np.zeros(M, dtype=np.int64)
    live = [used] + [0] * max_rounds
    for k in range(used):
        v, x, n, dl, made = paths[slot_path[k]]
        first_samples[k], first_delta[k] = 2 * n - 1, dl / 2.0
        for r in range(1, max_rounds + 1):
            n, dl = 2 * n - 1, dl / 2.0
            rounds[k], num_samples[k], delta[k] = r, n, dl
            if not (rr.needs_refinement(made[r - 1], tolerance) and r < max_rounds and 2 * n - 1 <= max_samples):
                nxt[k] = 0
                break
            live[r] += 1
            nxt[k] = 2 * n - 1
    return dict(slot=slot, slot_path=slot_path, num_refined=[used], first_samples=first_samples,
                first_delta=first_delta, live=live, rounds=rounds, num_samples=num_samples, delta=delta,
                next_samples=nxt)


@pytest.mark.parametrize("B", [0, 1, 64, 65, 1025])
@pytest.mark.parametrize("max_samples,max_rounds,M,tolerance", [(129, 2, 16, 0.0), (128, 3, 4, 0.125),
                                                                (129, 1, 1, 0.0), (257, 8, 600, 0.0)])
def test_decisions_on_the_host_equal_the_restatement(program, B, max_samples, max_rounds, M, tolerance):
    paths = _records(B, max_samples, max_rounds, tolerance, seed=B * 131 + M)
    hx = lambda x: float(x).hex()
    lines = ["%d %d %d %d %d %s" % (B, M, 65, max_samples, max_rounds, hx(tolerance))]
    for v, x, n, dl, made in paths:
        lines.append(" ".join(["%d %s %d %s" % (v, hx(x), n, hx(dl))] + ["%d %s" % (mv, hx(mx)) for mv, mx in made]))
    out = subprocess.run([program], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-3000:]
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
    want = _restate(paths, M, max_samples, max_rounds, tolerance)
    seen = set()
    for line in out.stdout.splitlines():
        name, n, *vals = line.split()
        assert len(vals) == int(n)
        seen.add(name)
        if name in ("first_delta", "delta"):
            got = np.array([float.fromhex(v) for v in vals])
            assert got.tobytes() == np.asarray(want[name], dtype=np.float64).tobytes(), name
        else:
            assert [int(v) for v in vals] == [int(v) for v in want[name]], name
    assert seen == set(want)
    if B >= 64 and M == 4:
        assert (want["slot"] == rr.NO_SLOT).any()           # more violators than slots
    if B >= 64:
        assert (want["slot"] == rr.TOO_LONG).any() and (want["slot"] >= 0).any()


# ------------------------------------------------------------------ the oracle's statement
@pytest.mark.parametrize("D", cases.DOFS)
def test_oracle_refinement_of_the_shared_shapes(D):
    ref = cases.joint_reference(D)
    refined, two, left, never = cases.summary(ref)
    print("D=%d refined %s two rounds %s still violating %s" % (D, refined, two, left))
    assert len(refined) >= 2
    assert len(two) >= 1
    assert len(never) >= 1
    if D in (1, 7, 8):
        assert len(left) >= 1
    # the slot map is in path order, every history follows n -> 2 n - 1 with delta halved exactly
    assert refined == sorted(refined) and ref["num_refined"] == len(refined)
    batch = cases.joint_batch(D)
    for k, b in enumerate(refined):
        n, dl = cases.SAMPLES, batch["delta"][b]
        assert rr.needs_refinement(ref["round0"][b]["record"], 0.0)
        for made in ref["history"][k]:
            n, dl = 2 * n - 1, dl / 2.0
            assert (made["n"], made["delta"]) == (n, dl)
            assert n <= cases.MAX_SAMPLES
        assert len(ref["history"][k]) == ref["rounds"][k] <= cases.MAX_ROUNDS
        assert (ref["num_samples"][k], ref["delta"][k]) == (n, dl)
        # the old samples are every second new one
        assert dl * 2 ** ref["rounds"][k] == batch["delta"][b]
    for b in never:
        assert not rr.needs_refinement(ref["round0"][b]["record"], 0.0)


def test_slot_overflow_and_sample_limits_in_the_oracle():
    full = cases.joint_reference(7)
    refined = cases.summary(full)[0]
    four = cases.joint_reference(7, max_refined=4)
    assert list(four["slot_path"]) == refined[:4]
    assert [b for b in range(cases.PATHS) if four["slot"][b] == rr.NO_SLOT] == refined[4:]
    short = cases.joint_reference(7, max_samples=65)
    assert short["num_refined"] == len(refined) and (short["rounds"][:len(refined)] == 1).all()
    assert any(f["record"][0] > 0 for f in short["final"] if f)
    none = cases.joint_reference(7, max_samples=64)
    assert none["num_refined"] == 0 and [b for b in range(cases.PATHS) if none["slot"][b] == rr.TOO_LONG] == refined


@pytest.mark.parametrize("D", [7, 16])
def test_waypoint_case_has_refined_paths(D):
    call, joint, ref = cases.waypoint_case(D)
    empty = cases.WAYPOINT_COUNTS.index(0)
    assert ref["num_refined"] >= 2
    assert ref["round0"][empty]["status"] == 11 and ref["slot"][empty] == rr.NOTHING
    assert len({len(k) for k in joint["knots"] if k is not None}) >= 2      # slots of different fill


def test_ragged_builder_gives_refined_paths_and_a_failed_one():
    batch, counts, ref = cases.ragged_batch()
    assert ref["num_refined"] >= 2
    assert ref["round0"][cases.PATHS - 1]["status"] == 4 and ref["slot"][cases.PATHS - 1] == rr.NOTHING
    assert set(counts) == {17, 33, 50}

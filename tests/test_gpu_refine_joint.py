"""Refined joint batches on the GPU (include/tpamd.h tpamd_time_joint_paths_refined_*) against the
engine's own plain entries and the oracle's statement of the loop (tests/refine_reference.py).
Everything is written into sentinel-filled arrays and every comparison is bit equality, NaN by
position. The shapes are those of tests/refine_cases.py, whose conditions tests/test_refine_cpu.py
asserts on the CPU (refined paths, two-round paths, paths that keep violations)."""
import ctypes as C
import importlib

import numpy as np
import pytest

import check_reference as cr
import refine_cases as cases
import refine_reference as rr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

PRE, PRE_INT = -7.25, -9
B, N = cases.PATHS, cases.SAMPLES
PER_SAMPLE = ("time", "s", "sd", "sdd", "sd2")
PER_SAMPLE_D = ("q", "qd", "qdd")
PER_PATH = ("status", "last_extremal_index", "max_time_increment")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev="cuda:0")


def same(a, b):
    """Bit equality, NaN by position."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all()) and np.where(na, 0.0, a).tobytes() == np.where(nb, 0.0, b).tobytes()


def solution_arrays(paths, stride, D, host, env):
    """Sentinel-filled tpamd_path_outputs arrays."""
    shapes = {k: (paths, stride) for k in PER_SAMPLE}
    shapes.update({k: (paths, stride, D) for k in PER_SAMPLE_D})
    shapes.update({k: (paths,) for k in PER_PATH})
    out = {}
    for k, shape in shapes.items():
        integer = k in ("status", "last_extremal_index")
        a = np.full(shape, PRE_INT if integer else PRE, dtype=np.int32 if integer else np.float64)
        out[k] = a if host else env["torch"].from_numpy(a).to(env["dev"])
    return out


def record_arrays(paths, host, env):
    out = {}
    for k in cr.KEYS:
        real = k == "worst_excess"
        a = np.full(paths, PRE if real else PRE_INT, dtype=np.float64 if real else np.int32)
        out[k] = a if host else env["torch"].from_numpy(a).to(env["dev"])
    return out


def refine_arrays(paths, M, NS, D, host, env):
    ints = lambda n: np.full(n, PRE_INT, dtype=np.int32)
    conv = (lambda a: a) if host else (lambda a: env["torch"].from_numpy(a).to(env["dev"]))
    return {"check": record_arrays(paths, host, env), "refined_check": record_arrays(M, host, env),
            "slot": conv(ints(paths)), "slot_path": conv(ints(M)), "num_refined": conv(ints(1)),
            "rounds": conv(ints(M)), "num_samples": conv(ints(M)), "delta": conv(np.full(M, PRE)),
            "refined": solution_arrays(M, NS, D, host, env)}


def to_numpy(x):
    if isinstance(x, dict):
        return {k: to_numpy(v) for k, v in x.items()}
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def engine_inputs(batch, host, env, counts=None, rows=None):
    sel = slice(None) if rows is None else rows
    keys = {"knots": "knots", "control_points": "control_points", "max_velocity": "vmax", "max_acceleration": "amax",
            "path_start": "path_start", "delta": "delta", "sd_start": "sd_start", "time_start": "time_start"}
    inp = {k: np.ascontiguousarray(batch[v][sel], dtype=np.float64) for k, v in keys.items()}
    if counts is not None:
        inp["num_samples_per_path"] = np.ascontiguousarray(counts, dtype=np.int32)
    if not host:
        inp = {k: env["torch"].from_numpy(v).to(env["dev"]) for k, v in inp.items()}
    return inp


def run_refined(env, batch, D, stride=N, max_rounds=cases.MAX_ROUNDS, max_samples=cases.MAX_SAMPLES, M=B,
                tolerance=0.0, counts=None, host=False):
    paths = batch["control_points"].shape[0]
    inp = engine_inputs(batch, host, env, counts)
    out = solution_arrays(paths, stride, D, host, env)
    ref = refine_arrays(paths, M, max_samples, D, host, env)
    got = env["E"].time_joint_paths_refined(inp, out, stride, max_rounds, max_samples, M, tolerance=tolerance,
                                            safety=batch["safety"], refined=ref, host=host)
    if not host:
        env["torch"].cuda.synchronize()
    return to_numpy(out), to_numpy(got)


def run_plain(env, batch, D, stride=N, counts=None, rows=None, delta=None):
    """time_joint_paths + check_joint_paths into sentinel arrays."""
    b = batch if delta is None else dict(batch, delta=delta)
    paths = b["control_points"][slice(None) if rows is None else rows].shape[0]
    inp = engine_inputs(b, False, env, counts, rows)
    out = solution_arrays(paths, stride, D, False, env)
    env["E"].time_joint_paths(inp, out, stride, safety=batch["safety"])
    rec = env["E"].check_joint_paths(inp, out, stride, safety=batch["safety"], outputs=record_arrays(paths, False, env))
    env["torch"].cuda.synchronize()
    return to_numpy(out), to_numpy(rec)


_alone = {}


def solved_alone(env, key, batch, D, b, n, delta):
    """The engine's plain solve of path b alone at (n, delta), once per (case, b, n)."""
    k = (key, b, n)
    if k not in _alone:
        full = np.array(batch["delta"], dtype=np.float64)
        full[b] = delta
        _alone[k] = run_plain(env, batch, D, stride=n, rows=slice(b, b + 1), delta=full)
    return _alone[k]


def assert_slots(env, key, batch, D, got, ref, max_samples, M, oracle=True):
    """Slot map, counters, every used slot against the plain solve of its path alone and against the
    oracle, and the sentinel everywhere else."""
    assert same(got["slot"], ref["slot"]) and same(got["slot_path"], ref["slot_path"])
    assert got["num_refined"][0] == ref["num_refined"]
    assert same(got["rounds"], ref["rounds"]) and same(got["num_samples"], ref["num_samples"])
    assert same(got["delta"], ref["delta"])
    sol = got["refined"]
    for k in range(M):
        b = int(ref["slot_path"][k])
        n = int(ref["num_samples"][k])
        want_rec = ref["refined_check"][k]
        assert cr.same_record(cr.record_of(got["refined_check"], k), want_rec), (k, b)
        for name in PER_SAMPLE + PER_SAMPLE_D:
            assert (sol[name][k, n:] == PRE).all(), (name, k)
        if b < 0:
            for name in PER_PATH:
                assert (sol[name][k] == (PRE if name == "max_time_increment" else PRE_INT)), (name, k)
            continue
        alone, alone_rec = solved_alone(env, key, batch, D, b, n, ref["delta"][k])
        for name in PER_SAMPLE + PER_SAMPLE_D:
            assert same(sol[name][k, :n], alone[name][0]), (name, k, b)
        for name in PER_PATH:
            assert same(sol[name][k], alone[name][0]), (name, k, b)
        assert cr.same_record(cr.record_of(alone_rec, 0), want_rec), (k, b)
        if oracle:
            f = ref["final"][k]
            assert sol["status"][k] == f["status"], (k, b)
            if f["status"] == 0:
                assert same(sol["sd2"][k, :n], f["sd2"]) and same(sol["sdd"][k, :n], f["sdd"]), (k, b)


@pytest.fixture(scope="module")
def main_runs(env):
    return {}


def main_run(env, main_runs, D):
    if D not in main_runs:
        main_runs[D] = run_refined(env, cases.joint_batch(D), D)
    return main_runs[D]


@pytest.mark.parametrize("D", cases.DOFS)
def test_device_entry_equals_plain_calls_and_the_reference(env, main_runs, D):
    batch, ref = cases.joint_batch(D), cases.joint_reference(D)
    out, got = main_run(env, main_runs, D)
    plain, plain_rec = run_plain(env, batch, D)
    for name in PER_SAMPLE + PER_SAMPLE_D + PER_PATH:
        assert same(out[name], plain[name]), name
    for name in cr.KEYS:
        assert same(got["check"][name], plain_rec[name]), name
    for b in range(B):
        assert cr.same_record(cr.record_of(got["check"], b), ref["round0"][b]["record"]), b
    assert_slots(env, ("main", D), batch, D, got, ref, cases.MAX_SAMPLES, B)


def test_more_violators_than_slots(env, main_runs):
    D, M = 7, 4
    batch, ref = cases.joint_batch(D), cases.joint_reference(D, max_refined=4)
    out, got = run_refined(env, batch, D, M=M)
    assert list(got["slot_path"]) == [0, 2, 3, 4]
    violators = [b for b in range(B) if rr.needs_refinement(ref["round0"][b]["record"], 0.0)]
    assert [b for b in range(B) if got["slot"][b] == rr.NO_SLOT] == violators[4:]
    assert_slots(env, ("main", D), batch, D, got, ref, cases.MAX_SAMPLES, M)
    full = main_run(env, main_runs, D)[1]
    for k in range(M):
        n = int(got["num_samples"][k])
        for name in PER_SAMPLE + PER_SAMPLE_D:
            assert same(got["refined"][name][k, :n], full["refined"][name][k, :n]), (name, k)


def test_max_samples_limits(env):
    D = 7
    batch = cases.joint_batch(D)
    two_round = cases.summary(cases.joint_reference(D))[1]
    ref65 = cases.joint_reference(D, max_samples=65)
    out, got65 = run_refined(env, batch, D, max_samples=65)
    assert_slots(env, ("main", D), batch, D, got65, ref65, 65, B)
    for b in two_round:
        k = int(got65["slot"][b])
        assert got65["rounds"][k] == 1 and got65["num_samples"][k] == 65 and got65["refined_check"]["violations"][k] > 0
    ref64 = cases.joint_reference(D, max_samples=64)
    out, got64 = run_refined(env, batch, D, max_samples=64)
    assert_slots(env, ("main", D), batch, D, got64, ref64, 64, B)
    assert got64["num_refined"][0] == 0
    violators = [b for b in range(B) if rr.needs_refinement(ref64["round0"][b]["record"], 0.0)]
    assert violators and all(got64["slot"][b] == rr.TOO_LONG for b in violators)
    # one round into arrays of 129 samples: what max_samples 65 gave
    out, got1 = run_refined(env, batch, D, max_rounds=1)
    assert_slots(env, ("main", D), batch, D, got1, cases.joint_reference(D, max_rounds=1), cases.MAX_SAMPLES, B)
    for name in ("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta"):
        assert same(got1[name], got65[name]), name
    for name in cr.KEYS:
        assert same(got1["refined_check"][name], got65["refined_check"][name]), name
    for name in PER_SAMPLE + PER_SAMPLE_D:
        assert same(got1["refined"][name][:, :65], got65["refined"][name]), name


def test_slot_map_across_waves_and_chunks(env):
    """600 paths (three chunks of k_refine_select, every wave of a chunk with violators): the shared 16
    paths at D = 3, path b = path b % 16, so the round-0 records are the oracle's. With max_samples 64
    every violator is too long (-3); with 129 and 100 slots the first 100 violators in path order,
    which lie in all three chunks, get the slots and the others -2. The slot map is slot_map's, and a slot holds what the slot of the
    same path holds in the 16-path run."""
    D, big, M = 3, 600, 100
    small, ref = cases.joint_batch(D), cases.joint_reference(D)
    pick = np.arange(big) % B
    batch = {k: (np.ascontiguousarray(v[pick]) if isinstance(v, np.ndarray) and v.shape[:1] == (B,) else v)
             for k, v in small.items()}
    records = [ref["round0"][b]["record"] for b in pick]
    counts = np.full(big, N)
    for max_samples in (64, cases.MAX_SAMPLES):
        out, got = run_refined(env, batch, D, max_samples=max_samples, M=M)
        slot, slot_path, used = rr.slot_map(records, counts, max_samples, M, 0.0)
        assert same(got["slot"], slot) and same(got["slot_path"], slot_path) and got["num_refined"][0] == used
        for b in range(big):
            assert cr.same_record(cr.record_of(got["check"], b), records[b]), b
    violators = sum(rr.needs_refinement(r, 0.0) for r in records)
    assert used == M and (slot == rr.NO_SLOT).sum() == violators - M > 0
    assert all((slot[lo:lo + 256] >= 0).any() for lo in (0, 256, 512))
    first = {int(b): k for k, b in enumerate(ref["slot_path"]) if b >= 0}
    for k in range(M):
        k16 = first[int(slot_path[k]) % B]
        n = int(ref["num_samples"][k16])
        assert got["rounds"][k] == ref["rounds"][k16] and got["num_samples"][k] == n
        assert cr.same_record(cr.record_of(got["refined_check"], k), ref["refined_check"][k16]), k
        f = ref["final"][k16]
        assert same(got["refined"]["sd2"][k, :n], f["sd2"]) and same(got["refined"]["sdd"][k, :n], f["sdd"]), k


def test_tolerance(env):
    D = 7
    batch, ref = cases.joint_batch(D), cases.joint_reference(D)
    excess = sorted(r["record"][1] for r in ref["round0"] if r["record"][0] > 0)
    assert len(excess) >= 2 and excess[0] < excess[-1]
    out, got = run_refined(env, batch, D, tolerance=excess[-1] + 1.0)
    assert (got["slot"] == rr.NOTHING).all() and got["num_refined"][0] == 0 and (got["slot_path"] == -1).all()
    for name in PER_SAMPLE + PER_SAMPLE_D + PER_PATH:
        v = got["refined"][name]
        assert (v == (PRE if v.dtype.kind == "f" else PRE_INT)).all(), name
    mid = len(excess) // 2
    tol = 0.5 * (excess[mid - 1] + excess[mid])
    assert excess[mid - 1] < tol < excess[mid]
    ref_mid = cases.joint_reference(D, tolerance=tol)
    assert 0 < ref_mid["num_refined"] < ref["num_refined"]
    out, got = run_refined(env, batch, D, tolerance=tol)
    assert_slots(env, ("main", D), batch, D, got, ref_mid, cases.MAX_SAMPLES, B)


def test_ragged_batch_with_a_failed_path(env):
    D, stride = 7, 50
    batch, counts, ref = cases.ragged_batch(D, stride)
    assert ref["num_refined"] >= 2
    out, got = run_refined(env, batch, D, stride=stride, counts=counts)
    plain, plain_rec = run_plain(env, batch, D, stride=stride, counts=counts)
    for name in PER_SAMPLE + PER_SAMPLE_D + PER_PATH:
        assert same(out[name], plain[name]), name
    for name in cr.KEYS:
        assert same(got["check"][name], plain_rec[name]), name
    assert out["status"][B - 1] == 4 and got["check"]["violations"][B - 1] == -1 and got["slot"][B - 1] == rr.NOTHING
    assert_slots(env, ("ragged", D), batch, D, got, ref, cases.MAX_SAMPLES, B)


@pytest.mark.parametrize("D", [7, 16])
def test_host_entry_equals_the_device_entry(env, main_runs, D):
    batch = cases.joint_batch(D)
    out_d, got_d = main_run(env, main_runs, D)
    out_h, got_h = run_refined(env, batch, D, host=True)
    for name in PER_SAMPLE + PER_SAMPLE_D + PER_PATH:
        assert same(out_h[name], out_d[name]), name
        assert same(got_h["refined"][name], got_d["refined"][name]), name
    for name in ("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta"):
        assert same(got_h[name], got_d[name]), name
    for name in cr.KEYS:
        assert same(got_h["check"][name], got_d["check"][name]), name
        assert same(got_h["refined_check"][name], got_d["refined_check"][name]), name


def test_query_device_answers_as_after_the_plain_call(env):
    D = 7
    torch, E = env["torch"], env["E"]
    batch = cases.joint_batch(D)
    inp = engine_inputs(batch, False, env)
    K = 5
    answers = []
    for refined in (False, True):
        out = solution_arrays(B, N, D, False, env)
        out.pop("sd2")                               # the query has to use the engine's copy
        if refined:
            E.time_joint_paths_refined(inp, out, N, cases.MAX_ROUNDS, cases.MAX_SAMPLES, B, safety=batch["safety"])
        else:
            E.time_joint_paths(inp, out, N, safety=batch["safety"])
        torch.cuda.synchronize()
        end = out["time"][:, -1:].clone()
        tq = (end * torch.linspace(0.05, 0.95, K, dtype=torch.float64, device=env["dev"])[None, :]).contiguous()
        res = [torch.full((B, K), PRE, dtype=torch.float64, device=env["dev"]) for _ in range(3)]
        ok = torch.full((B, K), PRE_INT, dtype=torch.int32, device=env["dev"])
        E.query(out["time"], out["s"], out["sd"], out["status"], tq, res[0], res[1], res[2], ok=ok)
        torch.cuda.synchronize()
        answers.append([to_numpy(x) for x in res + [ok, tq]])
    for a, b in zip(*answers):
        assert same(a, b)
    assert (answers[0][3] != PRE_INT).all()


def test_call_level_errors_write_nothing(env):
    D = 7
    eng, E = env["eng"], env["E"]
    batch = cases.joint_batch(D)
    for host in (False, True):
        inp = engine_inputs(batch, host, env)
        out = solution_arrays(B, N, D, host, env)
        ref = refine_arrays(B, B, cases.MAX_SAMPLES, D, host, env)
        call = lambda **kw: E.time_joint_paths_refined(
            inp, out, N, kw.get("max_rounds", 2), kw.get("max_samples", cases.MAX_SAMPLES), B,
            safety=batch["safety"], refined=kw.get("refined", ref), host=host)
        with pytest.raises(eng.TpamdError, match="-3"):
            call(max_samples=N - 1)
        with pytest.raises(eng.TpamdError, match="-3"):
            call(max_rounds=0)
        with pytest.raises(eng.TpamdError, match="-1"):
            call(refined=dict(ref, slot_path=None))
        # a NULL ref, straight through the C-ABI
        cp = inp["control_points"]
        bt = eng._JointBatch(B, D, N, cp.shape[1], 0, 0, batch["safety"])
        ji, po = eng._JointInputs.from_dict(inp), eng._PathOutputs.from_dict(out)
        opt = eng._RefineOptions(2, cases.MAX_SAMPLES, B, 0, 0.0)
        lib = eng.load_library()
        if host:
            rc = lib.tpamd_time_joint_paths_refined_host(E._h, C.byref(bt), C.byref(ji), C.byref(po), C.byref(opt), None)
        else:
            rc = lib.tpamd_time_joint_paths_refined_device(E._h, C.byref(bt), C.byref(ji), C.byref(po), C.byref(opt),
                                                           None, None)
        assert rc == -1
        # 17 joints
        wide = dict(batch)
        for k, width in (("control_points", None), ("vmax", 17), ("amax", 17)):
            wide[k] = np.ones((B, batch["control_points"].shape[1], 17)) if width is None else np.ones((B, 17))
        with pytest.raises(eng.TpamdError, match="-3"):
            E.time_joint_paths_refined(engine_inputs(wide, host, env), out, N, 2, cases.MAX_SAMPLES, B,
                                       safety=batch["safety"], refined=ref, host=host)
        if not host:
            env["torch"].cuda.synchronize()
        for tree in (to_numpy(out), to_numpy(ref)):
            for k, v in tree.items():
                for name, a in (v.items() if isinstance(v, dict) else [(k, v)]):
                    assert (a == (PRE if a.dtype.kind == "f" else PRE_INT)).all(), (host, k, name)

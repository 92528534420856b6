"""Ragged Cartesian and rows batches on the GPU (tpamd_time_cartesian_paths_ragged_*,
tpamd_optimize_rows_ragged_*, Engine.time_cartesian_paths / optimize_rows with
num_samples_per_path / first_row).

Every comparison is bit equality. The reference of path b is the CPU oracle run on that path
ALONE with N = n[b] (for the rows form: the uniform engine call on that path alone). The paths are
the seven families of tests/cartesian_paths.py at the counts {3, 4, 64, 255, 256, 257, 513, 600}
in arrays of stride 600: the minimum, the last thread of a block, a block that holds one sample,
a path that fills the stride. D = 6 and 7 take the fused K1, D = 5 the generic route. Input rows
beyond a path's count are NaN (strided) or another path's rows (packed), so an end condition
taken from the stride instead of the count shows as a differing bit."""
import importlib
import os

import numpy as np
import pytest

import cartesian_paths as cp
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

N = 600
COUNTS = (3, 4, 64, 255, 256, 257, 513, 600)
PER_SAMPLE = ("time", "s", "sd", "sdd")
PER_JOINT = ("q", "qd", "qdd")
PER_PATH = ("status", "last_extremal_index")
PRE = -7.25                      # prefill of the double outputs
PRE_INT = -9                     # prefill of the int32 outputs
ARRAYS = ("ik_positions", "jacobians", "vmax", "amax", "vtrans", "vrot", "path_start", "delta",
          "sd_start", "time_start")
NAMES = dict(vmax="max_velocity", amax="max_acceleration", vtrans="max_translational_velocity",
             vrot="max_rotational_velocity", path_start="path_start", delta="delta",
             sd_start="sd_start", time_start="time_start")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    from oracle import tpo
    return dict(torch=torch, eng=eng, syn=syn, tpo=tpo, E=eng.Engine(0), dev="cuda:0")


@pytest.fixture(scope="module")
def generic_engine(env):
    """An engine created with TPAMD_FORCE_GENERIC=1: D = 6 / 7 take the rows route."""
    os.environ["TPAMD_FORCE_GENERIC"] = "1"
    try:
        E = env["eng"].Engine(0)
    finally:
        del os.environ["TPAMD_FORCE_GENERIC"]
    return E


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same(a, b, what):
    assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), what


def _make_case(tpo, D):
    """56 paths: every family at every count. Per path the oracle's result on that path alone;
    the strided arrays [B][N] with NaN behind every path; the packed tables with the paths' rows
    shuffled and two rows of NaN at the end."""
    paths, counts, refs = [], [], []
    for fi, name in enumerate(cp.FAMILIES):
        for ci, n in enumerate(COUNTS):
            b = cp.make_family(name, 3, D, n)
            if name in cp.CURVED:
                b = cp.with_starts(b)
            j = (fi + ci) % 3           # with_starts: 0 plain, 1 start velocity, 2 start parameter
            one = {k: np.ascontiguousarray(b[k][j:j + 1]) for k in ARRAYS}
            one["safety"] = b["safety"]
            ref = cp.oracle_solve(tpo, one, 1)
            assert ref["status"][0] == 0, (name, n)
            paths.append(one)
            counts.append(n)
            refs.append(ref)
    B = len(paths)
    assert B <= 64 and len({p["safety"] for p in paths}) == 1
    ik = np.full((B, N, D), np.nan)
    jac = np.full((B, N, 6, D), np.nan)
    for b, (p, n) in enumerate(zip(paths, counts)):
        ik[b, :n] = p["ik_positions"][0]
        jac[b, :n] = p["jacobians"][0]
    per_path = {k: np.ascontiguousarray(np.concatenate([p[k] for p in paths]))
                for k in ARRAYS if k not in ("ik_positions", "jacobians")}
    order = np.random.default_rng(1234 + D).permutation(B)
    rows = sum(counts) + 2
    tq, tj = np.full((rows, D), np.nan), np.full((rows, 6, D), np.nan)
    first = np.zeros(B, np.int32)
    r = 0
    for b in order:
        first[b] = r
        tq[r:r + counts[b]] = paths[b]["ik_positions"][0]
        tj[r:r + counts[b]] = paths[b]["jacobians"][0]
        r += counts[b]
    return dict(D=D, B=B, counts=np.array(counts, np.int32), refs=refs, ik=ik, jac=jac, per_path=per_path,
                first=first, tq=tq, tj=tj, safety=paths[0]["safety"])


@pytest.fixture(scope="module")
def cases(env):
    return {D: _make_case(env["tpo"], D) for D in (5, 6, 7)}


def _prefilled(B, D, xp_full):
    out = {k: xp_full((B, N), PRE) for k in PER_SAMPLE}
    out.update({k: xp_full((B, N, D), PRE) for k in PER_JOINT})
    out["max_time_increment"] = xp_full((B,), PRE)
    out["status"] = xp_full((B,), PRE_INT, True)
    out["last_extremal_index"] = xp_full((B,), PRE_INT, True)
    return out


def _solve(env, case, E=None, packed=False, host=False, counts=None, ragged=True):
    """One call through Engine.time_cartesian_paths; outputs as numpy arrays, prefilled first."""
    torch = env["torch"]
    B, D = case["B"], case["D"]
    counts = case["counts"] if counts is None else np.asarray(counts, np.int32)
    inp = dict(ik_positions=case["tq"] if packed else case["ik"], jacobians=case["tj"] if packed else case["jac"])
    inp.update({NAMES[k]: v for k, v in case["per_path"].items()})
    if host:
        full = lambda shape, v, integer=False: np.full(shape, v, np.int32 if integer else np.float64)
        ns, fr = counts, case["first"]
    else:
        dev = env["dev"]
        inp = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in inp.items()}
        full = lambda shape, v, integer=False: torch.full(shape, v, dtype=torch.int32 if integer else torch.float64,
                                                          device=dev)
        ns, fr = torch.from_numpy(counts).to(dev), torch.from_numpy(case["first"]).to(dev)
    out = _prefilled(B, D, full)
    kw = dict(num_samples_per_path=ns, first_row=fr if packed else None) if ragged else {}
    (E or env["E"]).time_cartesian_paths(inp, out, safety=case["safety"], host=host, **kw)
    if host:
        return out
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _check_against_oracle(case, got, what, skip=()):
    """[0, n[b]) equals the oracle on the path alone; [n[b], N) keeps the prefill."""
    for b, (n, ref) in enumerate(zip(case["counts"], case["refs"])):
        if b in skip:
            continue
        w = "%s: path %d (n %d)" % (what, b, n)
        assert got["status"][b] == 0, w
        assert got["last_extremal_index"][b] == ref["last_extremal_index"][0], w
        for k in PER_SAMPLE + PER_JOINT:
            _same(got[k][b, :n], ref["t" if k == "time" else k][0], w + " " + k)
            assert (got[k][b, n:] == PRE).all(), w + " " + k + " behind the path's end"


def _same_outputs(a, b, what):
    for k in PER_SAMPLE + PER_JOINT + PER_PATH + ("max_time_increment",):
        _same(a[k], b[k], what + ": " + k)


@pytest.fixture(scope="module")
def strided(env, cases):
    """The strided ragged result of every joint count (test 1 checks it; the others compare with it)."""
    return {D: _solve(env, cases[D]) for D in cases}


# ------------------------------------------------------------------ 1. strided
@pytest.mark.parametrize("D", [5, 6, 7])
def test_strided_ragged_equals_the_oracle_per_path(env, cases, strided, generic_engine, D):
    _check_against_oracle(cases[D], strided[D], "strided D %d" % D)
    if D == 6:
        gen = _solve(env, cases[D], generic_engine)
        _same_outputs(gen, strided[D], "generic route D 6")


# ------------------------------------------------------------------- 2. packed
@pytest.mark.parametrize("D", [5, 6, 7])
def test_packed_rows_equal_the_strided_call(env, cases, strided, generic_engine, D):
    """The paths' rows shuffled in one table, a neighbour's rows directly behind each path."""
    case = cases[D]
    got = _solve(env, case, packed=True)
    _same_outputs(got, strided[D], "packed D %d" % D)
    for b, n in enumerate(case["counts"]):
        _same(got["q"][b, :n], case["tq"][case["first"][b]:case["first"][b] + n], "gathered q, path %d" % b)
    if D == 7:
        _same_outputs(_solve(env, case, generic_engine, packed=True), strided[D], "packed, generic route D 7")


# ------------------------------------------------------- 3. all counts equal N
@pytest.mark.parametrize("D", [5, 6, 7])
def test_all_counts_equal_to_the_stride_equal_the_uniform_entry(env, generic_engine, D):
    parts = []
    for name in cp.FAMILIES:
        b = cp.make_family(name, 2, D, N)
        parts.append(cp.with_starts(b) if name in cp.CURVED else b)
    u = cp.concat(parts)
    B = u["ik_positions"].shape[0]
    case = dict(D=D, B=B, counts=np.full(B, N, np.int32), ik=u["ik_positions"], jac=u["jacobians"],
                tq=u["ik_positions"].reshape(B * N, D), tj=u["jacobians"].reshape(B * N, 6, D),
                first=(np.arange(B) * N).astype(np.int32), safety=u["safety"],
                per_path={k: u[k] for k in ARRAYS if k not in ("ik_positions", "jacobians")})
    for E, route in ((None, "fused" if D in (6, 7) else "generic"),) + (((generic_engine, "forced generic"),) if D in (6, 7) else ()):
        uniform = _solve(env, case, E, ragged=False)
        assert (uniform["status"] == 0).all()
        _same_outputs(_solve(env, case, E), uniform, "strided, all N, %s D %d" % (route, D))
        _same_outputs(_solve(env, case, E, packed=True), uniform, "packed, all N, %s D %d" % (route, D))


# ------------------------------------------------------------ 4. host = device
@pytest.mark.parametrize("D", [5, 6])
def test_host_entry_equals_device_entry(env, cases, strided, D):
    _same_outputs(_solve(env, cases[D], host=True), strided[D], "host strided D %d" % D)
    _same_outputs(_solve(env, cases[D], host=True, packed=True), strided[D], "host packed D %d" % D)


# ---------------------------------------------------------------- 5. bad counts
def _joint_status_of_counts(env, D, counts):
    """What tpamd_time_joint_paths_device reports for these counts (stride N)."""
    torch, eng, syn = env["torch"], env["eng"], env["syn"]
    B = len(counts)
    jb = syn.make_joint_batch(B, D, N)
    inp = eng.upload_joint_batch(jb, env["dev"])
    inp["num_samples_per_path"] = torch.from_numpy(np.asarray(counts, np.int32)).to(env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    env["E"].time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    return out["status"].cpu().numpy()


@pytest.mark.parametrize("packed", [False, True], ids=["strided", "packed"])
@pytest.mark.parametrize("D", [5, 6])
def test_bad_counts_fail_their_path_alone(env, cases, D, packed):
    """Counts 1, 0 and N + 1 among good paths, through the C entry with guard regions around every
    output array."""
    import ctypes as C
    torch, eng, case, dev = env["torch"], env["eng"], cases[D], env["dev"]
    B = case["B"]
    bad = {5: 1, 20: 0, 41: N + 1}
    counts = case["counts"].copy()
    for b, n in bad.items():
        counts[b] = n
    want = _joint_status_of_counts(env, D, counts)
    assert want[5] != 0 and want[20] != 0 and want[41] == 6 and (np.delete(want, list(bad)) == 0).all()
    G = 512                                                    # guard elements on either side
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    inp = dict(ik_positions=t(case["tq"] if packed else case["ik"]), jacobians=t(case["tj"] if packed else case["jac"]))
    inp.update({NAMES[k]: t(v) for k, v in case["per_path"].items()})
    shapes = {k: (B, N) for k in PER_SAMPLE}
    shapes.update({k: (B, N, D) for k in PER_JOINT})
    shapes.update(max_time_increment=(B,), status=(B,), last_extremal_index=(B,))
    flat, out = {}, {}
    for k, shape in shapes.items():
        integer = k in PER_PATH
        size = int(np.prod(shape))
        flat[k] = torch.full((size + 2 * G,), PRE_INT if integer else PRE,
                             dtype=torch.int32 if integer else torch.float64, device=dev)
        out[k] = flat[k][G:G + size].view(*shape)
    ns, fr = t(counts), t(case["first"])
    bt = eng._CartesianBatch(B, D, N, 0, float(case["safety"]))
    ci, po = eng._CartesianInputs.from_dict(inp), eng._PathOutputs.from_dict(out)
    E = env["E"]
    rc = E._lib.tpamd_time_cartesian_paths_ragged_device(
        E._h, C.byref(bt), C.byref(ci), eng._ptr(ns), eng._ptr(fr) if packed else None, C.byref(po),
        C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k, f in flat.items():
        f = f.cpu().numpy()
        pre = PRE_INT if k in PER_PATH else PRE
        assert (f[:G] == pre).all() and (f[-G:] == pre).all(), "guard of " + k
    _check_against_oracle(case, got, "bad counts D %d" % D, skip=bad)
    for b in bad:
        assert got["status"][b] == want[b], (b, got["status"][b], want[b])
        for k in PER_SAMPLE + PER_JOINT:
            assert (got[k][b] == PRE).all(), (b, k)
    # a NULL count array is a call-level error, as for the uniform entry's NULL arrays
    assert E._lib.tpamd_time_cartesian_paths_ragged_device(
        E._h, C.byref(bt), C.byref(ci), None, None, C.byref(po),
        C.c_void_p(torch.cuda.current_stream().cuda_stream)) == -1


# ----------------------------------------------------------------- 6. rows form
@pytest.mark.parametrize("D", [1, 17], ids=["C2_one_word", "C34_two_words"])
def test_rows_form_ragged_equals_the_uniform_call_per_path(env, D):
    """optimize_rows with per-path counts at C = 2 and C = 34 (both k_lp_rows word counts): joint
    rows of D = 1 and D = 17 paths; row entries behind a path's end are NaN."""
    torch, tpo, syn, E, dev = env["torch"], env["tpo"], env["syn"], env["E"], env["dev"]
    counts = np.array([3, 64, 65, 257, 600, 4], np.int32)
    B, Cn = len(counts), 2 * D
    rows = {k: np.full((B, N, Cn), np.nan) for k in ("a", "b", "lower", "upper")}
    s_end, per = np.zeros(B), []
    for b, n in enumerate(counts):
        jb = syn.make_joint_batch(1, D, int(n), first_path_index=40 + b)
        _, q1, q2 = tpo.joint_sample_path(jb["knots"][0], jb["control_points"][0], 0.0, jb["delta"][0], int(n))
        A, Bm, lo, hi = tpo.joint_constraint_setup(q1, q2, jb["vmax"][0], jb["amax"][0], 0.8)
        for k, v in zip(("a", "b", "lower", "upper"), (A, Bm, lo, hi)):
            rows[k][b, :n] = v
        s_end[b] = jb["delta"][0] * (n - 1)
        per.append((A, Bm, lo, hi))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    scal = dict(s_start=np.zeros(B), s_end=s_end, sd_start=np.zeros(B), time_start=np.linspace(0.0, 2.5, B))

    def outputs(Bn, n):
        o = {k: torch.full((Bn, n), PRE, dtype=torch.float64, device=dev) for k in PER_SAMPLE}
        o["status"] = torch.full((Bn,), PRE_INT, dtype=torch.int32, device=dev)
        o["last_extremal_index"] = torch.full((Bn,), PRE_INT, dtype=torch.int32, device=dev)
        o["max_time_increment"] = torch.full((Bn,), PRE, dtype=torch.float64, device=dev)
        return o

    inp = {k: t(v) for k, v in rows.items()}
    inp.update({k: t(v) for k, v in scal.items()})
    out = outputs(B, N)
    E.optimize_rows(inp, out, num_samples_per_path=t(counts))
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in out.items()}
    host_out = {k: v.copy() for k, v in {**{k: np.full((B, N), PRE) for k in PER_SAMPLE},
                                          "status": np.full(B, PRE_INT, np.int32),
                                          "last_extremal_index": np.full(B, PRE_INT, np.int32),
                                          "max_time_increment": np.full(B, PRE)}.items()}
    E.optimize_rows({**rows, **scal}, host_out, num_samples_per_path=counts, host=True)
    for b, n in enumerate(counts):
        one = {k: t(v[None]) for k, v in zip(("a", "b", "lower", "upper"), per[b])}
        one.update({k: t(v[b:b + 1]) for k, v in scal.items()})
        ref = outputs(1, int(n))
        E.optimize_rows(one, ref)
        torch.cuda.synchronize()
        ref = {k: v.cpu().numpy() for k, v in ref.items()}
        assert ref["status"][0] == 0, b
        for g, route in ((got, "device"), (host_out, "host")):
            w = "rows C %d, %s, path %d (n %d)" % (Cn, route, b, n)
            for k in PER_PATH + ("max_time_increment",):
                assert g[k][b] == ref[k][0], w + " " + k
            for k in PER_SAMPLE:
                _same(g[k][b, :n], ref[k][0], w + " " + k)
                assert (g[k][b, n:] == PRE).all(), w + " " + k + " behind the path's end"

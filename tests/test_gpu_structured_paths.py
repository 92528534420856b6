"""The engine on structured and degenerate path geometry (tests/structured_paths.py): bit-parity
with the CPU oracle and the independent property checker (tests/hp_reference.py) for every
family at every specialised and generic joint count, mixed structured/random batches through the
pipelined engine and time_joint_groups, ragged sample counts, Cartesian paths, and the
downstream entries (query, resample, fastest stop) on profiles whose time has plateaus."""
import importlib

import numpy as np
import pytest

import hp_reference as hp
import structured_paths as sp
from conftest import PKG_NAME
from test_fastest_stop_cpu import fastest_stop_at_time
from test_structured_paths_cpu import ACCEL_STRICT

pytestmark = pytest.mark.gpu

KEYS = ("time", "s", "sd", "sdd", "q", "qd", "qdd")


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    from oracle import tpo
    return dict(torch=torch, eng=eng, syn=syn, tpo=tpo, E=eng.Engine(0), dev="cuda:0")


def _solve(env, E, b, N):
    eng, torch = env["eng"], env["torch"]
    B, _, D = b["control_points"].shape
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    return inp, out


def _assert_bit_parity(out, ref, what):
    st = out["status"].cpu().numpy()
    np.testing.assert_array_equal(st, ref["status"], err_msg=what)
    ok = st == 0
    np.testing.assert_array_equal(out["last_extremal_index"].cpu().numpy()[ok],
                                  ref["last_extremal_index"][ok], err_msg=what)
    for k in KEYS:
        g = out[k].cpu().numpy()
        r = ref["t" if k == "time" else k]
        np.testing.assert_array_equal(g[ok], r[ok], err_msg="%s %s" % (what, k))
    return ok


def _shapes():
    """(D, N) pairs: every specialised and generic D, the sample counts in turn, and N = 2000
    at D = 7 and 16 as well."""
    out = []
    for k, D in enumerate(sp.SPECIALISED_DOFS + sp.GENERIC_DOFS):
        out.append((D, sp.SAMPLE_COUNTS[k % len(sp.SAMPLE_COUNTS)]))
        if D in (7, 16):
            out.append((D, 2000))
    return out


def _family_batch(name, D, N):
    rest = sp.make_family(name, 4, D, N)
    starts = sp.with_starts(sp.make_family(name, 4, D, N, seed=1), seed=D)
    return sp.concat([rest, starts])


@pytest.mark.parametrize("D,N,seed", [(7, 65, None), (7, 2000, None), (7, 500, 3), (6, 333, 3)])
def test_chain_blocks_stop_where_the_speculated_row_vanishes(env, D, N, seed):
    """A repeated interior waypoint leaves a stretch where every q' is below kTiny. FindSdd skips
    such rows, so an extremal enters the stretch with sdd = 0. The speculative chain of the
    specialised sweeps used to keep the previous row's candidate there (a quotient by a q' near
    1e-17), push sd2 onto the 1e6 cap and leave the oracle's sdd; these are the paths where it
    did (D = 7 and 6)."""
    if seed is None:
        b = _family_batch("stop_interior", D, N)
    else:
        b = sp.make_family("stop_interior", 12, D, N, seed=seed)
    ref = sp.oracle_solve(env["tpo"], b, N)
    _, out = _solve(env, env["E"], b, N)
    assert _assert_bit_parity(out, ref, "stop_interior D=%d N=%d" % (D, N)).all()
    hp.check_profile(b, out, stationary_ok=True, accel_allowance=None)


@pytest.mark.parametrize("name", sp.FAMILIES)
def test_joint_mode_family_matches_the_oracle_and_the_properties(env, name):
    tpo, E = env["tpo"], env["E"]
    stop = name in sp.STOP_FAMILIES
    for D, N in _shapes():
        b = _family_batch(name, D, N)
        ref = sp.oracle_solve(tpo, b, N)
        _, out = _solve(env, E, b, N)
        what = "%s D=%d N=%d" % (name, D, N)
        ok = _assert_bit_parity(out, ref, what)
        assert ok.all(), what
        strict = N == 2000 and name in ACCEL_STRICT
        hp.check_profile(b, out, stationary_ok=stop, paths=range(4),
                         accel_allowance=0 if strict else None)
        hp.check_profile(b, out, stationary_ok=stop, paths=range(4, 8), accel_allowance=None)


def _mixed_batch(D, N, random_paths):
    fams = [f for f in sp.FAMILIES if not f.startswith("straight")]
    parts = [sp.make_family(f, 12, D, N, seed=3) for f in fams]
    parts.append(sp.syn.make_joint_batch(random_paths, D, N, num_waypoints=sp.WAYPOINTS,
                                         first_path_index=900_000 + D))
    b = sp.concat(parts)
    perm = np.random.default_rng(D).permutation(b["control_points"].shape[0])
    return {k: (np.ascontiguousarray(v[perm]) if isinstance(v, np.ndarray) else v)
            for k, v in b.items()}


def test_mixed_batches_through_the_pipelined_engine_and_joint_groups(env):
    """At least 256 paths, structured and random interleaved, on an engine with pipelining on
    (two solves in a row, the second overlapping the first), and as two groups of one
    time_joint_groups call."""
    torch, eng, tpo = env["torch"], env["eng"], env["tpo"]
    E2 = eng.Engine(0)
    E2.set_pipelining(1)
    b7 = _mixed_batch(7, 500, 100)
    b6 = _mixed_batch(6, 333, 60)
    assert b7["control_points"].shape[0] >= 256
    r7 = sp.oracle_solve(tpo, b7, 500, nthreads=16)
    r6 = sp.oracle_solve(tpo, b6, 333, nthreads=16)
    B7, B6 = b7["control_points"].shape[0], b6["control_points"].shape[0]
    i7, o7 = eng.upload_joint_batch(b7, env["dev"]), eng.alloc_joint_outputs(B7, 500, 7, env["dev"])
    i6, o6 = eng.upload_joint_batch(b6, env["dev"]), eng.alloc_joint_outputs(B6, 333, 6, env["dev"])
    E2.time_joint_paths(i7, o7, 500)
    E2.time_joint_paths(i6, o6, 333)
    E2.fence()
    torch.cuda.synchronize()
    _assert_bit_parity(o7, r7, "pipelined D=7")
    _assert_bit_parity(o6, r6, "pipelined D=6")
    g7, g6 = eng.alloc_joint_outputs(B7, 500, 7, env["dev"]), eng.alloc_joint_outputs(B6, 333, 6, env["dev"])
    env["E"].time_joint_groups([dict(inputs=i7, outputs=g7, num_samples=500),
                                dict(inputs=i6, outputs=g6, num_samples=333)])
    torch.cuda.synchronize()
    _assert_bit_parity(g7, r7, "groups D=7")
    _assert_bit_parity(g6, r6, "groups D=6")
    E2.close()


def test_ragged_sample_counts_on_the_stop_family(env):
    torch, eng, tpo, E = env["torch"], env["eng"], env["tpo"], env["E"]
    D, stride = 7, 600
    counts = np.array([600, 3, 17, 63, 64, 65, 599, 300, 128, 451, 5, 77], dtype=np.int32)
    B = len(counts)
    b = sp.concat([sp.make_family(f, 4, D, stride, seed=5) for f in sp.STOP_FAMILIES])
    b["delta"] = np.ascontiguousarray(b["knots"][:, -1] / (counts - 1))
    inp = eng.upload_joint_batch(b, env["dev"])
    inp["num_samples_per_path"] = torch.from_numpy(counts).to(env["dev"])
    out = eng.alloc_joint_outputs(B, stride, D, env["dev"])
    for k in KEYS:
        out[k].fill_(-7.0)
    E.time_joint_paths(inp, out, stride)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in KEYS}
    st = out["status"].cpu().numpy()
    for i, n in enumerate(counts):
        one = {k: b[k][i:i + 1] for k in ("knots", "control_points", "vmax", "amax", "path_start",
                                          "delta", "sd_start", "time_start")}
        one["safety"] = 0.8
        ref = sp.oracle_solve(tpo, one, int(n), nthreads=1)
        assert st[i] == ref["status"][0] == 0, (i, n)
        assert out["last_extremal_index"][i].item() == ref["last_extremal_index"][0]
        for k in KEYS:
            np.testing.assert_array_equal(got[k][i, :n], ref["t" if k == "time" else k][0],
                                          err_msg="%s path %d n %d" % (k, i, n))
            assert (got[k][i, n:] == -7.0).all(), "wrote past n[b]"
    b["num_samples_per_path"] = counts
    hp.check_profile(b, out, stationary_ok=True, accel_allowance=None)


def _cartesian_from_family(syn, b, N, seed):
    """IK tables from a family's splines, built the way make_cartesian_batch builds them."""
    B, _, D = b["control_points"].shape
    u = b["delta"][:, None] * np.arange(N)[None, :]
    q = syn.eval_joint_splines(b["control_points"], b["knots"], u)
    r = np.arange(6)[None, None, :, None]
    d = np.arange(D)[None, None, None, :]
    J = 0.25 * np.sin(q[:, :, None, :] * (r + 1.0) + 0.37 * d) + (r == d % 6)
    lim = np.random.default_rng(seed).uniform(0.0, 1.0, (B, 2))
    return dict(ik_positions=np.ascontiguousarray(q), jacobians=np.ascontiguousarray(J),
                vmax=b["vmax"], amax=b["amax"], vtrans=0.6 + 0.9 * lim[:, 0],
                vrot=0.8 + 1.2 * lim[:, 1], path_start=np.zeros(B), delta=b["delta"],
                sd_start=np.zeros(B), time_start=np.linspace(0.0, 2.0, B), num_samples=N,
                safety=0.8)


@pytest.mark.parametrize("D", [6, 7])
def test_cartesian_mode_on_straight_idle_and_stop_paths(env, D):
    torch, eng, syn, tpo, E = (env[k] for k in ("torch", "eng", "syn", "tpo", "E"))
    for k, name in enumerate(("straight_linear", "straight_long", "idle_one", "idle_most",
                              "stop_interior", "stop_first", "stop_last")):
        N = (64, 500, 2000)[k % 3]
        b = _cartesian_from_family(syn, sp.make_family(name, 6, D, N, seed=2), N, seed=D + k)
        ref = tpo.time_cartesian_batch(b["ik_positions"], b["jacobians"], b["vmax"], b["amax"],
                                       b["vtrans"], b["vrot"], b["path_start"], b["delta"],
                                       time_start=b["time_start"], nthreads=8)
        out = eng.alloc_joint_outputs(6, N, D, env["dev"])
        E.time_cartesian_paths(syn.upload_cartesian_batch(b, env["dev"]), out)
        torch.cuda.synchronize()
        ok = _assert_bit_parity(out, ref, "cartesian %s D=%d N=%d" % (name, D, N))
        assert ok.sum() >= 4, (name, ref["status"])


def test_query_resample_and_fastest_stop_on_time_plateaus(env):
    torch, tpo, E = env["torch"], env["tpo"], env["E"]
    D, N = 7, 800
    b = sp.concat([sp.make_family(f, 3, D, N, seed=7) for f in ("stop_first", "stop_last")])
    B = b["control_points"].shape[0]
    inp, out = _solve(env, E, b, N)
    ref = sp.oracle_solve(tpo, b, N)
    _assert_bit_parity(out, ref, "stop families")
    t = out["time"].cpu().numpy()
    # query times: inside every plateau and exactly at its two ends, plus a spread
    K = 64
    tq = np.zeros((B, K))
    plateau = np.zeros((B, 4))
    for i in range(B):
        flat = np.flatnonzero(np.diff(t[i]) == 0)
        assert flat.size, i
        pts = [t[i, flat[0]], np.nextafter(t[i, flat[0]], np.inf), t[i, flat[-1] + 1],
               t[i, flat[-1] + 2] if flat[-1] + 2 < N else t[i, -1], t[i, 0], t[i, -1]]
        plateau[i] = pts[:4]
        spread = np.linspace(t[i, 0] - 0.1, t[i, -1] + 0.1, K - len(pts))
        tq[i] = np.sort(np.concatenate([pts, spread]))
    dev = env["dev"]
    f = dict(dtype=torch.float64, device=dev)
    qs, qsd, qsdd = (torch.empty(B, K, **f) for _ in range(3))
    okq = torch.zeros(B, K, dtype=torch.int32, device=dev)
    E.query(out["time"], out["s"], out["sd"], out["status"], torch.from_numpy(tq).to(dev),
            qs, qsd, qsdd, okq)
    torch.cuda.synchronize()
    for i in range(B):
        q_, q1, q2 = tpo.joint_sample_path(b["knots"][i], b["control_points"][i], 0.0, b["delta"][i], N)
        p = tpo.Profile(N, 2 * D)
        p.set_max_loops(10 * N)
        assert p.setup(*tpo.joint_constraint_setup(q1, q2, b["vmax"][i], b["amax"][i]), 0.0,
                       b["delta"][i] * (N - 1)) == 0 and p.optimize() == 0
        r = np.array([p.query(x)[1:] for x in tq[i]])
        np.testing.assert_array_equal(qs[i].cpu().numpy(), r[:, 0])
        np.testing.assert_array_equal(qsd[i].cpu().numpy(), r[:, 1])
        np.testing.assert_array_equal(qsdd[i].cpu().numpy(), r[:, 2])
    assert int(okq.min()) == 1

    names = ("out_time", "out_s", "out_sd", "out_sdd", "out_q", "out_qd", "out_qdd")
    sol = [out[k].cpu().numpy() for k in ("s", "sd", "sdd", "q", "qd", "qdd")]
    for skip, dt in ((False, 0.004), (True, 0.004), (True, 1e-6)):
        fn = tpo.resample_skip if skip else tpo.resample_uniform
        refs = [fn(t[i], *[x[i] for x in sol], 0.0, dt, b["amax"][i]) for i in range(B)]
        cap = max(len(r[0]) for r in refs) + 3
        ro = {k: torch.zeros((B, cap, D) if k in ("out_q", "out_qd", "out_qdd") else (B, cap), **f)
              for k in names}
        ro["count"] = torch.zeros(B, dtype=torch.int32, device=dev)
        E.resample_uniform(out, inp["max_acceleration"], torch.zeros(B, **f), dt, ro, skip=skip)
        torch.cuda.synchronize()
        cnt = ro["count"].cpu().numpy()
        for i in range(B):
            M = len(refs[i][0])
            assert cnt[i] == M
            for k, r in zip(names, refs[i]):
                np.testing.assert_array_equal(ro[k][i, :M].cpu().numpy(), r,
                                              err_msg="%s skip=%s dt=%g" % (k, skip, dt))

    # fastest stop, queried inside and at the ends of the plateaus
    am = inp["max_acceleration"]
    th, sh = t, out["s"].cpu().numpy()
    qdh, qddh, amh = out["qd"].cpu().numpy(), out["qdd"].cpu().numpy(), b["amax"]
    for col in range(4):
        qt = np.ascontiguousarray(plateau[:, col])
        got = E.fastest_stop(out["time"], out["s"], out["qd"], out["qdd"], am,
                             torch.from_numpy(qt).to(dev), profile=True)
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in got.items()}
        for i in range(B):
            st, spar, idx, dur, pt, pr, pd = fastest_stop_at_time(
                th[i].tolist(), sh[i].tolist(), qdh[i].tolist(), qddh[i].tolist(), amh[i].tolist(),
                float(qt[i]))
            assert g["status"][i] == st and g["stop_index"][i] == idx, (col, i)
            assert g["stop_parameter"][i].tobytes() == np.float64(spar).tobytes(), (col, i)
            assert g["duration"][i].tobytes() == np.float64(dur).tobytes(), (col, i)
            m = len(pt)
            for key, r in (("profile_time", pt), ("profile_rate2", pr), ("profile_drate2", pd)):
                assert g[key][i, :m].tobytes() == np.asarray(r, dtype=np.float64).tobytes(), (col, i, key)

"""The qd/qdd emission of the joint sweep (JointSweep::emit_range: software-pipelined trips that the
forward wave stops between trips): every output bit for bit against the CPU oracle, at the sample
counts where a trip is short, ends on one sample or splits into two groups of passes, on a long
batch whose many loops stop the emission many times, without qd/qdd, on a Cartesian batch and on ragged paths."""
import importlib

import numpy as np
import pytest

import cartesian_paths as cp
import structured_paths as sp
from conftest import PKG_NAME

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


def _solve(env, E, b, N, **alloc):
    eng, torch = env["eng"], env["torch"]
    B, _, D = b["control_points"].shape
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"], **alloc)
    E.time_joint_paths(inp, out, N)
    E.fence()
    torch.cuda.synchronize()
    return inp, out


def _assert_bit_parity(out, ref, what, keys=KEYS):
    st = out["status"].cpu().numpy()
    np.testing.assert_array_equal(st, ref["status"], err_msg=what)
    ok = st == 0
    np.testing.assert_array_equal(out["last_extremal_index"].cpu().numpy()[ok],
                                  ref["last_extremal_index"][ok], err_msg=what)
    for k in keys:
        g = out[k].cpu().numpy()
        r = ref["t" if k == "time" else k]
        np.testing.assert_array_equal(g[ok], r[ok], err_msg="%s %s" % (what, k))
    return ok


@pytest.fixture(scope="module")
def long_batch(env):
    """64 paths x 7 joints x 2000 samples and the oracle's solution, computed once."""
    b = env["syn"].make_joint_batch(64, 7, 2000)
    ref = sp.oracle_solve(env["tpo"], b, 2000, nthreads=16)
    assert (ref["status"] == 0).all()
    return b, ref


@pytest.mark.parametrize("D", [3, 7, 8, 14])
@pytest.mark.parametrize("N", [63, 64, 65, 129, 193, 300])
def test_every_trip_shape_matches_the_oracle(env, D, N):
    """Trips of fewer than 64 samples, cnt * D no multiple of 64, a last trip of one sample, two
    groups of passes (D = 14), short paths. All 32 paths are solved, by the oracle and here."""
    b = env["syn"].make_joint_batch(32, D, N)
    ref = sp.oracle_solve(env["tpo"], b, N)
    assert (ref["status"] == 0).all()
    _, out = _solve(env, env["E"], b, N)
    assert _assert_bit_parity(out, ref, "D=%d N=%d" % (D, N)).all()


def test_long_paths_twice_the_same_bits(env, long_batch):
    b, ref = long_batch
    _, first = _solve(env, env["E"], b, 2000)
    assert _assert_bit_parity(first, ref, "first solve").all()
    _, second = _solve(env, env["E"], b, 2000)
    for k in KEYS + ("status", "last_extremal_index"):
        assert first[k].cpu().numpy().tobytes() == second[k].cpu().numpy().tobytes(), k


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_long_paths_through_every_pipelining_mode(env, long_batch, mode):
    b, ref = long_batch
    E = env["eng"].Engine(0)
    E.set_pipelining(mode)
    try:
        _, out = _solve(env, E, b, 2000)
        assert _assert_bit_parity(out, ref, "pipelining mode %d" % mode).all()
    finally:
        E.close()


def test_without_qd_and_qdd_nothing_else_changes(env, long_batch):
    b, ref = long_batch
    _, out = _solve(env, env["E"], b, 2000, with_derivs=False)
    assert "qd" not in out and "qdd" not in out
    assert _assert_bit_parity(out, ref, "no derivatives", keys=("time", "s", "sd", "sdd")).all()


def test_cartesian_batch_with_extra_rows(env):
    """D = 6 with the two Cartesian rows (E = 2) at N = 129: curved paths, some with a start
    velocity or a shifted start."""
    torch, eng, syn, tpo = env["torch"], env["eng"], env["syn"], env["tpo"]
    N = 129
    b = cp.concat([cp.with_starts(cp.make_family(f, 8, 6, N, seed=4), seed=k)
                   for k, f in enumerate(("singular", "idle"))])
    ref = cp.oracle_solve(tpo, b)
    out = eng.alloc_joint_outputs(16, N, 6, env["dev"])
    env["E"].time_cartesian_paths(syn.upload_cartesian_batch(b, env["dev"]), out)
    torch.cuda.synchronize()
    ok = _assert_bit_parity(out, ref, "cartesian D=6 N=%d" % N)
    assert ok.all(), ref["status"]


def test_ragged_sample_counts(env):
    torch, eng, syn, tpo, E = (env[k] for k in ("torch", "eng", "syn", "tpo", "E"))
    D, stride = 7, 300
    counts = np.array([63, 64, 65, 129, 193, 300, 128, 127, 191, 192, 257, 299, 100, 77, 200, 256],
                      dtype=np.int32)
    B = len(counts)
    b = syn.make_joint_batch(B, D, stride)
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
    lei = out["last_extremal_index"].cpu().numpy()
    for i, n in enumerate(counts):
        one = {k: b[k][i:i + 1] for k in ("knots", "control_points", "vmax", "amax", "path_start",
                                          "delta", "sd_start", "time_start")}
        one["safety"] = b["safety"]
        ref = sp.oracle_solve(tpo, one, int(n), nthreads=1)
        assert st[i] == ref["status"][0] == 0, (i, n)
        assert lei[i] == ref["last_extremal_index"][0], (i, n)
        for k in KEYS:
            np.testing.assert_array_equal(got[k][i, :n], ref["t" if k == "time" else k][0],
                                          err_msg="%s path %d n %d" % (k, i, n))
            assert (got[k][i, n:] == -7.0).all(), "wrote past n[b]"

"""Cartesian paths on the GPU against the oracle and the independent reference
(tests/hp_reference.py): every joint count the C-ABI accepts (D = 1 .. 16, C = 2D + 2 rows: 4 .. 34,
across the one- and two-word LP row sets), the fused D = 6 / 7 kernels against the generic path,
the straight moves' bang-bang window, and the pose sampler at the edges of quat_log / quat_power."""
import ctypes as C
import importlib
import os

import numpy as np
import pytest

import cartesian_paths as cp
import hp_reference as hp
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

KEYS = ("time", "s", "sd", "sdd", "q", "qd", "qdd")
NTHREADS = 8


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
    """An engine created with TPAMD_FORCE_GENERIC=1: D = 6 / 7 take k_cartesian_rows + run_rows."""
    os.environ["TPAMD_FORCE_GENERIC"] = "1"
    try:
        E = env["eng"].Engine(0)
    finally:
        del os.environ["TPAMD_FORCE_GENERIC"]
    return E


def _engine_solve(env, b, E=None):
    torch, eng, syn = env["torch"], env["eng"], env["syn"]
    B, N, D = b["ik_positions"].shape
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    (E or env["E"]).time_cartesian_paths(syn.upload_cartesian_batch(b, env["dev"]), out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _assert_same(got, ref, what):
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=what)
    ok = ref["status"] == 0
    np.testing.assert_array_equal(got["last_extremal_index"][ok], ref["last_extremal_index"][ok],
                                  err_msg=what)
    for k in KEYS:
        np.testing.assert_array_equal(got[k][ok], ref["t" if k == "time" else k][ok],
                                      err_msg="%s: %s" % (what, k))


def _family_batch(D, N, names=cp.FAMILIES, seed=0):
    parts = []
    for name in names:
        b = cp.make_family(name, 2, D, N, seed)
        if name in cp.CURVED:
            b = cp.with_starts(b, seed)
        parts.append(b)
    return cp.concat(parts)


def _check_dof(env, D, Ns, generic=None):
    for N in Ns:
        b = _family_batch(D, N)
        ref = cp.oracle_solve(env["tpo"], b, NTHREADS)
        assert (ref["status"] == 0).all()
        got = _engine_solve(env, b)
        _assert_same(got, ref, "D %d N %d" % (D, N))
        hp.check_cartesian_profile(b, got, accel_allowance=None)
        if generic is not None:
            gen = _engine_solve(env, b, generic)
            _assert_same(gen, ref, "generic D %d N %d" % (D, N))


# ----------------------------------------------------------- every joint count
@pytest.mark.parametrize("D", [d for d in range(1, 15)])
def test_every_dof_count_matches_the_oracle_and_the_reference(env, generic_engine, D):
    """Bit parity with the oracle and check_cartesian_profile, every family; D = 6 and 7 also on
    the generic path (TPAMD_FORCE_GENERIC=1), which must give the same bits as the fused one."""
    _check_dof(env, D, (300,), generic_engine if D in (6, 7) else None)


@pytest.mark.parametrize("D", [15, 16], ids=["D15_C32_one_word", "D16_C34_two_words"])
def test_lp_word_boundary_row_counts(env, D):
    """C = 2D + 2: D = 15 fills one 32-row word exactly, D = 16 needs the two-word row set
    (k_lp_rows<2>) -- until now run on one synthetic rows-mode path only."""
    _check_dof(env, D, (3, 4, 64, 300, 2000))


@pytest.mark.parametrize("D", [2, 6, 7])
def test_sample_count_edges(env, generic_engine, D):
    _check_dof(env, D, cp.SAMPLE_COUNTS, generic_engine if D in (6, 7) else None)


def test_long_path_8192_samples(env, generic_engine):
    b = cp.concat([cp.with_starts(cp.make_family("idle", 2, 7, 8192), 1),
                   cp.make_family("straight_trans", 2, 7, 8192)])
    ref = cp.oracle_solve(env["tpo"], b, NTHREADS)
    got = _engine_solve(env, b)
    _assert_same(got, ref, "N 8192")
    _assert_same(_engine_solve(env, b, generic_engine), ref, "generic N 8192")
    hp.check_cartesian_profile(b, got, accel_allowance=None)


# ------------------------------------------------------------------- optimality
@pytest.mark.parametrize("name", cp.STRAIGHT)
@pytest.mark.parametrize("D", [1, 6, 7, 16])
def test_straight_moves_end_in_the_bang_bang_window(env, name, D):
    """Rest to rest along a straight line: the engine's time up to sample N-2 is the bang-bang
    optimum of the path shortened by one sample, within the grid's corner allowance
    (hp_reference.cartesian_bang_bang_time), and the active rows are those of the regime."""
    for N in (64, 2000):
        b = cp.make_family(name, 4, D, N)
        got = _engine_solve(env, b)
        assert (got["status"] == 0).all()
        rep = hp.check_cartesian_profile(b, got)
        for i in range(4):
            assert got["sd"][i, -2] == 0.0
            lo, hi = hp.straight_window(b, i)
            t = got["time"][i, -2] - got["time"][i, 0]
            assert lo <= t <= hi, (name, D, N, i, lo, t, hi)
        if name == "straight_trans":
            assert rep["trans_active"] > 0
        elif name == "straight_rot":
            assert rep["rot_active"] > 0


# --------------------------------------------------------------- pose sampling
def _device_poses(env, e):
    torch, E = env["torch"], env["E"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(env["dev"])
    kn, tr, ro = t(e["knots"]), t(e["translation"]), t(e["rotation"])
    ps, dl = t(e["path_start"]), t(e["delta"])
    Bn, P = tr.shape[0], tr.shape[1]
    out = torch.full((Bn, e["N"], 7), -7.0, dtype=torch.float64, device=env["dev"])
    rc = E._lib.tpamd_sample_pose_splines_device(
        E._h, Bn, e["N"], P, kn.data_ptr(), tr.data_ptr(), ro.data_ptr(), ps.data_ptr(),
        dl.data_ptr(), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


# Quaternion tolerance against the reference: the kernel takes log / atan2 / sin / cos / exp from
# the device math library; measured at most 6.7e-16 (P = 3, 16, 1023), held to 4e-15 as the oracle
# is on the CPU. Translations are sums of three products, held to the same 4e-15; padded samples
# are the last control pose, bit for bit.
QUAT_TOL = 4e-15


@pytest.mark.parametrize("P,N", [(3, 80), (16, 400), (1023, 1100)])
def test_pose_sampling_at_the_edges_matches_the_reference(env, P, N):
    e = cp.pose_edge_paths(P, N)
    rc, dev = _device_poses(env, e)
    assert rc == 0
    host = env["E"].sample_pose_splines(e["knots"], e["translation"], e["rotation"],
                                        e["path_start"], e["delta"], N)
    np.testing.assert_array_equal(host, dev)
    worst = 0.0
    for b in range(e["knots"].shape[0]):
        ref = hp.sample_poses(e["knots"][b], e["translation"][b], e["rotation"][b],
                              e["path_start"][b], e["delta"][b], N).astype(float)
        _, pad = hp.pose_parameters(e["knots"][b], e["path_start"][b], e["delta"][b], N)
        np.testing.assert_array_equal(dev[b, pad], ref[pad], err_msg="padding, path %d" % b)
        assert np.max(np.abs(dev[b, :, :3] - ref[:, :3])) <= 4e-15, b
        err = float(np.max(np.abs(dev[b, :, 3:] - ref[:, 3:])))
        worst = max(worst, err)
        assert err <= QUAT_TOL, (b, err)
    print("pose sampling P %d: largest quaternion difference to the reference %.3e" % (P, worst))


def test_pose_sampling_one_sample(env):
    e = cp.pose_edge_paths(16, 400)
    e = dict(e, N=1)
    rc, dev = _device_poses(env, e)
    assert rc == 0
    for b in range(e["knots"].shape[0]):
        ref = hp.sample_poses(e["knots"][b], e["translation"][b], e["rotation"][b],
                              e["path_start"][b], e["delta"][b], 1).astype(float)
        assert np.max(np.abs(dev[b] - ref)) <= QUAT_TOL


def test_pose_sampling_refuses_more_control_points_than_lds_holds(env):
    """P = 1023 fills the 64 KB of LDS the kernel asks for (above); P = 1024 would not and must be
    refused before any launch, by both entry points."""
    e = cp.pose_edge_paths(1024, 1100)
    rc, dev = _device_poses(env, e)
    assert rc == -3                                        # TPAMD_E_UNSUPPORTED
    assert (dev == -7.0).all()                             # nothing written
    E = env["E"]
    a = {k: np.ascontiguousarray(e[k], dtype=np.float64) for k in
         ("knots", "translation", "rotation", "path_start", "delta")}
    out = np.zeros((a["knots"].shape[0], e["N"], 7))
    rc = E._lib.tpamd_sample_pose_splines_host(
        E._h, a["knots"].shape[0], e["N"], 1024, a["knots"].ctypes.data, a["translation"].ctypes.data,
        a["rotation"].ctypes.data, a["path_start"].ctypes.data, a["delta"].ctypes.data,
        out.ctypes.data)
    assert rc == -3

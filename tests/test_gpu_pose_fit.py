"""The Cartesian waypoint fit on the GPU (tpamd_fit_pose_waypoints_host / _device,
Engine.fit_pose_waypoints): one ragged call over every case family of tests/pose_fit_reference.py, the
joint control points against the oracle bit for bit, the pose control points and path_end against the
long-double restatement, the packing, the empty path, and the host form against the device form."""
import ctypes as C
import importlib

import numpy as np
import pytest

import pose_fit_reference as pfr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

TPAMD_PLAN_INVALID_ARGUMENT = 3


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    return dict(torch=torch, eng=eng, tpo=tpo, E=eng.Engine(0), dev=torch.device("cuda", 0))


def _pack(cases):
    D = cases[0]["D"]
    off = np.concatenate([[0], np.cumsum([c["W"] for c in cases])]).astype(np.int32)
    pose = np.concatenate([c["pose"].reshape(-1, 7) for c in cases])
    joints = np.concatenate([c["joints"].reshape(-1, D) for c in cases])
    tr = np.array([c["tr"] for c in cases])
    rr = np.array([c["rr"] for c in cases])
    return off, np.ascontiguousarray(pose), np.ascontiguousarray(joints), tr, rr


def _fit_device(env, cases):
    torch, dev = env["torch"], env["dev"]
    off, pose, joints, tr, rr = _pack(cases)
    up = lambda a: torch.from_numpy(a).to(dev)
    fit = env["E"].fit_pose_waypoints(up(pose), up(joints), off, up(tr), up(rr))
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in fit.items()}


def _fit_host(env, cases):
    off, pose, joints, tr, rr = _pack(cases)
    return env["E"].fit_pose_waypoints(pose, joints, off, tr, rr)


def _check_against_references(env, cases, fit):
    """Packing, counts and statuses exact; joint control points bit-equal to the oracle; pose control
    points and path_end within the bound of the long-double reference. Returns the worst deviations."""
    tpo = env["tpo"]
    npts = np.array([0 if c["W"] < 1 else max(3 * c["W"] - 2, 4) for c in cases], dtype=np.int32)
    np.testing.assert_array_equal(fit["num_points"], npts)
    np.testing.assert_array_equal(fit["point_offsets"], np.concatenate([[0], np.cumsum(npts)]))
    np.testing.assert_array_equal(fit["status"], np.where(npts == 0, TPAMD_PLAN_INVALID_ARGUMENT, 0))
    assert fit["knots"].shape == (int((npts + 3 * (npts > 0)).sum()),)
    assert fit["translation_points"].shape == (int(npts.sum()), 3)
    worst = dict(translation=0.0, rotation=0.0, path_end=0.0)
    ko = 0
    for k, c in enumerate(cases):
        P = int(npts[k])
        if P == 0:
            assert fit["path_end"][k] == 0.0
            continue
        p0 = int(fit["point_offsets"][k])
        knots = fit["knots"][ko:ko + P + 3]
        ko += P + 3
        assert fit["path_end"][k] == knots[-1]
        ocp = tpo.polyline_to_bspline3_waypoints(c["joints"], c["rr"])
        assert ocp.tobytes() == fit["joint_control_points"][p0:p0 + P].tobytes(), (k, c["family"])
        jf_cp, _ = tpo.joint_fit_spline(c["joints"], c["rr"])
        assert jf_cp.tobytes() == ocp.tobytes()
        ref = pfr.fit(c["pose"], c["joints"], c["tr"], c["rr"])
        worst["translation"] = max(worst["translation"], pfr.deviation(fit["translation_points"][p0:p0 + P], ref["translation"]))
        worst["rotation"] = max(worst["rotation"], pfr.deviation(fit["rotation_points"][p0:p0 + P], ref["rotation"]))
        worst["path_end"] = max(worst["path_end"], pfr.deviation(knots[-1:], ref["knots"][-1:]))
        assert pfr.deviation(knots, ref["knots"]) < 1e-13
        # corners pass through untouched
        if c["W"] > 1:
            assert (fit["translation_points"][p0:p0 + P:3] == c["pose"][:, :3]).all()
            assert (fit["rotation_points"][p0:p0 + P:3] == c["pose"][:, 3:]).all()
    return worst


def test_ragged_fit_against_oracle_and_long_double(env):
    """B = 12 ragged D = 7 paths (W = 1, 2, 3, 4, 6, 2, 3, 5, 1, 2, 3, 0) over every family."""
    cases = pfr.gpu_batch()
    assert [c["W"] for c in cases] == [1, 2, 3, 4, 6, 2, 3, 5, 1, 2, 3, 0]
    assert {c["family"] for c in cases} >= set(pfr.FAMILIES)
    dev_fit, host_fit = _fit_device(env, cases), _fit_host(env, cases)
    worst = _check_against_references(env, cases, dev_fit)
    print("device pose fit, worst deviation from long double / max(1, |x|): %r" % worst)
    for key, value in worst.items():
        assert value <= pfr.BOUND, (key, value)
    for key in dev_fit:                       # the _host and _device forms agree bit for bit
        assert np.asarray(dev_fit[key]).tobytes() == np.asarray(host_fit[key]).tobytes(), key


@pytest.mark.parametrize("D", [1, 16])
def test_one_path_of_the_other_joint_counts(env, D):
    rng = np.random.default_rng(900 + D)
    pose, joints = pfr.make_case("random", 4, D, rng)
    cases = [dict(family="random", W=4, D=D, tr=0.1, rr=0.2, pose=pose, joints=joints)]
    fit = _fit_device(env, cases)
    worst = _check_against_references(env, cases, fit)
    print("device pose fit D %d, worst deviation: %r" % (D, worst))
    assert max(worst.values()) <= pfr.BOUND
    host = _fit_host(env, cases)
    for key in fit:
        assert np.asarray(fit[key]).tobytes() == np.asarray(host[key]).tobytes(), key


def _raw_device_fit(env, cases, slack=5, fill=-7.0):
    """tpamd_fit_pose_waypoints_device into tensors pre-filled with `fill`, `slack` slots larger than
    the call needs."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    off, pose, joints, tr, rr = _pack(cases)
    B, D = len(cases), cases[0]["D"]
    npts = np.array([0 if c["W"] < 1 else max(3 * c["W"] - 2, 4) for c in cases])
    P, K = int(npts.sum()), int((npts + 3 * (npts > 0)).sum())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    new = lambda *shape: torch.full(shape, fill, dtype=torch.float64, device=dev)
    out = dict(knots=new(K + slack), translation_points=new(P + slack, 3), rotation_points=new(P + slack, 4),
               joint_control_points=new(P + slack, D), path_end=new(B + slack),
               num_points=torch.full((B + slack,), -7, dtype=torch.int32, device=dev),
               status=torch.full((B + slack,), -7, dtype=torch.int32, device=dev))
    args = [up(pose), up(joints), up(tr), up(rr)]
    po = np.full(B + 1, -7, dtype=np.int32)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    rc = E._lib.tpamd_fit_pose_waypoints_device(
        E._h, B, D, off.ctypes.data, *(ptr(a) for a in args), ptr(out["knots"]), ptr(out["translation_points"]),
        ptr(out["rotation_points"]), ptr(out["joint_control_points"]), ptr(out["num_points"]), po.ctypes.data,
        ptr(out["path_end"]), ptr(out["status"]), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc, {k: v.cpu().numpy() for k, v in out.items()}, po, (P, K, B)


def test_empty_path_writes_nothing_and_disturbs_nobody(env):
    """The path without waypoints gets INVALID_ARGUMENT, num_points 0 and path_end 0 and no slots: the
    -7.0 fill behind the packed outputs is intact, and every other path's outputs are those of a
    call without it. An empty path in the middle of the batch behaves the same way."""
    cases = pfr.gpu_batch()
    rc, full, po, (P, K, B) = _raw_device_fit(env, cases)
    assert rc == 0 and po[-1] == P and po[-2] == P
    assert full["status"][B - 1] == TPAMD_PLAN_INVALID_ARGUMENT and full["num_points"][B - 1] == 0
    assert full["path_end"][B - 1] == 0.0
    for key, used in (("knots", K), ("translation_points", P), ("rotation_points", P), ("joint_control_points", P),
                      ("path_end", B), ("num_points", B), ("status", B)):
        assert (full[key][used:] == -7).all(), key
        assert not (full[key][:used] == -7).any(), key
    rc, without, po2, (P2, K2, B2) = _raw_device_fit(env, cases[:-1])
    assert rc == 0 and (P2, K2, B2) == (P, K, B - 1)
    for key, used in (("knots", K), ("translation_points", P), ("rotation_points", P), ("joint_control_points", P),
                      ("path_end", B - 1), ("num_points", B - 1), ("status", B - 1)):
        assert full[key][:used].tobytes() == without[key][:used].tobytes(), key
    middle = cases[:4] + [cases[-1]] + cases[4:-1]
    rc, mid, po3, _ = _raw_device_fit(env, middle)
    assert rc == 0 and po3[4] == po3[5]
    for key in ("knots", "translation_points", "rotation_points", "joint_control_points"):
        assert mid[key].tobytes() == without[key].tobytes(), key
    assert mid["status"][4] == TPAMD_PLAN_INVALID_ARGUMENT and mid["path_end"][4] == 0.0
    np.testing.assert_array_equal(np.delete(mid["path_end"][:B], 4), without["path_end"][:B - 1])


def test_call_level_errors_write_nothing(env):
    torch, dev, E, eng = env["torch"], env["dev"], env["E"], env["eng"]
    cases = pfr.gpu_batch()[:3]
    off, pose, joints, tr, rr = _pack(cases)
    bad = off.copy()
    bad[0] = 1
    with pytest.raises(eng.TpamdError):
        E.fit_pose_waypoints(pose, joints, bad, tr, rr)
    bad = off.copy()
    bad[2] = bad[1] - 1
    with pytest.raises(eng.TpamdError):
        E.fit_pose_waypoints(pose, joints, bad, tr, rr)
    with pytest.raises(eng.TpamdError):
        E.fit_pose_waypoints(pose, np.zeros((pose.shape[0], 17)), off, tr, rr)
    out = np.full(8, -7.0)
    po = np.full(4, -7, dtype=np.int32)
    rc = E._lib.tpamd_fit_pose_waypoints_host(E._h, -1, 7, off.ctypes.data, pose.ctypes.data, joints.ctypes.data,
                                              tr.ctypes.data, rr.ctypes.data, out.ctypes.data, out.ctypes.data,
                                              out.ctypes.data, out.ctypes.data, po.ctypes.data, po.ctypes.data,
                                              out.ctypes.data, po.ctypes.data)
    assert rc == -1 and (out == -7).all() and (po == -7).all()
    rc = E._lib.tpamd_fit_pose_waypoints_host(E._h, 3, 7, off.ctypes.data, pose.ctypes.data, joints.ctypes.data,
                                              None, rr.ctypes.data, out.ctypes.data, out.ctypes.data,
                                              out.ctypes.data, out.ctypes.data, po.ctypes.data, po.ctypes.data,
                                              out.ctypes.data, po.ctypes.data)
    assert rc == -1 and (out == -7).all() and (po == -7).all()

"""The IK-target sampler on the GPU (tpamd_sample_ik_targets_host / _device, Engine.sample_ik_targets):
ragged batches built from the device fit's own output and from hand-made pose splines at the edges of
the quaternion B-spline (cartesian_paths.pose_edge_paths, P = 3 and P = 16 in one call), against the
oracle's EvalCurve (bit for bit), the long-double pose reference (hp_reference.sample_poses), the
uniform pose sampler (bit for bit), with padded rows, untouched neighbours and a P = 2000 path."""
import ctypes as C
import importlib

import numpy as np
import pytest

import cartesian_paths as cp
import hp_reference as hp
import pose_fit_reference as pfr
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

TOL = 4e-15                     # tests/test_gpu_cartesian_hp.py QUAT_TOL


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


def _check_path(env, knots, tr, rot, jcp, delta, pose, joint, what):
    """One path's targets against the references. Returns the largest pose deviation."""
    tpo = env["tpo"]
    rows = pose.shape[0]
    ref = hp.sample_poses(knots, tr, rot, 0.0, delta, rows)
    par, pad = hp.pose_parameters(knots, 0.0, delta, rows)
    np.testing.assert_array_equal(pose[pad], ref[pad].astype(float), err_msg="padded poses, " + what)
    np.testing.assert_array_equal(pose[pad], np.tile(np.concatenate([tr[-1], rot[-1]]), (int(pad.sum()), 1)))
    np.testing.assert_array_equal(joint[pad], np.tile(jcp[-1], (int(pad.sum()), 1)), err_msg="padded joints, " + what)
    for r in np.flatnonzero(~pad):
        rc, val = tpo.eval_curve(knots, 2, jcp, par[r])
        assert rc == 0 and val.tobytes() == joint[r].tobytes(), (what, int(r))
    err = np.abs(pose.astype(hp.LD) - ref)
    worst = float(err.max()) if rows else 0.0
    assert worst <= TOL, (what, worst)
    return worst


def test_targets_from_the_device_fit(env):
    """The device fit's own output as the spline (knots.back() is one number on both sides of the
    padding rule), delta per path chosen for 1, 255, 256, 257 and 1003 rows in one call."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    cases = [c for c in pfr.gpu_batch() if c["W"] >= 2][:5]
    off = np.concatenate([[0], np.cumsum([c["W"] for c in cases])]).astype(np.int32)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    fit = E.fit_pose_waypoints(up(np.concatenate([c["pose"] for c in cases])),
                               up(np.concatenate([c["joints"] for c in cases])), off,
                               up(np.array([c["tr"] for c in cases])), up(np.array([c["rr"] for c in cases])))
    path_end = fit["path_end"].cpu().numpy()
    rows = np.array([1, 255, 256, 257, 1003])
    delta = path_end / np.maximum(rows - 6, 1)            # the last few rows of every path are padding
    row_offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    pose, joint = E.sample_ik_targets(fit, up(delta), row_offsets)
    torch.cuda.synchronize()
    assert pose.is_cuda and joint.is_cuda
    host = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in fit.items()}
    pose_h, joint_h = E.sample_ik_targets(host, delta, row_offsets)      # the _host form, bit for bit
    pose, joint = pose.cpu().numpy(), joint.cpu().numpy()
    assert pose.tobytes() == pose_h.tobytes() and joint.tobytes() == joint_h.tobytes()
    worst, ko = 0.0, 0
    for k in range(len(cases)):
        P, p0 = int(host["num_points"][k]), int(host["point_offsets"][k])
        r = slice(int(row_offsets[k]), int(row_offsets[k + 1]))
        worst = max(worst, _check_path(env, host["knots"][ko:ko + P + 3], host["translation_points"][p0:p0 + P],
                                       host["rotation_points"][p0:p0 + P], host["joint_control_points"][p0:p0 + P],
                                       delta[k], pose[r], joint[r], "fitted path %d" % k))
        ko += P + 3
    print("IK targets from the device fit: largest pose deviation from long double %.3e" % worst)


def _edge_batch(D=7):
    """cartesian_paths.pose_edge_paths(3, 80) and (16, 400) concatenated into one ragged batch, with
    random joint control points. Every family keeps its delta and row count (path_start is 0 here:
    row r belongs to r * delta)."""
    rng = np.random.default_rng(31)
    paths = []
    for P, N in ((3, 80), (16, 400)):
        e = cp.pose_edge_paths(P, N)
        for b in range(e["knots"].shape[0]):
            paths.append(dict(P=P, rows=N, knots=e["knots"][b], tr=e["translation"][b], rot=e["rotation"][b],
                              delta=float(e["delta"][b]), jcp=rng.uniform(-2.0, 2.0, (P, D))))
    return paths


def _fit_dict(paths):
    return dict(knots=np.concatenate([p["knots"] for p in paths]),
                translation_points=np.concatenate([p["tr"] for p in paths]),
                rotation_points=np.concatenate([p["rot"] for p in paths]),
                joint_control_points=np.concatenate([p["jcp"] for p in paths]),
                num_points=np.array([p["P"] for p in paths], dtype=np.int32), point_offsets=None)


def test_ragged_edge_splines_mixed_sizes(env):
    """P = 3 and P = 16 in one call, at the edges of quat_log / quat_power, rows on knots and on the
    padding edge; each uniform-P half equals Engine.sample_pose_splines with path_start 0 bit for bit."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    paths = _edge_batch()
    fit = _fit_dict(paths)
    rows = np.array([p["rows"] for p in paths])
    row_offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    delta = np.array([p["delta"] for p in paths])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dfit = {k: (up(v) if k not in ("num_points", "point_offsets") else v) for k, v in fit.items()}
    pose, joint = E.sample_ik_targets(dfit, up(delta), row_offsets)
    torch.cuda.synchronize()
    pose, joint = pose.cpu().numpy(), joint.cpu().numpy()
    worst = 0.0
    for k, p in enumerate(paths):
        r = slice(int(row_offsets[k]), int(row_offsets[k + 1]))
        worst = max(worst, _check_path(env, p["knots"], p["tr"], p["rot"], p["jcp"], p["delta"], pose[r], joint[r],
                                       "edge path %d (P %d)" % (k, p["P"])))
    print("IK targets on the edge splines: largest pose deviation from long double %.3e" % worst)
    for P in (3, 16):
        idx = [k for k, p in enumerate(paths) if p["P"] == P]
        N = paths[idx[0]]["rows"]
        uniform = E.sample_pose_splines(np.array([paths[k]["knots"] for k in idx]), np.array([paths[k]["tr"] for k in idx]),
                                        np.array([paths[k]["rot"] for k in idx]), 0.0, delta[idx], N)
        got = np.array([pose[row_offsets[k]:row_offsets[k + 1]] for k in idx])
        assert got.tobytes() == uniform.tobytes(), P


def test_neighbouring_rows_stay_untouched(env):
    """Pre-filled outputs: a path whose device-side delta is not positive keeps its rows, its
    neighbours are written as in a call of their own, and nothing is written behind the last row."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    paths = [_edge_batch()[k] for k in (0, 9, 3)]            # P = 3, 16, 3; rows 80, 400, 80
    fit = _fit_dict(paths)
    D = fit["joint_control_points"].shape[1]
    rows = np.array([p["rows"] for p in paths])
    row_offsets = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    total = int(rows.sum())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    arrays = [up(fit[k]) for k in ("knots", "translation_points", "rotation_points", "joint_control_points")]

    def call(delta):
        pose = torch.full((total + 9, 7), -7.0, dtype=torch.float64, device=dev)
        joint = torch.full((total + 9, D), -7.0, dtype=torch.float64, device=dev)
        dl = up(np.asarray(delta, dtype=float))
        ptr = lambda t: C.c_void_p(t.data_ptr())
        rc = E._lib.tpamd_sample_ik_targets_device(
            E._h, len(paths), D, fit["num_points"].ctypes.data, row_offsets.ctypes.data, *(ptr(a) for a in arrays), ptr(dl),
            ptr(pose), ptr(joint), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0
        return pose.cpu().numpy(), joint.cpu().numpy()

    good = [p["delta"] for p in paths]
    pose, joint = call(good)
    assert (pose[total:] == -7).all() and (joint[total:] == -7).all() and not (pose[:total] == -7).any()
    for bad in (0.0, -1.0, float("nan")):
        pose_b, joint_b = call([good[0], bad, good[2]])
        mid = slice(int(row_offsets[1]), int(row_offsets[2]))
        assert (pose_b[mid] == -7).all() and (joint_b[mid] == -7).all()
        for r in (slice(0, int(row_offsets[1])), slice(int(row_offsets[2]), total)):
            assert pose_b[r].tobytes() == pose[r].tobytes() and joint_b[r].tobytes() == joint[r].tobytes()
        assert (pose_b[total:] == -7).all() and (joint_b[total:] == -7).all()
    # the host form refuses such a delta and writes nothing
    out_p, out_j = np.full((total, 7), -7.0), np.full((total, D), -7.0)
    dl = np.array([good[0], 0.0, good[2]])
    rc = E._lib.tpamd_sample_ik_targets_host(
        E._h, len(paths), D, fit["num_points"].ctypes.data, row_offsets.ctypes.data, fit["knots"].ctypes.data,
        fit["translation_points"].ctypes.data, fit["rotation_points"].ctypes.data,
        fit["joint_control_points"].ctypes.data, dl.ctypes.data, out_p.ctypes.data, out_j.ctypes.data)
    assert rc == -1 and (out_p == -7).all() and (out_j == -7).all()
    two = fit["num_points"].copy()
    two[1] = 2
    dl = np.array(good)
    rc = E._lib.tpamd_sample_ik_targets_host(
        E._h, len(paths), D, two.ctypes.data, row_offsets.ctypes.data, fit["knots"].ctypes.data,
        fit["translation_points"].ctypes.data, fit["rotation_points"].ctypes.data,
        fit["joint_control_points"].ctypes.data, dl.ctypes.data, out_p.ctypes.data, out_j.ctypes.data)
    assert rc == -1 and (out_p == -7).all()


def test_a_path_of_2000_control_points_is_sampled(env):
    """No LDS limit: P = 2000 (the uniform pose sampler stops at 1023), next to a P = 3 path."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    rng = np.random.default_rng(2000)
    P, D, rows = 2000, 7, 2100
    kn = np.concatenate([[0.0, 0.0], np.arange(P - 1, dtype=float), [P - 2.0, P - 2.0]])
    rot = rng.standard_normal((P, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    big = dict(P=P, rows=rows, knots=kn, tr=rng.uniform(-1, 1, (P, 3)), rot=rot, delta=kn[-1] / (rows - 30),
               jcp=rng.uniform(-2, 2, (P, D)))
    paths = [_edge_batch()[2], big]
    fit = _fit_dict(paths)
    row_offsets = np.array([0, paths[0]["rows"], paths[0]["rows"] + rows], dtype=np.int32)
    delta = np.array([p["delta"] for p in paths])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dfit = {k: (up(v) if k not in ("num_points", "point_offsets") else v) for k, v in fit.items()}
    pose, joint = E.sample_ik_targets(dfit, up(delta), row_offsets)
    torch.cuda.synchronize()
    pose, joint = pose.cpu().numpy(), joint.cpu().numpy()
    worst = 0.0
    for k, p in enumerate(paths):
        r = slice(int(row_offsets[k]), int(row_offsets[k + 1]))
        worst = max(worst, _check_path(env, p["knots"], p["tr"], p["rot"], p["jcp"], p["delta"], pose[r], joint[r],
                                       "P %d" % p["P"]))
    print("IK targets, P = 2000: largest pose deviation from long double %.3e" % worst)

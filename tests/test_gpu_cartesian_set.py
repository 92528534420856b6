"""Cartesian planner sets on the GPU (tpamd_planner_set_create_cartesian, _upload_ik_tables[_device],
_download_ik_table): tests/cpp/test_cartesian_set_gpu.cc plans sets of 256 planners at D = 5 (generic
rows kernel), 6 and 7 (fused kernels) with both sampling methods out of resident IK tables and holds
every Plan's summaries and trajectories against one oracle IK-table planner per planner, bit for bit;
it asserts that every oracle planner returns OK at every step and reaches its target. It also covers
the modified-state re-upload, per-planner failures, capacity growth, the _device upload on a
non-blocking stream, the kind checks and the PCIe bytes of a Plan."""
import numpy as np
import pytest

from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_cartesian_sets_against_oracle_planners(tmp_path):
    require_gpu()
    exe = build_driver("test_cartesian_set_gpu.cc", tmp_path, libs=("engine", "oracle", "hip", "m"), flags=("-pthread",))
    out = run_driver(exe, timeout=1500, head=6000, tail=3000)
    assert out.count("family: D") == 6
    assert out.count("modified") == 3 and "modified + growth" in out
    assert out.count("failures: internal at Plan") == 2
    assert "device upload against host upload: 12 of 12 Plan calls equal, 64 tables equal" in out
    assert "IK-table entries on a joint set: refused, plans unchanged" in out
    assert "device upload with a bad delta and a bad state: statuses 0 1 1 0" in out


def test_cartesian_sets_against_mirror_planners_and_downstream(tmp_path):
    """tests/cpp/test_cartesian_set_mirror_gpu.cc: sets loaded through SetCartesianPaths from real
    TimeableCartesianSplinePaths equal one mirror PathTimingTrajectory per planner planning window
    by window; setpoints, packed downloads, stop parameters, stopping trajectories and the buffer-set
    insert on such a set give what the host flows give on the downloaded trajectory."""
    require_gpu()
    exe = build_driver("test_cartesian_set_mirror_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=1200)
    assert out.count("mirror family (") == 2
    assert "Cartesian methods on a joint set: refused" in out


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.parametrize("D,method", [(5, 0), (7, 1)])
def test_cartesian_planner_set_from_cuda_tensors(D, method):
    """engine.PlannerSet(cartesian=True) fed CUDA tensors (the Jacobians are computed with torch ops
    on the device and never leave it) against a set fed the same tables as numpy arrays: every
    Plan's summary, the packed trajectories and sample_at_ticks into CUDA tensors agree bit for bit."""
    import importlib
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    from oracle import tpo
    tpo.build()
    MS = 1_000_000
    B, N = 24, 300
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5000 + D)
    qs, offsets, kend, delta = [], [0], [], []
    for b in range(B):
        wps = rng.uniform(-1, 1, (int(rng.integers(3, 7)), D))
        cps, knots = tpo.joint_fit_spline(wps, 0.2)
        dl = (0.25 if b % 2 else 0.4) * knots[-1] / (N - 1)
        rows = int(round(knots[-1] / dl)) + N + 1
        q, _, _ = tpo.joint_sample_path(knots, cps, 0.0, dl, rows)
        qs.append(np.ascontiguousarray(q))
        offsets.append(offsets[-1] + rows)
        kend.append(knots[-1])
        delta.append(dl)
    offsets = np.asarray(offsets, dtype=np.int32)
    q = torch.from_numpy(np.concatenate(qs)).to(dev)
    c = torch.arange(6, device=dev, dtype=torch.float64)[None, :, None]
    d = torch.arange(D, device=dev, dtype=torch.float64)[None, None, :]
    J = (0.2 * torch.sin(q[:, None, :] * (c + 1.0) + 0.31 * d) + (c == d)).contiguous()
    vmax = torch.from_numpy(rng.uniform(0.5, 1.1, (B, D))).to(dev)
    amax = torch.from_numpy(rng.uniform(1.2, 3.0, (B, D))).to(dev)
    vt = torch.from_numpy(rng.uniform(0.3, 0.6, B)).to(dev)
    vr = torch.from_numpy(rng.uniform(0.8, 1.2, B)).to(dev)
    pe, dl = torch.tensor(kend, dtype=torch.float64, device=dev), torch.tensor(delta, dtype=torch.float64, device=dev)
    E = eng.Engine(0)
    kw = dict(time_step_ns=4 * MS, sampling_method=method, max_planning_iterations=10000, cartesian=True)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as a, eng.PlannerSet(E, B, D, N, **kw) as h:
        assert a.cartesian and h.cartesian
        a.set_ik_tables(q, J, offsets, pe, vmax, amax, vt, vr, dl)                 # CUDA tensors: the _device entry
        h.set_ik_tables(*(x.cpu().numpy() if hasattr(x, "cpu") else x for x in (q, J, offsets, pe, vmax, amax, vt, vr, dl)))
        tq, tJ = a.download_ik_table(3)
        r = slice(int(offsets[3]), int(offsets[4]))
        assert _bits(tq) == _bits(q[r]) and _bits(tJ) == _bits(J[r])
        with pytest.raises(eng.TpamdError):
            a.download_path(0)
        with pytest.raises(eng.TpamdError):
            a.set_waypoints(torch.zeros((2, D), dtype=torch.float64), np.array([0, 2], dtype=np.int32),
                            np.ones((1, D)), np.ones((1, D)), 0.01, ids=[0])
        start = np.zeros(B, dtype=np.int64)
        steps = 0
        while steps < 200:
            sa, sh = a.plan(start, 750 * MS), h.plan(start, 750 * MS)
            for name in sa:
                assert _bits(sa[name]) == _bits(sh[name]), (steps, name)
            assert (sa["status"] == 0).all()
            ta, th = a.download_trajectories(), h.download_trajectories()
            torch.cuda.synchronize()
            for name in ta:
                assert _bits(ta[name]) == _bits(th[name]), (steps, name)
            t0 = torch.from_numpy(start + 2 * MS).to(dev)
            xa = a.sample_at_ticks(t0, MS, 16)
            xh = h.sample_at_ticks(start + 2 * MS, MS, 16, host=True)
            torch.cuda.synchronize()
            assert xa["q"].is_cuda
            for name in ("status", "q", "qd", "qdd"):
                assert _bits(xa[name]) == _bits(xh[name]), (steps, name)
            assert (xa["status"].cpu() == 0).all()
            steps += 1
            done = sa["target_reached"].numpy() != 0
            if done.all():
                break
            start = np.where(done, start, np.minimum(sa["end_time_ns"].numpy(), start + 200 * MS))
        assert steps > 8 and done.all()
        with eng.PlannerSet(E, 2, D, N, time_step_ns=4 * MS) as joint:
            with pytest.raises(eng.TpamdError):
                joint.set_ik_tables(qs[0], J[:qs[0].shape[0]].cpu().numpy(), np.array([0, qs[0].shape[0]], dtype=np.int32),
                                    kend[0], np.ones((1, D)), np.ones((1, D)), 0.5, 1.0, delta[0], ids=[0])
            with pytest.raises(eng.TpamdError):
                joint.download_ik_table(0)

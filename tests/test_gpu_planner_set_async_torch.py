"""PlannerSet.plan_async on the GPU: the enqueued-only Plan driven from PyTorch on a non-default
stream equals plan() on a twin PlannerSet, field by field and in the setpoints read into CUDA
tensors, over a first Plan and three replans (B = 70, D = 7, N = 100)."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


def test_plan_async_equals_plan_on_a_twin():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    B, D, N, T, max_windows = 70, 7, 100, 6, 3
    ms = 1_000_000
    rng = np.random.default_rng(20)
    dev = torch.device("cuda", 0)
    E = eng.Engine(0)
    W = 3
    wps = torch.from_numpy(rng.uniform(-1.5, 1.5, (B * W, D))).to(dev)
    offsets = np.arange(B + 1, dtype=np.int32) * W
    vmax = torch.from_numpy(rng.uniform(1.0, 2.0, (B, D))).to(dev)
    amax = torch.from_numpy(rng.uniform(2.0, 5.0, (B, D))).to(dev)
    delta = torch.full((B,), 0.005, dtype=torch.float64, device=dev)
    stream = torch.cuda.Stream(device=dev)
    with eng.PlannerSet(E, B, D, N, time_step_ns=ms) as ps, \
            eng.PlannerSet(E, B, D, N, time_step_ns=ms, max_planning_iterations=max_windows - 1) as twin:
        for s in (ps, twin):
            s.set_waypoints(wps, offsets, vmax, amax, delta)
        h0, t0 = ps.capacity()
        ps.reserve(h0 + 10, 0)
        assert ps.capacity() == (h0 + 10, t0)
        torch.cuda.synchronize()
        ok_plans = 0
        for k in range(4):
            start = torch.full((B,), (1000 + 100 * k) * ms, dtype=torch.int64, device=dev)
            horizon = torch.full((B,), 400 * ms, dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            handle = ps.plan_async(start, horizon, max_windows=max_windows, stream=stream)
            # the sample counts of this plan are on the device: what needs them says so
            with pytest.raises(eng.TpamdError):
                ps.download_trajectories()
            with pytest.raises(eng.TpamdError):
                ps.plan_async(start, horizon, stream=stream)
            assert handle.summary.is_cuda and handle.info.is_cuda
            got = handle.result()
            want = twin.plan(start.cpu(), horizon.cpu())
            assert ps.last_plan_bytes() == (0, 0)
            for name, value in want.items():
                assert torch.equal(got[name], value), (k, name)
            info = got["info"]
            assert info["num_ok"] == int((want["status"] == 0).sum())
            assert info["num_failed"] == B - info["num_ok"] and info["num_exhausted"] == 0
            assert info["max_windows_solved"] == int(want["windows"].max())
            assert info["needed_history"] == 0 and info["needed_trajectory"] == 0
            ok_plans += info["num_ok"]
            ticks = start + 20 * ms
            a = ps.sample_at_ticks(ticks, 4 * ms, T)
            b = twin.sample_at_ticks(ticks, 4 * ms, T)
            torch.cuda.synchronize()
            assert torch.equal(a["status"], b["status"])
            assert int((a["status"] == 0).sum()) > 0
            for name in ("q", "qd", "qdd"):
                assert a[name].cpu().numpy().tobytes() == b[name].cpu().numpy().tobytes(), (k, name)
            ta, tb = ps.download_trajectories(), twin.download_trajectories()
            torch.cuda.synchronize()
            for name in ("offsets", "time", "s", "sd", "sdd", "q", "qd", "qdd"):
                assert ta[name].cpu().numpy().tobytes() == tb[name].cpu().numpy().tobytes(), (k, name)
        assert ok_plans >= 2 * B
    E.close()

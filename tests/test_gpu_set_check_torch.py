"""PlannerSet.set_checking / check_results / check_results_device from PyTorch: the records a
plan_async call leaves, read into a CUDA tensor by a call enqueued behind it on the same non-default
stream with no synchronisation in between, equal the host entry's and those of a twin set that
plans synchronously, over a first Plan and two replans of several windows each (B = 40, D = 7,
N = 64). With checking off the same calls give the "nothing checked" record and the same plans."""
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu


def test_check_results_follow_plan_async_on_a_stream():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    B, D, N, W, max_windows = 40, 7, 64, 5, 4
    ms = 1_000_000
    rng = np.random.default_rng(31)
    dev = torch.device("cuda", 0)
    E = eng.Engine(0)
    wps = torch.from_numpy(rng.uniform(-2.0, 2.0, (B * W, D))).to(dev)
    offsets = np.arange(B + 1, dtype=np.int32) * W
    vmax = torch.from_numpy(rng.uniform(1.0, 2.0, (B, D))).to(dev)
    amax = torch.from_numpy(rng.uniform(2.0, 4.0, (B, D))).to(dev)
    delta = torch.full((B,), 0.02, dtype=torch.float64, device=dev)       # coarse: OK windows that violate rows
    stream = torch.cuda.Stream(device=dev)
    size = eng.PLANNER_CHECK_DTYPE.itemsize
    kw = dict(time_step_ns=ms, max_planning_iterations=max_windows - 1)
    with eng.PlannerSet(E, B, D, N, **kw) as ps, eng.PlannerSet(E, B, D, N, **kw) as twin, \
            eng.PlannerSet(E, B, D, N, **kw) as plain:
        for s in (ps, twin, plain):
            s.set_waypoints(wps, offsets, vmax, amax, delta)
        ps.set_checking(True)
        twin.set_checking(True)
        ps.reserve(ps.capacity()[0] + 4 * N, 8192)      # plan_async cannot grow a buffer
        torch.cuda.synchronize()
        ids = torch.tensor([B - 1, 2, 0, 17], dtype=torch.int32, device=dev)
        many = violating = 0
        for k in range(3):
            start = torch.full((B,), (100 + 150 * k) * ms, dtype=torch.int64, device=dev)
            horizon = torch.full((B,), 2500 * ms, dtype=torch.int64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            out = torch.full((B, size), 0xAB, dtype=torch.uint8, device=dev)
            some = torch.full((4, size), 0xAB, dtype=torch.uint8, device=dev)
            handle = ps.plan_async(start, horizon, max_windows=max_windows, stream=stream)
            ps.check_results_device(out, stream=stream)                   # enqueued only, behind the Plan
            ps.check_results_device(some, ids=ids, stream=stream)
            got = handle.result()
            stream.synchronize()
            device_records = out.cpu().numpy().view(eng.PLANNER_CHECK_DTYPE).reshape(B)
            host_records = ps.check_results()
            assert device_records.tobytes() == host_records.tobytes(), k
            assert some.cpu().numpy().tobytes() == host_records[ids.cpu().numpy()].tobytes(), k
            want = twin.plan(start.cpu(), horizon.cpu())
            assert twin.check_results().tobytes() == host_records.tobytes(), k
            # checking changes no plan
            base = plain.plan(start.cpu(), horizon.cpu())
            for name, value in base.items():
                assert torch.equal(want[name], value) and torch.equal(got[name], value), (k, name)
            ta, tb = twin.download_trajectories(), plain.download_trajectories()
            torch.cuda.synchronize()
            for name in ("offsets", "time", "s", "sd", "sdd", "q", "qd", "qdd"):
                assert ta[name].cpu().numpy().tobytes() == tb[name].cpu().numpy().tobytes(), (k, name)
            none = plain.check_results()
            assert (none["windows"] == 0).all() and (none["violations"] == -1).all()
            assert np.isnan(none["worst_excess"]).all() and np.isnan(none["worst_parameter"]).all()
            # the records count the windows the summaries count
            ok = want["status"].numpy() == 0
            assert (host_records["windows"][ok] == want["windows"].numpy()[ok]).all()
            many += int((host_records["windows"] >= 2).sum())
            violating += int((host_records["violations"] > 0).sum())
        assert many > 0
        print("planners with >= 2 windows:", many, "with violations:", violating)
        # call-level errors write nothing
        keep = out.clone()
        with pytest.raises(eng.TpamdError):
            ps.check_results_device(torch.zeros((B + 1, size), dtype=torch.uint8, device=dev))
        with pytest.raises(eng.TpamdError):
            ps.check_results(np.array([0, 0], dtype=np.int32))
        with pytest.raises(eng.TpamdError):
            ps.check_results(np.array([B], dtype=np.int32))
        torch.cuda.synchronize()
        assert torch.equal(out, keep)
    E.close()

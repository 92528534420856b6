"""The tensor API of the planner state records (engine.PlannerSet.state_info / export_state /
import_state / copy_from): what the calls return, bad input, and an export and an import enqueued
on a side stream behind plan_async without the host in between."""
import importlib

import numpy as np
import pytest

import set_state_cases as cases
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

MS = cases.MS


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return dict(torch=torch, eng=eng, E=cases.engine(), dev=torch.device("cuda", 0))


def _moving_set(env, B, D, N, **kw):
    eng = env["eng"]
    rng = np.random.default_rng(31 + D)
    ps = eng.PlannerSet(env["E"], B, D, N, num_points=16, time_step_ns=4 * MS, **kw)
    W = rng.integers(2, 7, size=B)
    off = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    st, _ = ps.set_waypoints(rng.uniform(-2, 2, size=(int(off[-1]), D)), off, rng.uniform(1, 2, size=(B, D)),
                             rng.uniform(2, 4, size=(B, D)), 0.02)
    assert (st.numpy() == 0).all()
    return ps


def test_tensor_api(env):
    torch, eng = env["torch"], env["eng"]
    B, D, N = 6, 5, 40
    with _moving_set(env, B, D, N) as a, eng.PlannerSet(env["E"], 3, D, N, num_points=4, time_step_ns=4 * MS) as b:
        s = a.plan(1000 * MS, 300 * MS)
        assert (s["status"].numpy() == 0).all()
        info = a.state_info([4, 1])
        assert info.dtype == eng.PLANNER_STATE_INFO_DTYPE and info.shape == (2,)
        assert info["trajectory_count"].tolist() == s["num_samples"].numpy()[[4, 1]].tolist()
        blob, off = a.export_state(ids=[4, 1])
        assert blob.is_cuda and blob.dtype == torch.uint8 and not off.is_cuda and off.dtype == torch.int64
        assert off.tolist() == [0, int(info["bytes"][0]), int(info["bytes"][0] + info["bytes"][1])]
        assert blob.numel() == off[-1] <= 2 * a.state_bytes_bound
        assert a.last_export_status.is_cuda and a.last_export_status.cpu().tolist() == [0, 0]
        # into a caller's tensor, at slots of the bound
        bound = a.state_bytes_bound
        out = torch.zeros(2 * bound, dtype=torch.uint8, device=env["dev"])
        blob2, off2 = a.export_state(ids=[4, 1], out=out, offsets=[0, bound, 2 * bound])
        assert blob2.data_ptr() == out.data_ptr() and off2.tolist() == [0, bound, 2 * bound]
        torch.cuda.synchronize()
        recs = cases.split(blob, off)
        assert [bytes(out[k * bound:k * bound + len(recs[k])].cpu().numpy()) for k in range(2)] == recs
        # import: a CUDA blob through the device entry, a host blob through the host entry
        b.reserve(history=int(info["history_count"].max()), trajectory=int(info["trajectory_count"].max()))
        got = b.import_state(blob, off, ids=[2, 0])
        assert got["status"].is_cuda and got["summary"].shape == (2, 56)
        torch.cuda.synchronize()
        assert got["status"].cpu().tolist() == [cases.RESOURCE_EXHAUSTED if info["num_points"][k] > 4 else 0
                                                for k in range(2)]
        got = b.import_state(blob.cpu(), off, ids=[2, 0])
        assert not got["status"].is_cuda and got["status"].tolist() == [0, 0]
        assert got["num_samples"].tolist() == info["trajectory_count"].tolist()
        assert cases.split(*b.export_state(ids=[2, 0])) == recs
        # the sample counts follow the import: the packed download is sized from them
        t = b.download_trajectories(ids=[2, 0])
        torch.cuda.synchronize()
        assert t["offsets"].cpu().tolist() == [0, int(info["trajectory_count"][0]), int(info["trajectory_count"].sum())]
        got = b.copy_from(a, src_ids=[3], dst_ids=[1])
        assert got["status"].tolist() == [0] and cases.split(*b.export_state(ids=[1])) == cases.split(*a.export_state(ids=[3]))
        # bad input raises and changes nothing
        before = cases.split(*b.export_state())
        with pytest.raises(eng.TpamdError):
            b.import_state(blob, off, ids=[0, 0, 1])                 # offsets do not match the ids
        with pytest.raises(eng.TpamdError):
            b.import_state(blob[1:], off)                            # not 16-byte aligned
        with pytest.raises(eng.TpamdError):
            b.import_state(blob.cpu()[:100], off)                    # shorter than the offsets say
        with pytest.raises(eng.TpamdError):
            b.export_state(out=torch.zeros(16, dtype=torch.uint8, device=env["dev"]))
        with pytest.raises(eng.TpamdError):
            b.copy_from(a, src_ids=[0, 1], dst_ids=[0])
        with pytest.raises(eng.TpamdError):
            b.copy_from(a, src_ids=[0], dst_ids=[3])
        with pytest.raises(eng.TpamdError):
            a.state_info([6])
        assert cases.split(*b.export_state()) == before


def test_export_and_import_on_a_side_stream_behind_plan_async(env):
    torch, eng, dev = env["torch"], env["eng"], env["dev"]
    B, D, N = 8, 7, 33
    with _moving_set(env, B, D, N) as a, _moving_set(env, B, D, N) as ref, \
            eng.PlannerSet(env["E"], B, D, N, num_points=16, time_step_ns=4 * MS) as b:
        for ps in (a, ref, b):
            ps.reserve(history=8 * N, trajectory=4096)
        assert (a.plan(1000 * MS, 300 * MS)["status"].numpy() == 0).all()
        assert (ref.plan(1000 * MS, 300 * MS)["status"].numpy() == 0).all()
        bound = a.state_bytes_bound
        slots = np.arange(B + 1, dtype=np.int64) * bound
        out = torch.zeros(B * bound, dtype=torch.uint8, device=dev)
        start = torch.full((B,), 1100 * MS, dtype=torch.int64, device=dev)
        horizon = torch.full((B,), 300 * MS, dtype=torch.int64, device=dev)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            handle = a.plan_async(start, horizon, max_windows=3, stream=side)
            # behind the plan, without the host in between: out of a, into b
            blob, off = a.export_state(out=out, offsets=slots, stream=side)
            a_status = a.last_export_status
            got = b.import_state(blob, off, stream=side)
        side.synchronize()
        summary = handle.result()
        assert (a_status.cpu().numpy() == 0).all() and (got["status"].cpu().numpy() == 0).all()
        # the reference set does the same plan, and only then exports: the records agree
        want = ref.plan_async(start, horizon, max_windows=3).result()
        for name in ("status", "num_samples", "end_time_ns"):
            assert summary[name].tolist() == want[name].tolist(), name
        recs = cases.split(*ref.export_state())
        sizes = [len(r) for r in recs]
        assert [bytes(out[k * bound:k * bound + sizes[k]].cpu().numpy()) for k in range(B)] == recs
        assert cases.split(*b.export_state()) == recs
        # the sample counts follow the device import without a Plan: the packed download is sized from them
        tb = b.download_trajectories()
        torch.cuda.synchronize()
        assert tb["offsets"].cpu().tolist() == np.concatenate([[0], np.cumsum(summary["num_samples"].numpy())]).tolist()
        ta = a.download_trajectories()
        torch.cuda.synchronize()
        for name in ("time", "q", "qd", "qdd"):
            assert tb[name].cpu().numpy().tobytes() == ta[name].cpu().numpy().tobytes(), name
        isum = got["summary"].cpu().numpy().view(eng.PLANNER_SUMMARY_DTYPE)[:, 0]
        assert isum["num_samples"].tolist() == summary["num_samples"].tolist()
        assert isum["end_time_ns"].tolist() == summary["end_time_ns"].tolist()
        # b plans on from what it was handed, as a does
        nxt = torch.full((B,), 1200 * MS, dtype=torch.int64, device=dev)
        sa = a.plan(nxt.cpu().numpy(), 300 * MS)
        sb = b.plan(nxt.cpu().numpy(), 300 * MS)
        for name in sa:
            assert sa[name].tolist() == sb[name].tolist(), name
        assert cases.split(*a.export_state()) == cases.split(*b.export_state())

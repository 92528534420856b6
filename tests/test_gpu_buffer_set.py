"""Buffer sets on the GPU (tpamd_buffer_set_*, TrajectoryBufferSet, engine.BufferSet).
tests/cpp/test_buffer_set_gpu.cc runs random operation rounds on 256-buffer sets through the
host-pointer and the _device entries next to mirror TrajectoryBuffers (bit-equal downloads, equal
statuses), the control loop with a planner set on the structured path families of
tests/structured_paths.py (written to a file here), the in-place stop against
tpamd_planner_set_stop_trajectories, packed device outputs inserted on the device, a linear
hipGraph capture and the capacity rules. The second test drives engine.BufferSet with CUDA tensors
against the C-ABI's host-pointer entries.

Not covered here: the reference of these tests is the project's own mirror, at D = 7, 14, 1 and 6;
the fuzz's _device set holds 2048 rows and receives at most 30 a call, and the host-entry set grows
before it fills, so the in-kernel compaction (bs_move_down_wg) practically never runs; id lists
stay far below the 1024 threads of the offset scans; no difference equals the tolerance exactly.
tests/test_gpu_buffer_readout_all_dofs.py covers those: every D = 1..16 against the independent
restatement of tests/buffer_reference.py, every layout case a compaction, lists of up to 2500 ids,
capacities on and one row beside the total, ticks on and 1 ns beside the stamps."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu

MS = 1_000_000
FAMILIES = ("straight_linear", "straight_long", "idle_one", "idle_most", "near_idle", "tie_scaled", "tie_mirror",
            "tie_all", "spread_up", "spread_down", "velocity_bound", "accel_bound", "stop_interior", "stop_first",
            "stop_last", "out_and_back")


def _write_paths(path, D, N, per_family):
    import structured_paths as sp
    npts, knots, cps, vmax, amax, delta = [], [], [], [], [], []
    for name in FAMILIES:
        b = sp.make_family(name, per_family, D, N)
        P = b["control_points"].shape[1]
        npts += [P] * per_family
        knots.append(b["knots"].reshape(-1))
        cps.append(b["control_points"].reshape(-1))
        vmax.append(b["vmax"].reshape(-1))
        amax.append(b["amax"].reshape(-1))
        delta.append(b["delta"].reshape(-1))
    with open(path, "wb") as f:
        f.write(np.array([len(npts), D, N], dtype=np.int32).tobytes())
        f.write(np.array(npts, dtype=np.int32).tobytes())
        for a in (knots, cps, vmax, amax, delta):
            f.write(np.concatenate(a).astype(np.float64).tobytes())
    return len(npts)


def test_buffer_set_against_mirror(tmp_path):
    require_gpu()
    paths = str(tmp_path / "paths.bin")
    assert _write_paths(paths, 7, 300, 16) == 256
    exe = build_driver("test_buffer_set_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, paths, timeout=900, head=4000, tail=3000)
    assert out.count("fuzz vs mirror") == 3
    for part in ("planner set -> buffers", "stop in place vs stop_trajectories", "packed device outputs inserted",
                 "graph capture of insert -> discard -> sample", "TPAMD_PLAN_MORE leaves the buffer unchanged",
                 "TrajectoryBufferSet: ok"):
        assert part in out, part


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


def test_buffer_set_from_cuda_tensors():
    """engine.BufferSet (CUDA tensors, _device entries on torch's stream) next to a second set
    driven through the C-ABI's host-pointer entries: the control loop with a PlannerSet, an
    in-place stop and the readouts give the same bits."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    L = eng.load_library()
    B, D, N, step = 40, 6, 200, 4 * MS
    rng = np.random.default_rng(20261018)
    W = rng.integers(3, 7, size=B)
    offsets = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    wps = rng.uniform(-2.0, 2.0, size=(int(offsets[-1]), D))
    vmax, amax = rng.uniform(1.0, 2.0, size=(B, D)), rng.uniform(2.0, 4.0, size=(B, D))
    dev = torch.device("cuda", 0)
    E = eng.Engine(0)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p)

    def host_download(h):
        off = np.zeros(B + 1, dtype=np.int64)
        one = np.zeros(D)
        L.tpamd_buffer_set_download(h, B, None, ptr(off), 0, ptr(one), ptr(one), ptr(one), ptr(one))
        rows = int(off[-1])
        t, q, qd, qdd = np.zeros(max(rows, 1)), np.zeros((max(rows, 1), D)), np.zeros((max(rows, 1), D)), np.zeros((max(rows, 1), D))
        if rows:
            assert L.tpamd_buffer_set_download(h, B, None, ptr(off), rows, ptr(t), ptr(q), ptr(qd), ptr(qdd)) == 0
        return off, t[:rows], q[:rows], qd[:rows], qdd[:rows]

    with eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=step) as ps, \
            eng.BufferSet(E, B, D, capacity=2048) as bs, eng.BufferSet(E, B, D, capacity=8) as href:
        status, _ = ps.set_waypoints(torch.from_numpy(wps).to(dev), offsets, torch.from_numpy(vmax).to(dev),
                                     torch.from_numpy(amax).to(dev), torch.full((B,), 0.01, dtype=torch.float64, device=dev))
        assert (status.cpu() == 0).all()
        bytes_before = bs.device_bytes
        hst = np.zeros(B, dtype=np.int32)
        for r in range(3):
            now = 1000 * MS + r * 80 * MS
            start = np.full(B, now, dtype=np.int64)
            if r:
                bs.discard_before(time_ns=torch.from_numpy(start).to(dev))
                assert L.tpamd_buffer_set_discard_before(href._handle(), B, None, ptr(start), None) == 0
            ps.plan(start, np.full(B, 240 * MS, dtype=np.int64))
            st = bs.insert_from(ps)["status"]
            assert L.tpamd_buffer_set_insert_from_planner_set(href._handle(), ps._handle(), B, None, None, ptr(hst)) == 0
            assert (st.cpu().numpy() == hst).all() and (hst == 0).all()
            # the packed readout of the planner set goes into a third set without leaving the device
            tr = ps.download_trajectories()
            with eng.BufferSet(E, B, D, capacity=2048) as other:
                assert (other.insert(tr["time"], tr["q"], tr["qd"], tr["qdd"], tr["offsets"])["status"].cpu() == 0).all()
                got = other.download()
                assert _bits(got["offsets"]) == _bits(tr["offsets"]) and _bits(got["q"]) == _bits(tr["q"])
        got, (off, t, q, qd, qdd) = bs.download(), host_download(href._handle())
        assert _bits(got["offsets"]) == off.tobytes() and _bits(got["time"]) == t.tobytes()
        assert _bits(got["q"]) == q.tobytes() and _bits(got["qd"]) == qd.tobytes() and _bits(got["qdd"]) == qdd.tobytes()
        assert int(off[-1]) > B * 20
        info = bs.info(time_ns=torch.from_numpy(start + 100 * MS).to(dev))
        hseq = np.zeros(B, dtype=np.int32)
        assert L.tpamd_buffer_set_info(href._handle(), B, None, None, None, ptr(hseq), None, None, None) == 0
        assert (info["num_samples"].cpu().numpy() == np.diff(off)).all() and (info["sequence"].cpu().numpy() == hseq).all()
        assert (info["positions_up_to"].cpu() > 0).any()
        # an in-place stop, then setpoints past the new end
        when = start + 100 * MS
        am = 2.0 * amax
        sst = bs.stop_before_time(torch.from_numpy(am).to(dev), 4e-3, time_ns=torch.from_numpy(when).to(dev))["status"]
        assert L.tpamd_buffer_set_stop_before_time(href._handle(), B, None, ptr(when), None, ptr(am), C.c_double(4e-3),
                                                   ptr(hst)) == 0
        assert (sst.cpu().numpy() == hst).all() and (hst == 0).sum() > 0
        T = 80
        sp = bs.sample_at_ticks(torch.from_numpy(start).to(dev), 3 * MS, T)
        hq, hqd, hqdd = (np.full((B, T, D), np.nan) for _ in range(3))
        hts = np.zeros((B, T), dtype=np.int32)
        assert L.tpamd_buffer_set_sample_at_ticks(href._handle(), B, None, ptr(start), 3 * MS, T, ptr(hq), ptr(hqd),
                                                  ptr(hqdd), ptr(hts)) == 0
        assert sp["q"].is_cuda and _bits(sp["status"]) == hts.tobytes()
        assert _bits(sp["q"]) == hq.tobytes() and _bits(sp["qd"]) == hqd.tobytes() and _bits(sp["qdd"]) == hqdd.tobytes()
        assert (hts == 0).any() and (hts == 2).any()
        assert bs.device_bytes == bytes_before           # the _device entries never allocate
        # TPAMD_PLAN_MORE from a set that is too small, and errors of the call
        with eng.BufferSet(E, 2, D, capacity=4) as tiny:
            st = tiny.insert(torch.arange(6, dtype=torch.float64, device=dev), torch.zeros(6, D, dtype=torch.float64, device=dev),
                             torch.zeros(6, D, dtype=torch.float64, device=dev), torch.zeros(6, D, dtype=torch.float64, device=dev),
                             torch.tensor([0, 1, 6], dtype=torch.int64, device=dev))["status"]
            assert st.cpu().tolist() == [0, 100]
            tiny.reserve(16)
            assert tiny.capacity == 16 and tiny.info()["num_samples"].cpu().tolist() == [1, 0]
        with pytest.raises(eng.TpamdError):
            bs.discard_before()
        with pytest.raises(eng.TpamdError):
            eng.BufferSet(E, 4, D, timestep_tolerance=0.0)

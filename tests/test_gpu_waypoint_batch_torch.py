"""Engine.time_waypoint_paths on CUDA tensors on a stream of the caller's (8 paths, 7 joints, 128
samples at most, 1 .. 6 waypoints) against the C-ABI's host entry called through ctypes."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

B, D, N = 8, 7, 128


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), lib=eng.load_library())


def _batch():
    rng = np.random.default_rng(77)
    counts = [3, 1, 6, 2, 4, 2, 5, 3]
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return dict(waypoints=rng.uniform(-1, 1, size=(int(offsets[-1]), D)), offsets=offsets,
                vmax=rng.uniform(0.5, 2.0, size=(B, D)), amax=rng.uniform(0.5, 2.0, size=(B, D)),
                ns=np.array([128, 97, 128, 64, 65, 33, 128, 3], dtype=np.int32), rounding=np.array([0.2, 0.0] * 4),
                time_start=np.linspace(0.0, 0.7, B))


def _host_entry(env, b, ns):
    eng, lib = env["eng"], env["lib"]
    out = {k: np.zeros((B, N)) for k in ("time", "s", "sd", "sdd")}
    out.update({k: np.zeros((B, N, D)) for k in ("q", "qd", "qdd")})
    out.update(status=np.full(B, -1, dtype=np.int32), last_extremal_index=np.zeros(B, dtype=np.int32),
               num_points=np.zeros(B, dtype=np.int32), path_end=np.zeros(B), delta_used=np.zeros(B))
    p = lambda a: None if a is None else a.ctypes.data
    bt = eng._WaypointBatch(B, D, N, 0, 0.8)
    wi = eng._WaypointInputs(p(b["offsets"]), p(b["waypoints"]), p(b["rounding"]), p(b["vmax"]), p(b["amax"]), p(ns),
                             None, None, p(b["time_start"]))
    po = eng._PathOutputs(p(out["time"]), p(out["s"]), p(out["sd"]), p(out["sdd"]), p(out["q"]), p(out["qd"]),
                          p(out["qdd"]), p(out["last_extremal_index"]), None, p(out["status"]), None)
    fo = eng._WaypointFitOutputs(p(out["num_points"]), p(out["path_end"]), p(out["delta_used"]), None, None)
    assert lib.tpamd_time_waypoint_paths_host(env["E"]._h, C.byref(bt), C.byref(wi), C.byref(po), C.byref(fo)) == 0
    return out


@pytest.mark.parametrize("ragged", [False, True])
def test_torch_entry_on_a_side_stream_equals_the_host_entry(env, ragged):
    torch, dev = env["torch"], env["dev"]
    b = _batch()
    ns = b["ns"] if ragged else None
    ref = _host_entry(env, b, ns)
    assert (ref["num_points"] == [7, 4, 16, 4, 10, 4, 13, 7]).all() and (ref["status"] == 0).sum() >= 6
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        up = lambda a: torch.from_numpy(a).to(dev, non_blocking=False)
        got = env["E"].time_waypoint_paths(up(b["waypoints"]), b["offsets"], up(b["vmax"]), up(b["amax"]), N,
                                           num_samples_per_path=None if ns is None else up(ns),
                                           rounding=up(b["rounding"]), time_start=up(b["time_start"]), stream=stream)
    stream.synchronize()
    for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd"):
        g = got[k].cpu().numpy()
        for i in np.flatnonzero(ref["status"] == 0):
            n = int(ns[i]) if ragged else N
            assert g[i, :n].tobytes() == ref[k][i, :n].tobytes(), (k, i)
            assert not g[i, n:].any(), "wrote past the path's sample count"
    for k in ("status", "last_extremal_index", "num_points", "path_end", "delta_used"):
        assert got[k].cpu().numpy().tobytes() == ref[k].tobytes(), k
    np.testing.assert_array_equal(got["delta_used"].cpu().numpy(),
                                  ref["path_end"] / ((ns if ragged else np.full(B, N)) - 1))

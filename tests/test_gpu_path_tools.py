"""The path_tools batch kernels (k_stopping_points, k_project_points) on the GPU at every joint
count D = 1..16, through the _host and _device entries of Engine.compute_stopping_points and
Engine.project_points_on_paths: 70 rows (one full 64-thread group and a partly filled one) and 0
rows, bit-equal to the mirror's results for the cases of tests/cpp/test_path_tools.cc (the dump
the CPU test reads), statuses included."""
import importlib
import os

import numpy as np
import pytest

from conftest import PKG_NAME
from native_driver import run_driver
from test_path_tools_cpu import build_driver, read_dump

pytestmark = pytest.mark.gpu

ALL_DOFS = list(range(1, 17))
OK, INVALID_ARGUMENT = 0, 3


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    d = tmp_path_factory.mktemp("path_tools_gpu")
    exe = build_driver(d)
    dump = os.path.join(str(d), "cases.txt")
    run_driver(exe, dump, timeout=600, tail=3000)
    stops, projs = read_dump(dump)
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), stops=stops, projs=projs)


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


@pytest.mark.parametrize("D", ALL_DOFS)
def test_stopping_points(env, D):
    torch, E, dev = env["torch"], env["E"], env["dev"]
    cases = [c for c in env["stops"] if c["D"] == D]
    assert len(cases) == 70 and sum(c["status"] == INVALID_ARGUMENT for c in cases) == 4
    pos, vel, acc = (np.stack([c[k] for c in cases]) for k in ("pos", "vel", "acc"))
    rounding = np.array([c["rounding"] for c in cases])
    want = np.stack([c["out"] for c in cases])
    status = np.array([c["status"] for c in cases], dtype=np.int32)
    for device in (False, True):
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if device else (lambda a: a)
        point, st = E.compute_stopping_points(conv(pos), conv(vel), conv(acc), conv(rounding))
        if device:
            assert point.is_cuda and st.is_cuda
            torch.cuda.synchronize()
        point, st = _np(point), _np(st)
        assert (st == status).all(), (D, device, st, status)
        ok = status == OK
        assert point[ok].tobytes() == want[ok].tobytes(), (D, device)
        assert np.isnan(point[~ok]).all(), (D, device, "a refused row was written")
        # no rows: nothing to do, no error
        empty = conv(np.zeros((0, D)))
        point0, st0 = E.compute_stopping_points(empty, empty, empty, conv(np.zeros(0)))
        assert tuple(point0.shape) == (0, D) and tuple(st0.shape) == (0,)
    # one rounding for all rows
    same = np.full(70, 0.2)
    a, _ = E.compute_stopping_points(pos, vel, acc, 0.2)
    b, _ = E.compute_stopping_points(pos, vel, acc, same)
    assert a[status == OK].tobytes() == b[status == OK].tobytes()


@pytest.mark.parametrize("D", ALL_DOFS)
def test_projections(env, D):
    torch, E, dev = env["torch"], env["E"], env["dev"]
    cases = [c for c in env["projs"] if c["D"] == D]
    assert len(cases) == 70 and sum(c["W"] == 0 for c in cases) == 2
    offsets = np.concatenate([[0], np.cumsum([c["W"] for c in cases])]).astype(np.int32)
    wps = np.concatenate([c["wps"].reshape(-1, D) for c in cases])
    point = np.stack([c["point"] for c in cases])
    status = np.array([c["status"] for c in cases], dtype=np.int32)
    ok = status == OK
    for device in (False, True):
        conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)) if device else (lambda a: a)
        got = E.project_points_on_paths(conv(wps), offsets, conv(point))
        if device:
            assert all(v.is_cuda for v in got.values())
            torch.cuda.synchronize()
        got = {k: _np(v) for k, v in got.items()}
        assert (got["status"] == status).all(), (D, device)
        assert (got["waypoint_index"][ok] == np.array([c["index"] for c in cases])[ok]).all(), (D, device)
        for key, name in (("distance", "distance_to_path"), ("parameter", "line_parameter")):
            assert got[name][ok].tobytes() == np.array([c[key] for c in cases])[ok].tobytes(), (D, device, name)
        assert got["projected_point"][ok].tobytes() == np.stack([c["proj"] for c in cases])[ok].tobytes(), (D, device)
        # an empty list keeps its outputs
        assert (got["waypoint_index"][~ok] == -1).all() and np.isnan(got["distance_to_path"][~ok]).all()
        assert np.isnan(got["projected_point"][~ok]).all()
        # no lists
        got0 = E.project_points_on_paths(conv(np.zeros((0, D))), np.zeros(1, dtype=np.int32), conv(np.zeros((0, D))))
        assert tuple(got0["status"].shape) == (0,)

"""GetPathStopParameter on the GPU (tpamd_fastest_stop_*, tpamd_planner_set_stop_parameters):
the generic entry on solver and resampler outputs bit for bit against the Python restatement of
tests/test_fastest_stop_cpu.py, its call-level errors, and the mirror / planner-set checks of
tests/cpp/test_host_stop.cc."""
import ctypes as C
import importlib

import numpy as np
import pytest

from conftest import PKG_NAME
from native_driver import build_driver, run_driver
from test_fastest_stop_cpu import PLAN_INVALID_ARGUMENT, fastest_stop_at_time

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    return dict(torch=torch, eng=eng, syn=syn, E=eng.Engine(0), dev="cuda:0")


def _queries(rng, time, count, kind):
    """One query per row: 0 on a sample, 1 between two samples, 2 before the first sample,
    3 on the last sample, 4 after the end, 5 mixed."""
    B = time.shape[0]
    q = np.zeros(B)
    for b in range(B):
        n = int(count[b])
        t = time[b, :n]
        k = kind if kind < 5 else int(rng.integers(0, 5))
        i = int(rng.integers(0, max(n - 1, 1)))
        if n == 0:
            q[b] = 0.0
        elif k == 0:
            q[b] = t[i]
        elif k == 1:
            q[b] = 0.5 * (t[i] + t[min(i + 1, n - 1)])
        elif k == 2:
            q[b] = t[0] - 0.25
        elif k == 3:
            q[b] = t[n - 1]
        else:
            q[b] = t[n - 1] + 1e-3
    return q


def _check_rows(env, time, s, qd, qdd, amax, count, rows, tag, seed, kinds=range(6)):
    """fastest_stop on device tensors (time [B][M] ...) for every query kind, against the
    restatement on the rows listed in `rows`."""
    torch, E = env["torch"], env["E"]
    rng = np.random.default_rng(seed)
    th, sh, qdh, qddh = (x.cpu().numpy() for x in (time, s, qd, qdd))
    cnt = count.cpu().numpy() if count is not None else np.full(time.shape[0], time.shape[1], np.int32)
    amh = amax.cpu().numpy()
    mids = 0
    for kind in kinds:
        q = _queries(rng, th, cnt, kind)
        got = E.fastest_stop(time, s, qd, qdd, amax, torch.from_numpy(q).to(env["dev"]), count=count,
                             profile=True)
        torch.cuda.synchronize()
        g = {k: v.cpu().numpy() for k, v in got.items()}
        for b in rows:
            n = int(cnt[b])
            ref = fastest_stop_at_time(th[b, :n].tolist(), sh[b, :n].tolist(), qdh[b, :n].tolist(),
                                       qddh[b, :n].tolist(), amh[b].tolist(), float(q[b]))
            st, sp, idx, dur, pt, pr, pd = ref
            where = (tag, kind, b)
            assert g["status"][b] == st and g["stop_index"][b] == idx, where
            assert g["stop_parameter"][b].tobytes() == np.float64(sp).tobytes(), where
            assert g["duration"][b].tobytes() == np.float64(dur).tobytes(), where
            m = len(pt)
            for key, r in (("profile_time", pt), ("profile_rate2", pr), ("profile_drate2", pd)):
                assert g[key][b, :m].tobytes() == np.asarray(r, dtype=np.float64).tobytes(), where + (key,)
            if st != PLAN_INVALID_ARGUMENT and m > 1 and idx < n - 1:
                mids += 1
    return mids


def test_solver_outputs_uniform_batch(env):
    torch, eng, syn, E = (env[k] for k in ("torch", "eng", "syn", "E"))
    B, D, N = 96, 7, 1000
    b = syn.make_joint_batch(B, D, N)
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    ok = np.nonzero(out["status"].cpu().numpy() == 0)[0]
    assert len(ok) > B // 2
    mids = _check_rows(env, out["time"], out["s"], out["qd"], out["qdd"], inp["max_acceleration"], None,
                       ok, "uniform", 1)
    assert mids > 0


def test_solver_outputs_ragged_mixed_batch(env):
    torch, eng, syn, E = (env[k] for k in ("torch", "eng", "syn", "E"))
    dofs, samples = syn.mixed_batch_shape(72)
    groups = syn.mixed_batch_groups(dofs, samples)
    assert {k[0] for k in groups} == {6, 7, 14}
    for (D, stride), pos in groups.items():
        ns = samples[pos]
        b = syn.make_mixed_group(pos, D, ns, stride)
        inp = eng.upload_joint_batch(b, env["dev"])
        inp["num_samples_per_path"] = torch.from_numpy(ns).to(env["dev"])
        out = eng.alloc_joint_outputs(len(pos), stride, D, env["dev"])
        for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd"):
            out[k].fill_(-7.0)
        E.time_joint_paths(inp, out, stride)
        torch.cuda.synchronize()
        ok = np.nonzero(out["status"].cpu().numpy() == 0)[0]
        _check_rows(env, out["time"], out["s"], out["qd"], out["qdd"], inp["max_acceleration"],
                    inp["num_samples_per_path"], ok, "mixed D=%d" % D, D, kinds=(0, 1, 3, 5))


@pytest.mark.parametrize("skip", [False, True])
def test_resampler_outputs(env, skip):
    torch, eng, syn, E = (env[k] for k in ("torch", "eng", "syn", "E"))
    B, D, N = 48, 7, 600
    b = syn.make_joint_batch(B, D, N, first_path_index=100)
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    dt = 0.004 if skip else 0.001
    cap = N + 1 if skip else int(out["time"][:, -1].max().item() / dt) + 8
    f = dict(dtype=torch.float64, device=env["dev"])
    ro = dict(out_time=torch.zeros(B, cap, **f), out_s=torch.zeros(B, cap, **f),
              out_sd=torch.zeros(B, cap, **f), out_sdd=torch.zeros(B, cap, **f),
              out_q=torch.zeros(B, cap, D, **f), out_qd=torch.zeros(B, cap, D, **f),
              out_qdd=torch.zeros(B, cap, D, **f),
              count=torch.zeros(B, dtype=torch.int32, device=env["dev"]))
    start = torch.zeros(B, **f)
    E.resample_uniform(out, inp["max_acceleration"], start, dt, ro, skip=skip)
    torch.cuda.synchronize()
    cnt = ro["count"].cpu().numpy()
    ok = np.nonzero((out["status"].cpu().numpy() == 0) & (cnt <= cap))[0]
    assert len(ok) > B // 2
    mids = _check_rows(env, ro["out_time"], ro["out_s"], ro["out_qd"], ro["out_qdd"], inp["max_acceleration"],
                       ro["count"], ok, "resample skip=%s" % skip, 3 + skip)
    assert mids > 0


def test_host_entry_matches_device_entry(env):
    torch, eng, syn, E = (env[k] for k in ("torch", "eng", "syn", "E"))
    B, D, N = 16, 6, 400
    b = syn.make_joint_batch(B, D, N)
    inp = eng.upload_joint_batch(b, env["dev"])
    out = eng.alloc_joint_outputs(B, N, D, env["dev"])
    E.time_joint_paths(inp, out, N)
    torch.cuda.synchronize()
    q = torch.linspace(0.0, 1.0, B, dtype=torch.float64, device=env["dev"])
    cnt = torch.full((B,), N - 3, dtype=torch.int32, device=env["dev"])
    dev = E.fastest_stop(out["time"], out["s"], out["qd"], out["qdd"], inp["max_acceleration"], q, count=cnt,
                         profile=True)
    host = E.fastest_stop(*(x.cpu() for x in (out["time"], out["s"], out["qd"], out["qdd"],
                                              inp["max_acceleration"], q)), count=cnt.cpu(), profile=True,
                          host=True)
    torch.cuda.synchronize()
    for k, v in dev.items():
        assert v.cpu().numpy().tobytes() == host[k].tobytes(), k


def test_call_level_errors(env):
    torch, eng, E = env["torch"], env["eng"], env["E"]
    lib = eng.load_library()
    B, M, D = 4, 10, 3
    f = dict(dtype=torch.float64, device=env["dev"])
    t = torch.arange(B * M, **f).reshape(B, M)
    s, qd, qdd = torch.zeros(B, M, **f), torch.zeros(B, M, D, **f), torch.zeros(B, M, D, **f)
    am, q = torch.ones(B, D, **f), torch.zeros(B, **f)
    o = [torch.zeros(B, **f), torch.zeros(B, dtype=torch.int32, device=env["dev"]), torch.zeros(B, **f),
         torch.full((B,), -9, dtype=torch.int32, device=env["dev"])]
    p = lambda x: None if x is None else x.data_ptr()

    def call(num_paths=B, stride=M, dofs=D, time=t, stop=o[0], prof=(None, None, None)):
        a = eng._FastestStopArgs(num_paths, stride, dofs, 0, p(time), p(s), p(qd), p(qdd), None, p(am), p(q),
                                 p(stop), p(o[1]), p(o[2]), p(o[3]), *[p(x) for x in prof])
        return lib.tpamd_fastest_stop_device(E._h, C.byref(a), None)

    assert call() == 0
    torch.cuda.synchronize()
    assert (o[3].cpu().numpy() == 0).all()            # status written
    assert call(num_paths=0) == 0
    for bad in (dict(num_paths=-1), dict(stride=0), dict(dofs=0), dict(dofs=17), dict(time=None),
                dict(stop=None), dict(prof=(torch.zeros(B, M, **f), None, None))):
        assert call(**bad) == -1, bad                  # TPAMD_E_INVALID_ARGUMENT
    with pytest.raises(eng.TpamdError):
        E.fastest_stop(t, s, torch.zeros(B, M, 17, **f), torch.zeros(B, M, 17, **f), torch.ones(B, 17, **f), q)


def test_mirror_and_planner_set_stop_parameters(env, tmp_path):
    # the env fixture has built the engine library
    exe = build_driver("test_host_stop.cc", tmp_path, libs=("host", "engine"), prebuilt=("engine",))
    run_driver(exe, timeout=900)

"""Streaming IK tables on the GPU (tpamd_planner_set_plan_streaming / _plan_resume /
_append_ik_rows[_device], tpamd_sample_ik_target_rows_*, PlannerSet.plan_streaming).

tests/cpp/test_cartesian_stream_gpu.cc walks sets of 32 planners (N = 64; D = 5: generic rows kernel,
6 and 7: fused kernels; both sampling methods) that start from the first N rows of every IK table and
are extended only when a planner waits for rows, and holds every completed Plan against one oracle
IK-table planner per planner on the FULL table and against a whole-table set, bit for bit: with
exactly the rows asked for, with 7 rows of lookahead through the _device entry, and with one append a
row short. It also covers the final tables, the capacity growth, tpamd_planner_set_plan on a short
table, the refused calls and the dropped suspensions. The target-row sampler and the PyTorch route
are tested here."""
import importlib

import numpy as np
import pytest

import cartesian_paths as cp
import pose_fit_reference as pfr
from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu

MS = 1_000_000
TPAMD_PLAN_NEEDS_ROWS = 7


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    require_gpu()
    return build_driver("test_cartesian_stream_gpu.cc", tmp_path_factory.mktemp("stream"),
                        libs=("engine", "oracle", "hip", "m"))


def _run(exe, *args):
    return run_driver(exe, *args, timeout=300, forbid_fail=True)


@pytest.mark.parametrize("D,method", [(5, 0), (5, 1), (6, 0), (6, 1), (7, 0), (7, 1)])
def test_streaming_sets_against_oracle_planners_and_whole_table_sets(driver, D, method):
    """Tests 1-4 and 7 of the driver for one family: exact need, lookahead, one append a row short."""
    out = _run(driver, "walk", D, method)
    for name in ("exact", "ahead", "short"):
        assert out.count("%s: D %d" % (name, D)) == 1, name
    assert "32 at the end" in out and "NO planner ends with fewer rows" not in out


def test_plan_on_a_short_table_still_fails_that_planner_alone(driver):
    assert "plan on a short table: TPAMD_PLAN_INTERNAL at Plan" in _run(driver, "plan")


def test_refused_calls_and_dropped_suspensions(driver):
    out = _run(driver, "refusals")
    assert "streaming entries on a joint set: refused, plans unchanged" in out
    assert "suspension dropped by reset and by upload: 3 of 3 Plans equal to a fresh set" in out


def test_streaming_mirror_with_a_split_dependent_ik(tmp_path):
    """tests/cpp/test_cartesian_stream_mirror_gpu.cc: SetCartesianPaths(streaming) + PlanStreaming with
    an IK seeded by the previous row equals one mirror PathTimingTrajectory per planner planning window
    by window, bit for bit; the whole-table set built with the same callback differs."""
    require_gpu()
    out = _run(build_driver("test_cartesian_stream_mirror_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m")))
    assert out.count("streaming mirror family (") == 2 and "PlanStreaming on a joint set: refused" in out


def test_streaming_mirror_through_the_device_chain(tmp_path):
    """tests/cpp/test_cartesian_stream_waypoint_gpu.cc: SetCartesianWaypointPaths(..., ik, streaming) +
    PlanStreaming (device targets for the missing rows, a device IK that receives the seed row, the
    _device append) against the non-streaming SetCartesianWaypointPaths set, bit for bit to the target."""
    require_gpu()
    out = _run(build_driver("test_cartesian_stream_waypoint_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m")))
    assert out.count("waypoint streaming D") == 2 and out.count("6 at the end") == 2
    assert out.count("the planner's splines are forgotten") == 2


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0))


def test_target_rows_equal_the_rows_of_a_whole_path_sampling(env):
    """tpamd_sample_ik_target_rows_* with random first rows against the same rows of
    tpamd_sample_ik_targets_*, bit for bit, _device and _host: edge splines of 3 and 16 control
    points and a path of 2000 control points; rows on both sides of knots.back() - delta."""
    torch, dev, E = env["torch"], env["dev"], env["E"]
    rng = np.random.default_rng(81)
    D = 7
    paths = []
    for P, N in ((3, 80), (16, 400)):
        e = cp.pose_edge_paths(P, N)
        for b in range(min(e["knots"].shape[0], 4)):
            paths.append(dict(P=P, rows=N, knots=e["knots"][b], tr=e["translation"][b], rot=e["rotation"][b],
                              delta=float(e["delta"][b]), jcp=rng.uniform(-2.0, 2.0, (P, D))))
    P, rows = 2000, 2100
    kn = np.concatenate([[0.0, 0.0], np.arange(P - 1, dtype=float), [P - 2.0, P - 2.0]])
    rot = rng.standard_normal((P, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    paths.append(dict(P=P, rows=rows, knots=kn, tr=rng.uniform(-1, 1, (P, 3)), rot=rot, delta=kn[-1] / (rows - 30),
                      jcp=rng.uniform(-2, 2, (P, D))))
    fit = dict(knots=np.concatenate([p["knots"] for p in paths]),
               translation_points=np.concatenate([p["tr"] for p in paths]),
               rotation_points=np.concatenate([p["rot"] for p in paths]),
               joint_control_points=np.concatenate([p["jcp"] for p in paths]),
               num_points=np.array([p["P"] for p in paths], dtype=np.int32), point_offsets=None)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    dfit = {k: (up(v) if k not in ("num_points", "point_offsets") else v) for k, v in fit.items()}
    delta = np.array([p["delta"] for p in paths])
    # every path's table reaches past knots.back(): rows below and from knots.back() - delta on
    full = np.array([p["rows"] + 40 for p in paths])
    full_off = np.concatenate([[0], np.cumsum(full)]).astype(np.int32)
    pose_w, joint_w = E.sample_ik_targets(dfit, up(delta), full_off)
    torch.cuda.synchronize()
    pose_w, joint_w = pose_w.cpu().numpy(), joint_w.cpu().numpy()
    below = above = 0
    for trial in range(4):
        first = np.array([int(rng.integers(0, f - 1)) for f in full], dtype=np.int32)
        if trial == 0:
            first[:] = 0
        if trial == 1:       # windows that straddle the padding edge
            first = np.array([max(int((p["knots"][-1] - p["delta"]) / p["delta"]) - 3, 0) for p in paths], dtype=np.int32)
        cnt = np.array([int(rng.integers(1, f - a + 1)) for f, a in zip(full, first)])
        if trial == 1:
            cnt = np.minimum(full - first, 12)
        off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
        pose_d, joint_d = E.sample_ik_targets(dfit, up(delta), off, first_row=first)
        torch.cuda.synchronize()
        pose_h, joint_h = E.sample_ik_targets(fit, delta, off, first_row=first)
        assert _bits(pose_d) == _bits(pose_h) and _bits(joint_d) == _bits(joint_h), trial
        for k, p in enumerate(paths):
            w = slice(int(full_off[k] + first[k]), int(full_off[k] + first[k] + cnt[k]))
            r = slice(int(off[k]), int(off[k + 1]))
            assert _bits(pose_h[r]) == _bits(pose_w[w]) and _bits(joint_h[r]) == _bits(joint_w[w]), (trial, k)
            par = (first[k] + np.arange(cnt[k])) * p["delta"]
            below += int((par < p["knots"][-1] - p["delta"]).sum())
            above += int((par >= p["knots"][-1] - p["delta"]).sum())
    assert below >= 3 * len(paths) and above >= 8 * len(paths)      # what the straddling trial alone guarantees
    eng = env["eng"]
    with pytest.raises(eng.TpamdError):       # a negative first row is a call-level error
        E.sample_ik_targets(fit, delta, full_off, first_row=-np.ones(len(paths), dtype=np.int32))


@pytest.mark.parametrize("D,method,lookahead", [(6, 0, 0), (7, 1, 5)])
def test_planner_set_plan_streaming_from_cuda_tensors(env, D, method, lookahead):
    """PlannerSet.set_pose_waypoints(streaming=True) + plan_streaming with an IK that returns the joint
    targets against the non-streaming set_pose_waypoints set: every Plan's summary and packed
    trajectories, bit for bit, up to target_reached; the PCIe bytes of every call."""
    torch, dev, E, eng = env["torch"], env["dev"], env["E"], env["eng"]
    B, N = 6, 64
    rng = np.random.default_rng(900 + D)
    goals = [pfr.make_case("random", 3 + b % 3, D, rng) for b in range(B)]
    vmax, amax = rng.uniform(0.6, 1.1, (B, D)), rng.uniform(1.5, 3.0, (B, D))
    vt, vr = rng.uniform(0.4, 0.6, B), rng.uniform(0.8, 1.2, B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = torch.arange(6, device=dev, dtype=torch.float64)[None, :, None]
    d = torch.arange(D, device=dev, dtype=torch.float64)[None, None, :]
    seeds = []

    def ik(pose_targets, joint_targets, row_offsets, seed_rows=None):
        assert pose_targets.is_cuda and joint_targets.is_cuda and pose_targets.shape == (row_offsets[-1], 7)
        if seed_rows is not None:
            assert seed_rows.is_cuda and seed_rows.shape == (len(row_offsets) - 1, D)
            seeds.append((seed_rows.clone(), joint_targets[torch.as_tensor(row_offsets[:-1].astype(np.int64), device=dev)]))
        q = joint_targets.clone()
        J = (0.2 * torch.sin(q[:, None, :] * (c + 1.0) + 0.31 * d) + (c == d)).contiguous()
        return q, J

    off = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in goals])]).astype(np.int32)
    pose, joints = up(np.concatenate([g[0] for g in goals])), up(np.concatenate([g[1] for g in goals]))
    kw = dict(time_step_ns=4 * MS, sampling_method=method, max_planning_iterations=10000,
              max_initial_velocity_error=1e-3, cartesian=True)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as whole, \
            eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as stream:
        # delta: a fraction of every path's length, as in tests/test_gpu_cartesian_set.py
        fit = E.fit_pose_waypoints(pose, joints, off, up(np.full(B, 0.05)), up(np.full(B, 0.2)))
        path_end = fit["path_end"].cpu().numpy()
        delta = np.where(np.arange(B) % 2, 0.25, 0.4) * path_end / (N - 1)
        args = (up(vmax), up(amax), up(vt), up(vr), up(delta))
        st_w, rows_w = whole.set_pose_waypoints(pose, joints, off, ik, *args)
        st_s, rows_s = stream.set_pose_waypoints(pose, joints, off, ik, *args, streaming=True)
        assert (st_w == 0).all() and (st_s == 0).all() and (rows_s == N).all() and (rows_w > 2 * N).all()
        for b in range(B):
            assert stream.download_ik_table(b)[0].shape[0] == N
        start = np.zeros(B, dtype=np.int64)
        suspensions = steps = 0
        done = np.zeros(B, dtype=bool)
        while steps < 300:
            sw = whole.plan(start, 750 * MS)
            up_w, down_w = whole.last_plan_bytes()
            ss, need_first, need_count = stream.plan_streaming(start, 750 * MS, ik, lookahead_rows=lookahead)
            assert not need_first.any() and not need_count.any()
            stats = stream.last_stream_stats
            suspensions += stats["suspensions"]
            for name in sw:
                assert _bits(sw[name]) == _bits(ss[name]), (steps, name)
            assert (ss["status"] == 0).all()
            tw, ts = whole.download_trajectories(), stream.download_trajectories()
            torch.cuda.synchronize()
            for name in tw:
                assert _bits(tw[name]) == _bits(ts[name]), (steps, name)
            # a streaming Plan moves what Plan moves upwards and at most 8 B per planner more downwards
            # per call of the chain; a resume moves nothing upwards
            assert stats["h2d"][0] == up_w == 24 * B and all(x == 0 for x in stats["h2d"][1:])
            assert stats["d2h"][0] <= down_w + 8 * B
            windows = int(sw["windows"].max())
            for x in stats["d2h"][1:]:
                assert x <= 56 * B + 8 * (windows + 2) + 8 + 8 * B
            steps += 1
            done = sw["target_reached"].numpy() != 0
            if done.all():
                break
            start = np.where(done, start, np.minimum(sw["end_time_ns"].numpy(), start + 200 * MS))
        assert done.all() and suspensions >= B
        # every extension was seeded with the last resident row, which the IK reproduced as its first row
        assert seeds and all(_bits(a) == _bits(b) for a, b in seeds)
        # the streamed tables are a prefix of the whole ones and shorter than them
        for b in range(B):
            qs, Js = stream.download_ik_table(b)
            qw, Jw = whole.download_ik_table(b)
            assert N < qs.shape[0] < qw.shape[0] == int(rows_w[b])
            assert _bits(qs) == _bits(qw[:qs.shape[0]]) and _bits(Js) == _bits(Jw[:qs.shape[0]]), b
        with pytest.raises(eng.TpamdError):
            stream.plan_resume()                       # nobody waits
    with eng.PlannerSet(E, 2, D, N, time_step_ns=4 * MS) as joint_set:
        with pytest.raises(eng.TpamdError):
            joint_set.plan_streaming(0, 750 * MS)
        with pytest.raises(eng.TpamdError):
            joint_set.append_ik_rows(np.zeros((1, D)), np.zeros((1, 6, D)), np.array([0, 1], dtype=np.int32), ids=[0])

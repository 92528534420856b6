"""Discarding consumed IK rows on the GPU (tpamd_planner_set_discard_ik_rows / _ik_table_info /
_download_ik_rows, PathTimingTrajectorySet::DiscardIkRows, PlannerSet.discard_ik_rows).

tests/cpp/test_cartesian_discard_gpu.cc holds the compaction kernel against the uploaded tables and
walks streaming sets of 32 planners (N = 64; D = 5, 6, 7; both sampling methods; paths of at least 8
windows) that discard after every Plan -- and, in a third walk, while planners wait for rows -- against
one oracle IK-table planner per planner on the FULL table and against a streaming twin that never
discards, bit for bit at every Plan. It also covers the appends that must not reallocate, a keep_from
above the floor, and the refused calls. The mirror and the PyTorch route are tested here."""
import importlib

import numpy as np
import pytest

import pose_fit_reference as pfr
from conftest import PKG_NAME
from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu

MS = 1_000_000


def _build(tmp, name, host_mirror):
    require_gpu()
    return build_driver(name + ".cc", tmp, libs=("host" if host_mirror else "oracle", "engine", "hip", "m"), flags=("-w",))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("discard"), "test_cartesian_discard_gpu", host_mirror=False)


def _run(exe, *args):
    return run_driver(exe, *args, timeout=300, forbid_fail=True)


@pytest.mark.parametrize("D", [5, 6, 7])
def test_compaction_keeps_the_live_rows_bit_for_bit(driver, D):
    """Test 1 of the driver: mixed tables, the six keep_from choices, accumulation, appends, growth."""
    out = _run(driver, "compact", D)
    assert "compaction D %d: 160 of 160 live-row readouts equal the uploaded slices" % D in out
    if D == 7:
        assert "4 overlapping 333-row shifts by 1" in out


@pytest.mark.parametrize("D,method", [(5, 0), (5, 1), (6, 0), (6, 1), (7, 0), (7, 1)])
def test_walk_with_discards_against_oracle_planners_and_a_twin(driver, D, method):
    """Tests 2 and 4 of the driver for one family: a discard after every Plan with exact-need appends,
    with 7 rows of lookahead through the _device append, and with a discard while planners wait."""
    out = _run(driver, "walk", D, method)
    for name in ("exact", "ahead", "waiting"):
        assert out.count("%s: D %d" % (name, D)) == 1, name
    assert out.count("32 of 32 planners with first_row > 0, 32 at the end") == 3


def test_append_after_a_discard_does_not_reallocate(driver):
    assert "no reallocation: the fitting appends kept the table, the next one grew it to 256 rows" in _run(driver, "norealloc")


def test_keep_from_above_the_floor_fails_that_planner_alone(driver):
    out = _run(driver, "above")
    assert "keep_from above the floor: TPAMD_PLAN_INTERNAL for that planner, all neighbour Plans" in out
    assert "plans again after a fresh upload" in out


def test_refused_discards_change_nothing(driver):
    out = _run(driver, "refusals")
    assert "refused discards: tables unchanged" in out
    assert "download_ik_table on a discarded planner: error and the total row count" in out


def test_mirror_plan_streaming_with_the_discard_flag(tmp_path):
    """tests/cpp/test_cartesian_discard_mirror_gpu.cc: PlanStreaming with the discard flag equals
    PlanStreaming without it (and one mirror PathTimingTrajectory per planner), bit for bit."""
    exe = _build(tmp_path, "test_cartesian_discard_mirror_gpu", host_mirror=True)
    out = _run(exe)
    assert out.count("discard mirror family (") == 2 and "DiscardIkRows on a joint set: refused" in out


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


@pytest.mark.parametrize("D,method", [(6, 0), (7, 1)])
def test_planner_set_plan_streaming_with_discard_from_cuda_tensors(env, D, method):
    """PlannerSet.plan_streaming(..., discard=True) against the non-streaming set_pose_waypoints set:
    every Plan's summary and packed trajectories, bit for bit, up to target_reached; ik_table_info
    shows first_row advancing; the discard moves 4 B per planner each way and the Plan's own bytes
    are those of a streaming Plan without it."""
    torch, dev, E, eng = env["torch"], env["dev"], env["E"], env["eng"]
    B, N = 6, 64
    rng = np.random.default_rng(900 + D)
    goals = [pfr.make_case("random", 3 + b % 3, D, rng) for b in range(B)]
    vmax, amax = rng.uniform(0.6, 1.1, (B, D)), rng.uniform(1.5, 3.0, (B, D))
    vt, vr = rng.uniform(0.4, 0.6, B), rng.uniform(0.8, 1.2, B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    c = torch.arange(6, device=dev, dtype=torch.float64)[None, :, None]
    d = torch.arange(D, device=dev, dtype=torch.float64)[None, None, :]

    def ik(pose_targets, joint_targets, row_offsets, seed_rows=None):
        q = joint_targets.clone()
        J = (0.2 * torch.sin(q[:, None, :] * (c + 1.0) + 0.31 * d) + (c == d)).contiguous()
        return q, J

    off = np.concatenate([[0], np.cumsum([g[0].shape[0] for g in goals])]).astype(np.int32)
    pose, joints = up(np.concatenate([g[0] for g in goals])), up(np.concatenate([g[1] for g in goals]))
    kw = dict(time_step_ns=4 * MS, sampling_method=method, max_planning_iterations=10000,
              max_initial_velocity_error=1e-3, cartesian=True)
    with eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as whole, \
            eng.PlannerSet(E, B, D, N, table_capacity=N, **kw) as stream:
        fit = E.fit_pose_waypoints(pose, joints, off, up(np.full(B, 0.05)), up(np.full(B, 0.2)))
        path_end = fit["path_end"].cpu().numpy()
        delta = np.where(np.arange(B) % 2, 0.25, 0.4) * path_end / (N - 1)
        args = (up(vmax), up(amax), up(vt), up(vr), up(delta))
        st_w, rows_w = whole.set_pose_waypoints(pose, joints, off, ik, *args)
        st_s, rows_s = stream.set_pose_waypoints(pose, joints, off, ik, *args, streaming=True)
        assert (st_w == 0).all() and (st_s == 0).all() and (rows_s == N).all()
        assert all(stream.ik_table_info(b) == (0, N, N) for b in range(B))
        start = np.zeros(B, dtype=np.int64)
        first = np.zeros(B, dtype=np.int64)
        steps = advanced = 0
        done = np.zeros(B, dtype=bool)
        while steps < 300:
            sw = whole.plan(start, 750 * MS)
            up_w, down_w = whole.last_plan_bytes()
            ss, need_first, need_count = stream.plan_streaming(start, 750 * MS, ik, discard=True)
            assert not need_first.any() and not need_count.any()
            stats = stream.last_stream_stats
            for name in sw:
                assert _bits(sw[name]) == _bits(ss[name]), (steps, name)
            tw, ts = whole.download_trajectories(), stream.download_trajectories()
            torch.cuda.synchronize()
            for name in tw:
                assert _bits(tw[name]) == _bits(ts[name]), (steps, name)
            # the Plan moves what a streaming Plan moves; the discard 4 B per planner up (the ids) and down
            assert stats["h2d"][0] == up_w == 24 * B and all(x == 0 for x in stats["h2d"][1:])
            assert stats["d2h"][0] <= down_w + 8 * B
            assert stats["discard_h2d"] == 4 * B and stats["discard_d2h"] == 4 * B
            info = [stream.ik_table_info(b) for b in range(B)]
            now = np.array([i[0] for i in info])
            assert (now == stats["first_row"]).all() and (now >= first).all()
            assert all(i[0] <= i[1] - 1 for i in info)
            advanced += int((now > first).sum())
            first = now
            steps += 1
            done = sw["target_reached"].numpy() != 0
            if done.all():
                break
            start = np.where(done, start, np.minimum(sw["end_time_ns"].numpy(), start + 200 * MS))
        assert done.all() and (first > 0).all() and advanced >= 2 * B
        # the live rows are the same path rows of the whole table; the rows from 0 are gone
        for b in range(B):
            f, qs, Js = stream.download_ik_rows(b)
            qw, Jw = whole.download_ik_table(b)
            assert f == first[b] and f + qs.shape[0] == stream.ik_table_info(b)[1] <= qw.shape[0]
            assert _bits(qs) == _bits(qw[f:f + qs.shape[0]]) and _bits(Js) == _bits(Jw[f:f + qs.shape[0]]), b
            with pytest.raises(eng.TpamdError):
                stream.download_ik_table(b)
        # an explicit discard: one planner, clamped to its last row
        last = stream.ik_table_info(2)[1] - 1
        assert stream.discard_ik_rows(keep_from=[last + 50], ids=[2]).tolist() == [last]
        assert stream.download_ik_rows(2)[1].shape[0] == 1
    with eng.PlannerSet(E, 2, D, N, time_step_ns=4 * MS) as joint_set:
        with pytest.raises(eng.TpamdError):
            joint_set.discard_ik_rows()
        with pytest.raises(eng.TpamdError):
            joint_set.ik_table_info(0)

"""Planner-set Plan at every joint count against the oracle's planner, through the replan programs
of plan_cases.py (what they contain is asserted on the oracle alone by test_plan_cases_cpu.py):
B = 12 planners, windows of 33 / 64 / 65 samples, up to 80 Plans with erase-only, one-, two- and
many-window Plans, every status, resets and new paths after every failure.

After every Plan of a set (host entries, numpy arrays) each planner is compared with its tpo.Planner:
the status always; for status 0 the summary fields and the trajectory arrays bit for bit, and the
invariants of plan_cases.check_invariants on the set's own arrays.

  sync        plan() on a set with default capacities and on one with history 2 N / trajectory 64
              (both buffers must grow, several times), then the DEADLINE_EXCEEDED run on a set with
              max_planning_iterations = 1
  async       plan_async() with max_windows 1, 2, 4 against oracle planners with
              max_planning_iterations = max_windows - 1, after reserve() from the oracle's own largest
              history and trajectory: no planner may run out of room
  exhausted   plan_async() at the tight capacities without reserve(): see the test
"""
import importlib

import numpy as np
import pytest

import plan_cases as pc
from conftest import PKG_NAME

pytestmark = pytest.mark.gpu

FIELDS = (("num_samples", "num_samples"), ("end_time_ns", "end_time"), ("final_decel_start_ns", "final_decel_start"),
          ("target_reached", "target_reached"), ("windows", "windows"), ("path_state", "path_state"),
          ("history_count", "history_count"))
ARRAYS = (("time", "time"), ("s", "path_parameter"), ("q", "positions"), ("qd", "velocities"), ("qdd", "accelerations"))
RESOURCE_EXHAUSTED = 8


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    from oracle import tpo
    tpo.build()
    eng = importlib.import_module(PKG_NAME + ".engine")
    E = eng.Engine(0)
    yield dict(tpo=tpo, eng=eng, E=E, torch=torch)
    E.close()


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


class Follower:
    """One PlannerSet driven through a program's steps and compared with the program's oracle planners."""

    def __init__(self, env, program, tight=False, **kw):
        self.env, self.program, self.N = env, program, program.N
        if tight:
            kw.update(history_capacity=2 * self.N, trajectory_capacity=pc.TIGHT_TRAJECTORY)
        self.ps = env["eng"].PlannerSet(env["E"], pc.B, program.D, self.N, time_step_ns=pc.TIME_STEP_NS,
                                        sampling_method=program.method, max_planning_iterations=program.max_iterations,
                                        constraint_safety=pc.SAFETY, max_initial_velocity_error=pc.MAX_INITIAL_VELOCITY_ERROR,
                                        cartesian=(program.kind == "cartesian"), **kw)
        self.paths = [None] * pc.B
        self.capacity = self.ps.capacity()
        self.history_growths = self.trajectory_growths = self.compared = 0

    def close(self):
        self.ps.close()

    def new_paths(self, new):
        """reset, then the new paths, for the planners a step lists"""
        if not new:
            return
        ids = np.array(sorted(new), dtype=np.int32)
        paths = [new[int(b)] for b in ids]
        for b, p in zip(ids, paths):
            self.paths[int(b)] = p
        self.ps.reset(ids)
        common = dict(initial_velocity=np.stack([p["initial_velocity"] for p in paths]), ids=ids,
                      path_state=np.array([p["state"] for p in paths], dtype=np.int32))
        vmax, amax = np.stack([p["vmax"] for p in paths]), np.stack([p["amax"] for p in paths])
        delta = np.array([p["delta"] for p in paths])
        if self.program.kind == "joint":
            self.ps.set_paths(np.concatenate([p["knots"] for p in paths]),
                              np.concatenate([p["control_points"].reshape(-1) for p in paths]),
                              np.array([p["control_points"].shape[0] for p in paths], dtype=np.int32), vmax, amax, delta,
                              **common)
        else:
            rows = np.concatenate([[0], np.cumsum([p["ik_positions"].shape[0] for p in paths])]).astype(np.int32)
            self.ps.set_ik_tables(np.concatenate([p["ik_positions"] for p in paths]),
                                  np.concatenate([p["jacobians"] for p in paths]), rows,
                                  np.array([p["path_end"] for p in paths]), vmax, amax,
                                  np.array([p["vtrans"] for p in paths]), np.array([p["vrot"] for p in paths]), delta,
                                  **common)

    def plan(self, step, max_windows=None, start=None, horizon=None):
        """The step's Plan: plan(), or plan_async() with max_windows. Returns the summary (numpy)."""
        start = step.start if start is None else start
        horizon = step.horizon if horizon is None else horizon
        if max_windows is None:
            summary = self.ps.plan(start, horizon)
        else:
            torch = self.env["torch"]
            dev = torch.device("cuda", 0)
            summary = self.ps.plan_async(torch.from_numpy(start).to(dev), torch.from_numpy(horizon).to(dev),
                                         max_windows=max_windows).result()
        cap = self.ps.capacity()
        self.history_growths += cap[0] > self.capacity[0]
        self.trajectory_growths += cap[1] > self.capacity[1]
        self.capacity = cap
        return {k: (v if k == "info" else v.numpy()) for k, v in summary.items()}

    def compare(self, step, summary, planners=range(pc.B)):
        traj = {k: (v.cpu().numpy() if v is not None else None) for k, v in self.ps.download_trajectories().items()}
        off = traj["offsets"]
        for b in planners:
            o, where = step.oracle[b], (self.program.kind, self.program.D, self.program.method, step.index, b,
                                        step.lives[b], step.edges[b])
            assert int(summary["status"][b]) == int(step.rc[b]), (where, int(summary["status"][b]), int(step.rc[b]))
            if step.rc[b] != 0:
                continue
            for field, attr in FIELDS:
                assert int(summary[field][b]) == int(getattr(o, attr)), (where, field, int(summary[field][b]), getattr(o, attr))
            r = slice(int(off[b]), int(off[b + 1]))
            assert r.stop - r.start == o.num_samples, where
            for key, attr in ARRAYS:
                assert _bits(traj[key][r]) == _bits(getattr(o, attr)), (where, key)
            if o.num_samples:
                pc.check_invariants(traj["time"][r], traj["s"][r], traj["qdd"][r], np.asarray(self.paths[b]["amax"]),
                                    pc.path_end_of(self.paths[b], self.N), self.program.kind, self.program.method, where)
                if o.target_reached:
                    assert (traj["qd"][r][-1] == 0).all(), where
            self.compared += 1


def run(follower, max_windows=None):
    """The whole program on one set. Returns the program's Stats."""
    stats = pc.Stats(follower.N)
    for step in follower.program.steps():
        follower.new_paths(step.new_paths)
        summary = follower.plan(step, max_windows)
        follower.compare(step, summary)
        stats.add(step)
    return stats


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("D", pc.ALL_DOFS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_sync_plan_equals_the_oracle(env, kind, D, method):
    tpo = env["tpo"]
    program = pc.Program(tpo, kind, D, method)
    default, tight = Follower(env, program), Follower(env, program, tight=True)
    try:
        stats = pc.Stats(program.N)
        for step in program.steps():
            for f in (default, tight):
                f.new_paths(step.new_paths)
                f.compare(step, f.plan(step))
            stats.add(step)
        assert default.compared == tight.compared == stats.ok >= 10 * pc.B
        # both buffers of the tight set grew (the history doubles, so 2 N -> more than the largest history)
        assert tight.capacity[0] >= stats.max_history > 2 * program.N and tight.capacity[1] >= stats.max_samples
        assert tight.history_growths >= 1 and tight.trajectory_growths >= 1
        print(kind, D, method, "N", program.N, stats.line(), "| growths (history, trajectory): default",
              (default.history_growths, default.trajectory_growths), "tight", (tight.history_growths, tight.trajectory_growths))
    finally:
        default.close()
        tight.close()
    # DEADLINE_EXCEEDED: a set and oracle planners with max_planning_iterations = 1
    late = Follower(env, pc.Program(tpo, kind, D, method, max_iterations=1, max_steps=pc.DEADLINE_STEPS))
    try:
        stats = run(late)
        assert stats.status[5] >= 1
        print(kind, D, method, "max_planning_iterations 1:", stats.line())
    finally:
        late.close()


# joint sets with max_windows 1, 2 and 4, Cartesian sets with 4
ASYNC_CASES = [(kind, D, method, w) for kind in pc.KINDS for D in pc.ALL_DOFS for method in (0, 1)
               for w in ((1, 2, 4) if kind == "joint" else (4,))]


@pytest.mark.parametrize("kind,D,method,max_windows", ASYNC_CASES)
def test_async_plan_equals_the_oracle(env, kind, D, method, max_windows):
    tpo = env["tpo"]
    iterations = min(200, max_windows - 1)
    # what reserve() needs, from the oracle's own run: the gate wants room for one more window on top
    # of the history a planner has, and no history exceeds the largest one a Plan left
    ahead = pc.Stats(pc.window_samples(D, method))
    for step in pc.Program(tpo, kind, D, method, max_iterations=iterations).steps():
        ahead.add(step)
    follower = Follower(env, pc.Program(tpo, kind, D, method, max_iterations=iterations))
    try:
        follower.ps.reserve(ahead.max_history + follower.N, max(ahead.max_samples, 1))
        reserved = follower.ps.capacity()
        stats = pc.Stats(follower.N)
        for step in follower.program.steps():
            follower.new_paths(step.new_paths)
            summary = follower.plan(step, max_windows)
            assert summary["info"]["num_exhausted"] == 0 and (summary["status"] != RESOURCE_EXHAUSTED).all()
            assert summary["info"]["num_ok"] == int((step.rc == 0).sum())
            follower.compare(step, summary)
            stats.add(step)
        assert follower.ps.capacity() == reserved
        assert follower.compared == stats.ok
        if max_windows == 4:
            assert stats.ok >= 10 * pc.B and stats.multi_window >= 1
        else:
            assert stats.status[5] >= 1
        print(kind, D, method, "max_windows", max_windows, stats.line())
    finally:
        follower.close()


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("D", pc.ALL_DOFS)
def test_async_plan_without_room(env, D, method):
    """plan_async at history 2 N / trajectory 64 without reserve(), max_windows 4, against the oracle
    with max_planning_iterations 3. A planner may end with RESOURCE_EXHAUSTED, and only for a reason
    the oracle's own counts give:
      * its trajectory does not fit: it went through all its windows (windows and history_count equal
        the oracle's), the oracle's trajectory is longer than the capacity, its trajectory is empty, and
        info.needed_trajectory is at least the oracle's count. Its next Plan (at the same start: its
        end time is its start time now) fails its precondition; then it is reset.
      * its history has no room for one more window: the gate stops it where count + N exceeds the
        capacity, and the counts a planner goes through lie between the one it had and the one the
        oracle ends with, so the larger of the two plus N exceeds the capacity; info.needed_history
        exceeds the capacity. Its trajectory is not empty: such a planner is neither resampled nor
        finished (include/tpamd.h), so it keeps the old trajectory as Plan's prologue cut it, the
        samples up to the start (GetTimeOffsetAfter), none on a new path. The count is asserted from
        the oracle's trajectory of the step before. It is reset at once.
    Every other planner equals the oracle as in the other tests. The program is told about each
    reset (force_reset), so the oracle planner starts afresh with the set's.
    With uniform sampling 64 samples are 256 ms, less than the first window of any of these paths
    takes, so there nearly every Plan that resamples is exhausted and the planners in step with the
    oracle are mostly the ones whose Plan fails alike: the count of successful Plans compared bit for
    bit is asserted (at least B) with skip sampling only, where trajectories of 64 samples are common.
    With skip sampling and N = 33 (D = 2, 5, 8, 11, 14) a trajectory holds at most one sample per
    history sample and the start, and the history capacity is 66, so no trajectory need run out
    there; each of those D has its trajectory exhaustion, and the refused Plan after it, in its
    uniform case (N = 65), where they are required like everywhere else."""
    tpo, max_windows = env["tpo"], 4
    follower = Follower(env, pc.Program(tpo, "joint", D, method, max_iterations=max_windows - 1), tight=True)
    N, ps = follower.N, follower.ps
    try:
        cap = ps.capacity()
        assert cap == (2 * N, pc.TIGHT_TRAJECTORY)
        before = np.zeros(pc.B, dtype=np.int64)        # the oracle's history counts before the step
        lost = {}                                       # planner -> (start, horizon) of the Plan that exhausted it
        old_time = [np.zeros(0)] * pc.B                 # the oracle's trajectory stamps before the step
        by_trajectory = by_history = refused = 0
        stats = pc.Stats(N)
        for step in follower.program.steps():
            follower.new_paths(step.new_paths)
            for b in step.new_paths:
                before[b] = 0
                old_time[b] = np.zeros(0)
            lost = {b: v for b, v in lost.items() if b not in step.new_paths}     # its life ended by itself
            start, horizon = step.start.copy(), step.horizon.copy()
            for b, (s, h) in lost.items():
                start[b], horizon[b] = s, h
            summary = follower.plan(step, max_windows, start, horizon)
            status = summary["status"]
            for b in lost:
                assert int(status[b]) == 1, (D, step.index, b, int(status[b]))
                follower.program.force_reset(b)
                refused += 1
            exhausted = [b for b in range(pc.B) if b not in lost and int(status[b]) == RESOURCE_EXHAUSTED]
            in_sync = [b for b in range(pc.B) if b not in lost and b not in exhausted]
            lost = {}
            needed_trajectory = 0
            for b in exhausted:
                o, where = step.oracle[b], (D, step.index, b, step.lives[b])
                if (int(summary["history_count"][b]) == o.history_count and int(summary["windows"][b]) == o.windows
                        and step.rc[b] == 0 and o.num_samples > cap[1]):
                    assert int(summary["num_samples"][b]) == 0, where
                    needed_trajectory = max(needed_trajectory, o.num_samples)
                    lost[b] = (int(step.start[b]), int(step.horizon[b]))
                    by_trajectory += 1
                else:
                    assert max(int(before[b]), o.history_count) + N > cap[0], (where, int(before[b]), o.history_count)
                    assert summary["info"]["needed_history"] > cap[0], where
                    kept = int((old_time[b] <= int(step.start[b]) / 1e9).sum())
                    assert int(summary["num_samples"][b]) == kept, (where, int(summary["num_samples"][b]), kept)
                    follower.program.force_reset(b)
                    by_history += 1
            info = summary["info"]
            assert info["num_exhausted"] == len(exhausted) and info["needed_trajectory"] >= needed_trajectory
            if not exhausted:
                assert info["needed_history"] == 0 and info["needed_trajectory"] == 0
            follower.compare(step, summary, in_sync)
            stats.add(step, in_sync)
            before = np.array([o.history_count for o in step.oracle], dtype=np.int64)
            old_time = [o.time for o in step.oracle]
        assert ps.capacity() == cap
        assert by_history >= 1
        if method == 0 or N > 33:       # see the docstring
            assert by_trajectory >= 1 and refused >= 1
        if method == 1:
            assert follower.compared >= pc.B
        print(D, method, "exhausted by trajectory", by_trajectory, "by history", by_history, "refused after", refused,
              "compared", follower.compared, stats.line())
    finally:
        follower.close()

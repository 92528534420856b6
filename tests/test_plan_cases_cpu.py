"""The replan programs of plan_cases.py on the oracle alone: every (kind, joint count, sampling method)
must contain what test_gpu_plan_all_dofs.py is there to compare -- Plans with 0, 1, 2 and 3 or more
windows, histories past 2 N samples, trajectories longer than the tight set's capacity, every
status, every edge with the status it is built for -- so that the GPU tests cannot pass vacuously.
The invariants the GPU tests assert on the set's own output are asserted here on the oracle's."""
import numpy as np
import pytest

import plan_cases as pc


@pytest.fixture(scope="module")
def tpo():
    from oracle import tpo
    tpo.build()
    return tpo


def check_oracle_invariants(step, paths, N, method, where):
    for b in range(pc.B):
        o = step.oracle[b]
        if step.rc[b] != 0 or o.num_samples == 0:
            continue
        pc.check_invariants(o.time, o.path_parameter, o.accelerations, np.asarray(paths[b]["amax"]),
                            pc.path_end_of(paths[b], N), paths[b]["kind"], method, where + (step.index, b))
        # at rest at the last sample once the target is reached
        if o.target_reached:
            assert (o.velocities[-1] == 0).all(), where + (step.index, b)


@pytest.mark.parametrize("method", (0, 1))
@pytest.mark.parametrize("D", pc.ALL_DOFS)
@pytest.mark.parametrize("kind", pc.KINDS)
def test_program_covers_what_the_gpu_tests_compare(tpo, kind, D, method):
    program = pc.Program(tpo, kind, D, method)
    N, stats, paths = program.N, pc.Stats(pc.window_samples(D, method)), [None] * pc.B
    for step in program.steps():
        paths = [step.new_paths.get(b, paths[b]) for b in range(pc.B)]
        stats.add(step)
        for b in range(pc.B):
            edge, rc, o = step.edges[b], int(step.rc[b]), step.oracle[b]
            if edge:
                assert rc in pc.EDGE_STATUS[edge], (step.index, b, edge, rc)
            if edge == "tangent":       # accepted, and the trajectory starts moving: sd_start > 0
                assert np.abs(o.velocities[0]).max() > 0, (step.index, b)
            if edge == "whole":
                assert o.target_reached and o.windows == 1, (step.index, b)
            if edge == "same_start":
                assert o.windows >= 1, (step.index, b)
        check_oracle_invariants(step, paths, N, method, (kind, D, method))
    # DEADLINE_EXCEEDED: the same program on planners with max_planning_iterations = 1
    deadline = pc.Stats(N)
    deadline_windows = set()
    for step in pc.Program(tpo, kind, D, method, max_iterations=1, max_steps=pc.DEADLINE_STEPS).steps():
        deadline.add(step)
        deadline_windows |= {step.oracle[b].windows for b in range(pc.B) if step.rc[b] == 5}
    print(kind, D, method, "N", N, stats.line())
    print(kind, D, method, "max_iterations 1:", deadline.line())
    assert all(stats.windows[w] >= 1 for w in (0, 1, 2, 3)), stats.windows
    assert stats.max_history > 2 * N
    assert stats.max_samples > pc.TIGHT_TRAJECTORY
    assert all(stats.status[rc] >= 1 for rc in (0, 1, 2, 3, 4)), stats.status
    assert deadline.status[5] >= 1 and deadline_windows == {2}, (deadline.status, deadline_windows)
    assert len(stats.reached) >= pc.B // 2
    assert stats.ok >= 10 * pc.B
    for edge, allowed in pc.EDGE_STATUS.items():
        assert sum(stats.edges[(edge, rc)] for rc in allowed) >= 1, edge

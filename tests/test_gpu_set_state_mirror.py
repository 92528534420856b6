"""Moving planners between sets through the C++ mirror (PathTimingTrajectorySet::ExportPlanners /
ImportPlanners / CopyPlanners): tests/cpp/test_set_state_gpu.cc holds every moved planner against a
host PathTimingTrajectory that was given the same waypoints and Plans and continues on the host --
getters at once after the move, then three more Plans, bit for bit -- for export + import into a set
of other capacities in reversed order, CopyPlanners into a third set and a rotation in place, at
D = 3 and 7 with both sampling methods; refused calls change nothing. The bridge from the
reference-named class: the bytes PlannerStateFromHost builds from a host planner equal the device
export of a set planner that was given the same calls, AdoptPlanner takes the host planner into a set
that continues bit-equal to a twin host planner, and ReleasePlanner hands it to a fresh host planner
that continues bit-equal as well."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_mirror_moves_planners_against_host_planners(tmp_path):
    require_gpu()
    exe = build_driver("test_set_state_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m"))
    out = run_driver(exe, timeout=300, forbid_fail=True)
    assert out.count("set state vs host planners") == 4
    assert out.count("equal to the device export, 6 of 6 continued Plans bit-equal") == 4

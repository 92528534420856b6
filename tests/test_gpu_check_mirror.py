"""CheckSolutions on BatchPathTiming, BatchWaypointTiming and BatchCartesianTiming
(tests/cpp/test_check_solutions_gpu.cc): 16 paths of the shapes (7, 65, 4) and (16, 33, 3); violations
== 0 exactly where the mirror's own TimeOptimalPathProfile::SolutionSatisfiesConstraints() is ok, and
timing results bit-equal with the option off and on."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_check_solutions_option_of_the_batch_classes(tmp_path):
    require_gpu()
    exe = build_driver("test_check_solutions_gpu.cc", tmp_path, libs=("host", "oracle", "engine", "hip", "m"), flags=("-w",))
    out = run_driver(exe, timeout=300, forbid_fail=True)
    for cls in ("BatchPathTiming", "BatchWaypointTiming", "BatchCartesianTiming"):
        for shape in ("(7, 65, 4)", "(16, 33, 3)"):
            assert "%s %s: " % (cls, shape) in out

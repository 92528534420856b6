"""RefineSolutions on BatchPathTiming and BatchWaypointTiming (tests/cpp/test_batch_refine_gpu.cc): 16
paths of the shapes (7, 33, 4) and (16, 33, 4), two rounds. Off is bit-equal to never set; on, every
path is held against tpamd_time_joint_paths_refined_host on the same arrays (a cured path carries
2 n - 1 or 4 n - 3 samples, violations == 0 and the slot's arrays; a path refinement does not improve
keeps its coarse arrays), the offsets follow the sample counts, and the waypoint batch equals the path
batch."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_refine_solutions_option_of_the_batch_classes(tmp_path):
    require_gpu()
    exe = build_driver("test_batch_refine_gpu.cc", tmp_path, libs=("host", "engine", "hip", "m"), flags=("-w",))
    out = run_driver(exe, timeout=300, forbid_fail=True)
    for cls in ("BatchPathTiming", "BatchWaypointTiming"):
        for shape in ("(7, 33, 4)", "(16, 33, 4)"):
            assert "%s %s: " % (cls, shape) in out

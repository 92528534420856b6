"""BatchCartesianTiming on paths of different lengths (tests/cpp/test_cartesian_ragged_mirror_gpu.cc):
40 paths of 40 distinct lengths, D in {6, 7}. Every result is bit-equal to timing that path alone
(and to the oracle), and EngineCallsOfLastCompute() is the number of (dofs, safety,
ceil(samples / 512)) buckets -- 4, where one call per exact sample count made 40."""
import pytest

from native_driver import build_driver, require_gpu, run_driver

pytestmark = pytest.mark.gpu


def test_mirror_times_40_lengths_in_one_call_per_bucket(tmp_path):
    require_gpu()
    exe = build_driver("test_cartesian_ragged_mirror_gpu.cc", tmp_path, libs=("host", "oracle", "engine", "hip", "m"),
                       flags=("-w",))
    out = run_driver(exe, timeout=300, forbid_fail=True)
    assert "oracle: 40 of 40 paths solved" in out
    assert "engine calls: 4, buckets: 4, distinct sample counts: 40" in out
    assert "bit-equal to the path alone: 40 of 40; to the oracle: 40 of 40" in out

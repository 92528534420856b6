"""The C++ host mirror of the reference API (TimeOptimalPathProfile, TimeablePath,
TimeableJointSplinePath, PathTimingTrajectory, BatchPathTiming) on a real GPU: a C++
test program linked against libtp_host.so (product) and the oracle (checker)."""
import os

import pytest

from native_driver import CPP, build_driver, run_driver


def _build_test_binary():
    return build_driver("test_host_api.cc", CPP, libs=("host", "engine", "oracle", "m"))


def test_host_api_builds_on_cpu():
    """CPU side: the mirror and its test program compile and link (no GPU call)."""
    exe = _build_test_binary()
    assert os.path.exists(exe)


@pytest.mark.gpu
def test_host_api_on_gpu():
    run_driver(_build_test_binary(), timeout=600)

"""BatchCartesianTiming on paths of different lengths (tests/cpp/test_cartesian_ragged_mirror_gpu.cc):
40 paths of 40 distinct lengths, D in {6, 7}. Every result is bit-equal to timing that path alone
(and to the oracle), and EngineCallsOfLastCompute() is the number of (dofs, safety,
ceil(samples / 512)) buckets -- 4, where one call per exact sample count made 40."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

pytestmark = pytest.mark.gpu


def test_mirror_times_40_lengths_in_one_call_per_bucket(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    importlib.import_module(PKG_NAME + ".engine").build_library()
    csrc = os.path.join(ROOT, PKG_NAME, "csrc")
    host = os.path.join(ROOT, PKG_NAME, "host")
    oracle = os.path.join(ROOT, "oracle")
    subprocess.check_call(["make", "-C", host, "-s"])
    subprocess.check_call(["make", "-C", oracle, "-s", "libtp_oracle.so"])
    exe = str(tmp_path / "test_cartesian_ragged_mirror_gpu")
    subprocess.check_call(
        ["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-w",
         "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_cartesian_ragged_mirror_gpu.cc"),
         "-L" + host, "-ltp_host", "-Wl,-rpath," + host, "-L" + oracle, "-ltp_oracle", "-Wl,-rpath," + oracle,
         "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + csrc])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-4000:])
    print(out.stderr[-2000:])
    assert out.returncode == 0 and "ALL OK" in out.stdout and "FAIL" not in out.stdout
    assert "oracle: 40 of 40 paths solved" in out.stdout
    assert "engine calls: 4, buckets: 4, distinct sample counts: 40" in out.stdout
    assert "bit-equal to the path alone: 40 of 40; to the oracle: 40 of 40" in out.stdout

"""Build and run the stand-alone C++ drivers under tests/cpp/.

Tests import this module the way they import conftest for ROOT / PKG_NAME. A test names what its
driver links and how it is compiled; the g++ command line, the libraries brought up to date before
it and the common pass criterion (exit status 0 and "ALL OK" on stdout) live here."""
import importlib
import os
import subprocess

import pytest

from conftest import ROOT, PKG_NAME

CPP = os.path.join(ROOT, "tests", "cpp")
HOST = os.path.join(ROOT, PKG_NAME, "host")
CSRC = os.path.join(ROOT, PKG_NAME, "csrc")
ORACLE = os.path.join(ROOT, "oracle")
ROCM = "/opt/rocm"

# library name -> (directory or None, link name, rpath?)
_LIBS = {
    "host": (HOST, "tp_host", True),
    "engine": (CSRC, "tpamd", True),
    "multi": (CSRC, "tpamd_multi", True),      # built by tests/test_gpu_multi.py itself
    "oracle": (ORACLE, "tp_oracle", True),
    "hip": (ROCM + "/lib", "amdhip64", False),
    "m": (None, "m", False),
}


def require_gpu():
    """Fails (never skips) a test marked gpu on a machine without one."""
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")


def update_library(name):
    """Brings one of the project's libraries up to date."""
    if name == "engine":
        importlib.import_module(PKG_NAME + ".engine").build_library()
    elif name == "host":
        subprocess.check_call(["make", "-C", HOST, "-s"])
    elif name == "oracle":
        subprocess.check_call(["make", "-C", ORACLE, "-s", "libtp_oracle.so"])


def driver_command(source, out_dir, libs=(), extra_sources=(), opt="-O1", flags=(), std="c++17",
                   fp_contract_off=True, name=None):
    """The g++ command of build_driver and the path of the executable it writes."""
    source = str(source)
    if not os.path.isabs(source):
        source = os.path.join(CPP, source)
    exe = os.path.join(str(out_dir), name or os.path.splitext(os.path.basename(source))[0])
    cmd = ["g++"] + ([opt] if opt else []) + ["-std=" + std]
    if fp_contract_off:
        cmd.append("-ffp-contract=off")
    cmd += list(flags)
    if "hip" in libs:
        cmd += ["-D__HIP_PLATFORM_AMD__", "-I" + ROCM + "/include"]
    cmd += ["-o", exe, source]
    cmd += [s if os.path.isabs(s) else os.path.join(ROOT, PKG_NAME, s) for s in extra_sources]
    rpaths = []
    for lib in libs:
        directory, link_name, rpath = _LIBS[lib]
        if directory and "-L" + directory not in cmd:
            cmd.append("-L" + directory)
        cmd.append("-l" + link_name)
        if rpath and "-Wl,-rpath," + directory not in rpaths:
            rpaths.append("-Wl,-rpath," + directory)
    return cmd + rpaths, exe


def build_driver(source, out_dir, libs=(), extra_sources=(), opt="-O1", flags=(), std="c++17",
                 fp_contract_off=True, name=None, prebuilt=(), timeout=None):
    """Compiles one driver with g++ and returns the path of the executable.

    source: a file name under tests/cpp/ or an absolute path. libs: what to link, in link order, from
    "host" (libtp_host.so), "engine" (libtpamd.so), "oracle" (libtp_oracle.so), "hip" (libamdhip64.so
    with the HIP headers), "multi" and "m"; each of the project's libraries gets its -L and rpath and
    is brought up to date first unless it is named in prebuilt. extra_sources: host sources compiled
    in, relative to the package directory. flags: further compiler flags, placed before the sources.
    timeout: a time limit for the compilation, in seconds."""
    for lib in ("engine", "host", "oracle"):
        if lib in libs and lib not in prebuilt:
            update_library(lib)
    cmd, exe = driver_command(source, out_dir, libs, extra_sources, opt, flags, std, fp_contract_off, name)
    subprocess.check_call(cmd, timeout=timeout)
    return exe


def run_driver(exe, *args, timeout=300, head=0, tail=4000, err_tail=2000, forbid_fail=False):
    """Runs a driver, prints the head and tail of its stdout and the tail of its stderr, asserts the
    common pass criterion and returns stdout. forbid_fail also refuses any "FAIL" on stdout."""
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=timeout)
    if head:
        print(out.stdout[:head])
    print(out.stdout[-tail:])
    print(out.stderr[-err_tail:])
    assert out.returncode == 0 and "ALL OK" in out.stdout
    if forbid_fail:
        assert "FAIL" not in out.stdout
    return out.stdout

"""Build and run tools/set_retarget_bench.cc on the GPU: one retarget call for 1024 seven-joint
planners in mid-motion against GetSetpoints + host ComputeStoppingPoint + SetWaypointPaths; the JSON
line also goes to profiles/set_retarget_bench.json.  python tools/gpu_set_retarget_bench.py [B trials]"""
import importlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
importlib.import_module(PKG + ".engine").build_library()
host, csrc = os.path.join(ROOT, PKG, "host"), os.path.join(ROOT, PKG, "csrc")
subprocess.check_call(["make", "-C", host, "-s"])
exe = os.path.join(ROOT, "tools", "set_retarget_bench")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include",
                       "-o", exe, exe + ".cc", "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib",
                       "-lamdhip64", "-lm", "-Wl,-rpath," + host, "-Wl,-rpath," + csrc])
out = subprocess.run([exe] + sys.argv[1:], capture_output=True, text=True)
sys.stdout.write(out.stdout)
sys.stderr.write(out.stderr)
if out.returncode == 0 and out.stdout.startswith("{"):
    with open(os.path.join(ROOT, "profiles", "set_retarget_bench.json"), "w") as f:
        f.write(out.stdout)
sys.exit(out.returncode)

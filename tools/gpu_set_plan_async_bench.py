"""Build and run tools/set_plan_async_bench.cc on the GPU: a steady replan of 1024 x 7 x 1000 planners
through tpamd_planner_set_plan, through tpamd_planner_set_plan_device with max_windows 1, 2 and 4, and
the four-call control cycle both ways; the JSON line also goes to profiles/set_plan_async_bench.json.
python tools/gpu_set_plan_async_bench.py [B trials N]"""
import importlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
importlib.import_module(PKG + ".engine").build_library()
csrc = os.path.join(ROOT, PKG, "csrc")
exe = os.path.join(ROOT, "tools", "set_plan_async_bench")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-o", exe, exe + ".cc",
                       "-L" + csrc, "-ltpamd", "-L/opt/rocm/lib", "-lamdhip64", "-lm", "-Wl,-rpath," + csrc])
out = subprocess.run([exe] + sys.argv[1:], capture_output=True, text=True)
sys.stdout.write(out.stdout)
sys.stderr.write(out.stderr)
if out.returncode == 0 and out.stdout.startswith("{"):
    with open(os.path.join(ROOT, "profiles", "set_plan_async_bench.json"), "w") as f:
        f.write(out.stdout)
sys.exit(out.returncode)

"""Build and run tools/cartesian_discard_bench.cc on the GPU: a streaming Cartesian planner set that never
discards table rows against one that discards after every Plan.  python tools/gpu_cartesian_discard_bench.py [B N]"""
import importlib, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "x-edr-trajectory-planning_amd"
importlib.import_module(PKG + ".engine").build_library()
host, csrc = os.path.join(ROOT, PKG, "host"), os.path.join(ROOT, PKG, "csrc")
subprocess.check_call(["make", "-C", host, "-s"])
exe = os.path.join(ROOT, "tools", "cartesian_discard_bench")
subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, exe + ".cc",
                       "-L" + host, "-ltp_host", "-L" + csrc, "-ltpamd", "-lm",
                       "-Wl,-rpath," + host, "-Wl,-rpath," + csrc])
sys.exit(subprocess.call([exe] + sys.argv[1:]))

"""What the ctypes binding knows about the C-ABI without calling it: how csrc/ is compiled, the
ctypes mirrors of the structs of include/tpamd.h, and the prototype of every function the header
declares, read from the header itself. engine.py re-exports all of it."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tpamd.h")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared",
               "-std=c++17"]

# (joint count, extra rows) instances of the specialised sweep kernel: one translation unit each
# (csrc/tpamd_launch.h TPAMD_SWEEP_INSTANCES must list the same pairs)
SWEEP_INSTANCES = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (14, 0), (6, 2), (7, 2)]

MULTI_SO = os.path.join(_CSRC, "libtpamd_multi.so")
DIAG_SO = os.path.join(_CSRC, "libtpamd_diag.so")


class TpamdError(RuntimeError):
    pass


def library_sources():
    """What libtpamd.so is compiled from: every header and HIP source under csrc/ and the C-ABI
    header. A library older than any of them is rebuilt."""
    return sorted(glob.glob(os.path.join(_CSRC, "*.h")) + glob.glob(os.path.join(_CSRC, "*.hip"))) + [_HEADER]


def _compile(target, extra_flags, force, verbose):
    """hipcc -c every translation unit (in parallel: the sweep instances take 10-18 s each), then
    link. Objects are kept per target under build/ so that a rebuild recompiles everything only
    when a source changed."""
    stale = force or not os.path.exists(target) or any(
        os.path.getmtime(d) > os.path.getmtime(target) for d in library_sources())
    if not stale:
        return target
    from concurrent.futures import ThreadPoolExecutor
    objdir = os.path.join(os.path.dirname(_HERE), "build",
                          "obj_" + os.path.splitext(os.path.basename(target))[0])
    os.makedirs(objdir, exist_ok=True)
    flags = [f for f in HIPCC_FLAGS if f != "-shared"] + list(extra_flags)
    units = [(os.path.join(objdir, "capi.o"), ["tpamd_capi.hip"]),
             (os.path.join(objdir, "fit.o"), ["tpamd_fit.hip"]),
             (os.path.join(objdir, "pose_fit.o"), ["tpamd_pose_fit.hip"]),
             (os.path.join(objdir, "retarget.o"), ["tpamd_retarget.hip"]),
             (os.path.join(objdir, "joint_fit.o"), ["tpamd_joint_fit.hip"]),
             (os.path.join(objdir, "refine.o"), ["tpamd_refine.hip"]),
             (os.path.join(objdir, "state.o"), ["tpamd_state.hip"])]
    for d, e in SWEEP_INSTANCES:
        units.append((os.path.join(objdir, "sweep_%d_%d.o" % (d, e)),
                      ["-DTPAMD_INST_D=%d" % d, "-DTPAMD_INST_E=%d" % e, "tpamd_sweep_inst.hip"]))

    def one(unit):
        obj, args = unit
        cmd = ["hipcc"] + flags + ["-c", "-o", obj] + args[:-1] + [os.path.join(_CSRC, args[-1])]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=_CSRC)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        objs = list(pool.map(one, units))
    cmd = ["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", target] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd, cwd=_CSRC)
    return target


def _compile_multi(engine_so, force, verbose):
    src = os.path.join(_CSRC, "tpamd_multi.cc")
    deps = [src, _HEADER, os.path.join(os.path.dirname(_HEADER), "tpamd_multi.h"), engine_so]
    if force or not os.path.exists(MULTI_SO) or any(
            os.path.getmtime(d) > os.path.getmtime(MULTI_SO) for d in deps if os.path.exists(d)):
        cmd = ["hipcc", "-O2", "-fPIC", "-shared", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", src,
               "-o", MULTI_SO, "-L" + _CSRC, "-ltpamd", "-L/opt/rocm/lib", "-lrccl", "-lpthread",
               "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=_CSRC)
    return MULTI_SO


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous()
    return t.data_ptr()


# ---------------------------------------------------------------- struct mirrors
class _Mirror(C.Structure):
    """The ctypes mirror of the struct _c_name_ of include/tpamd.h, field for field
    (tests/test_abi_cpu.py compares the layouts with the compiler's)."""
    _c_name_ = None

    def __init_subclass__(cls, **kw):
        super().__init_subclass__(**kw)
        cls._keys_ = tuple(name for name, _ in cls.__dict__.get("_fields_", ()))

    @classmethod
    def from_dict(cls, arrays):
        """A struct of pointers from a dict of arrays keyed by the field names (absent or None: NULL)."""
        return cls(*map(_ptr, map(arrays.get, cls._keys_)))


def _pointers(*names):
    return [(n, C.c_void_p) for n in names]


class _JointBatch(_Mirror):
    _c_name_ = "tpamd_joint_batch"
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("num_points", C.c_int32), ("max_solver_loops", C.c_int32),
                ("reserved", C.c_int32), ("constraint_safety", C.c_double)]


class _JointInputs(_Mirror):
    _c_name_ = "tpamd_joint_inputs"
    _fields_ = _pointers("knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
                         "sd_start", "sdd_start", "time_start", "num_samples_per_path")


class _PathOutputs(_Mirror):
    _c_name_ = "tpamd_path_outputs"
    _fields_ = _pointers("time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
                         "max_time_increment", "status", "sd2")


class _WaypointBatch(_Mirror):
    _c_name_ = "tpamd_waypoint_batch"
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("max_solver_loops", C.c_int32), ("constraint_safety", C.c_double)]


class _WaypointInputs(_Mirror):
    _c_name_ = "tpamd_waypoint_inputs"
    _fields_ = _pointers("waypoint_offsets", "waypoints", "rounding", "max_velocity", "max_acceleration",
                         "num_samples_per_path", "delta", "sd_start", "time_start")


class _WaypointFitOutputs(_Mirror):
    _c_name_ = "tpamd_waypoint_fit_outputs"
    _fields_ = _pointers("num_points", "path_end", "delta_used", "knots", "control_points")


class _Solution(_Mirror):
    _c_name_ = "tpamd_solution"
    _fields_ = _pointers("sd2", "sd", "sdd", "status")


class _CheckOutputs(_Mirror):
    _c_name_ = "tpamd_check_outputs"
    _fields_ = _pointers("violations", "worst_excess", "worst_sample", "worst_row", "first_sample")


class _RefineOptions(_Mirror):
    _c_name_ = "tpamd_refine_options"
    _fields_ = [("max_rounds", C.c_int32), ("max_samples", C.c_int32), ("max_refined", C.c_int32),
                ("reserved", C.c_int32), ("tolerance", C.c_double)]


class _RefineOutputs(_Mirror):
    _c_name_ = "tpamd_refine_outputs"
    _fields_ = ([("check", _CheckOutputs)] +
                _pointers("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta") +
                [("refined", _PathOutputs), ("refined_check", _CheckOutputs)])


# slot[b] below 0 (include/tpamd.h tpamd_refine_outputs)
REFINE_NOTHING, REFINE_NO_SLOT, REFINE_TOO_LONG = -1, -2, -3


class _RowsBatch(_Mirror):
    _c_name_ = "tpamd_rows_batch"
    _fields_ = [("num_paths", C.c_int32), ("num_samples", C.c_int32), ("num_rows", C.c_int32),
                ("max_solver_loops", C.c_int32)]


class _RowsInputs(_Mirror):
    _c_name_ = "tpamd_rows_inputs"
    _fields_ = _pointers("a", "b", "lower", "upper", "s_start", "s_end", "sd_start", "sdd_start", "time_start")


class _CartesianBatch(_Mirror):
    _c_name_ = "tpamd_cartesian_batch"
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("max_solver_loops", C.c_int32), ("constraint_safety", C.c_double)]


class _CartesianInputs(_Mirror):
    _c_name_ = "tpamd_cartesian_inputs"
    _fields_ = _pointers("ik_positions", "jacobians", "max_velocity", "max_acceleration",
                         "max_translational_velocity", "max_rotational_velocity", "path_start",
                         "delta", "sd_start", "sdd_start", "time_start")


class _ResampleArgs(_Mirror):
    _c_name_ = "tpamd_resample_args"
    _fields_ = ([("num_paths", C.c_int32), ("num_samples", C.c_int32), ("num_dofs", C.c_int32),
                 ("max_out", C.c_int32)] +
                _pointers("time", "s", "sd", "sdd", "q", "qd", "qdd", "max_acceleration", "start_sec") +
                [("time_step", C.c_double), ("status", C.c_void_p)] +
                _pointers("out_time", "out_s", "out_sd", "out_sdd", "out_q", "out_qd", "out_qdd", "count"))


class _FastestStopArgs(_Mirror):
    _c_name_ = "tpamd_fastest_stop_args"
    _fields_ = ([("num_paths", C.c_int32), ("stride", C.c_int32), ("num_dofs", C.c_int32),
                 ("reserved", C.c_int32)] +
                _pointers("time", "s", "qd", "qdd", "count", "max_acceleration", "query_time", "stop_parameter",
                          "stop_index", "duration", "status", "profile_time", "profile_rate2", "profile_drate2"))


class _StopTrajectoryArgs(_Mirror):
    _c_name_ = "tpamd_stop_trajectory_args"
    _fields_ = ([("num_paths", C.c_int32), ("stride", C.c_int32), ("num_dofs", C.c_int32),
                 ("reserved", C.c_int32)] +
                _pointers("time", "qd", "qdd", "count", "max_acceleration") +
                [("time_step", C.c_double)] +
                _pointers("stop_time", "stop_index", "status", "keep", "first", "last", "out_time", "out_qd",
                          "out_qdd"))


class _PlannerSetConfig(_Mirror):
    _c_name_ = "tpamd_planner_set_config"
    _fields_ = ([(n, C.c_int32) for n in (
        "num_planners", "num_dofs", "num_samples", "num_points", "history_capacity",
        "trajectory_capacity", "sampling_method", "max_planning_iterations")] +
                [("constraint_safety", C.c_double), ("max_initial_velocity_error", C.c_double),
                 ("time_step_ns", C.c_int64)])


# tpamd_planner_summary
PLANNER_SUMMARY_DTYPE = np.dtype([
    ("end_time_ns", np.int64), ("final_decel_start_ns", np.int64), ("start_time_ns", np.int64),
    ("num_samples", np.int32), ("target_reached", np.int32), ("planned_to_end", np.int32),
    ("windows", np.int32), ("path_state", np.int32), ("history_count", np.int32),
    ("status", np.int32), ("reserved", np.int32)])

# tpamd_plan_device_info
PLAN_DEVICE_INFO_FIELDS = ("num_ok", "num_failed", "num_exhausted", "needed_history", "needed_trajectory",
                           "max_windows_solved")


class _PlanDeviceInfo(_Mirror):
    _c_name_ = "tpamd_plan_device_info"
    _fields_ = [(n, C.c_int32) for n in PLAN_DEVICE_INFO_FIELDS] + [("reserved", C.c_int32 * 2)]


PLAN_RESOURCE_EXHAUSTED = 8     # TPAMD_PLAN_RESOURCE_EXHAUSTED

# tpamd_planner_state_info (56 bytes)
PLANNER_STATE_INFO_DTYPE = np.dtype([
    ("bytes", np.int64), ("num_points", np.int32), ("history_count", np.int32), ("trajectory_count", np.int32),
    ("table_rows", np.int32), ("first_row", np.int32), ("has_path", np.int32), ("path_state", np.int32),
    ("initial_plan", np.int32), ("planned_to_end", np.int32), ("target_reached", np.int32),
    ("trajectory_first", np.int32), ("status", np.int32)])

# tpamd_planner_check (48 bytes)
PLANNER_CHECK_DTYPE = np.dtype([
    ("windows", np.int32), ("violations", np.int32), ("last_window_violations", np.int32),
    ("worst_window", np.int32), ("worst_sample", np.int32), ("worst_row", np.int32),
    ("first_window", np.int32), ("first_sample", np.int32),
    ("worst_excess", np.float64), ("worst_parameter", np.float64)])


class _PlannerCheck(_Mirror):
    _c_name_ = "tpamd_planner_check"
    _fields_ = ([(n, C.c_int32) for n in PLANNER_CHECK_DTYPE.names[:8]] +
                [(n, C.c_double) for n in PLANNER_CHECK_DTYPE.names[8:]])


MIRRORS = {cls._c_name_: cls for cls in _Mirror.__subclasses__()}

# ---------------------------------------------------------------- prototypes from the header
_SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t}
_PROTOTYPE = re.compile(r"^[ \t]*((?:\w+[ \t]+)+\**)[ \t]*(tpamd_\w+)[ \t]*\(([^)]*)\)[ \t]*;", re.M)


def _ctype(decl, returned=False):
    """The ctypes type of one parameter declaration (its name, if any, is dropped) or return type."""
    words = decl.replace("*", " * ").split()
    const, stars = "const" in words, words.count("*")
    base = [w for w in words if w not in ("const", "*")]
    if not returned and len(base) > 1:
        base.pop()
    base = " ".join(base)
    if stars == 0 and returned and base == "void":
        return None
    if stars == 0 and base in _SCALARS:
        return _SCALARS[base]
    if returned:
        if stars == 1 and const and base == "char":
            return C.c_char_p
    elif stars and base:
        # a const pointer to a mirrored struct is an argument block, passed by reference; without
        # the const it is an array of records the call writes, passed by address like any array
        return C.POINTER(MIRRORS[base]) if stars == 1 and const and base in MIRRORS else C.c_void_p
    raise TpamdError("include/tpamd.h: no ctypes type for %r" % " ".join(decl.split()))


def _declarations(text):
    """(return type, name, parameter list) of every tpamd_ function declared in a header text."""
    return _PROTOTYPE.findall(re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def parse_prototypes(text):
    """{name: (restype, argtypes)} of every tpamd_ function a header text declares. A declaration
    with a type that has no ctypes counterpart here raises TpamdError."""
    out = {}
    for ret, name, params in _declarations(text):
        params = [p for p in params.split(",") if p.strip()]
        if len(params) == 1 and params[0].split() == ["void"]:
            params = []
        out[name] = (_ctype(ret, returned=True), [_ctype(p) for p in params])
    return out


def _header_text():
    with open(_HEADER) as f:
        return f.read()


# every symbol include/tpamd.h declares
ABI_SYMBOLS = [name for _, name, _ in _declarations(_header_text())]


def declare(lib):
    """Sets restype and argtypes of every function of include/tpamd.h on a loaded library."""
    for name, (restype, argtypes) in parse_prototypes(_header_text()).items():
        f = getattr(lib, name)
        f.restype, f.argtypes = restype, argtypes
    return lib

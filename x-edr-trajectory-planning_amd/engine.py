"""ctypes binding of the engine's C-ABI (include/tpamd.h -> csrc/libtpamd.so).

Plumbing only: device memory, streams and torch.distributed come from PyTorch;
all computation happens in the hand-written HIP kernels behind the C-ABI. There
is NO CPU fallback: if the shared library or a HIP device is missing, every
entry point raises.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
_SO = os.environ.get("TPAMD_LIBRARY") or os.path.join(_CSRC, "libtpamd.so")   # override: A/B builds
_SOURCES = ["tpamd_capi.hip", "tpamd_sweep_inst.hip", "tpamd_launch.h", "tpamd_kernels.h", "tpamd_device.h",
            "tpamd_sweep_joint.h", "tpamd_planner_set.h", "tpamd_cartesian_window.h", "tpamd_stop.h", "tpamd_switch.h", "tpamd_readout.h",
            "tpamd_rescale.h", "tpamd_buffer.h", "tpamd_fit.h", "tpamd_fit.hip", "tpamd_quat.h", "tpamd_pose_fit.h",
            "tpamd_pose_fit.hip", "tpamd_retarget.h", "tpamd_retarget.hip", "tpamd_joint_fit.h", "tpamd_joint_fit.hip",
            "tpamd_check.h", "tpamd_refine.h", "tpamd_refine.hip", "tpamd_state.h", "tpamd_state.hip"]
_HEADER = os.path.join(os.path.dirname(_HERE), "include", "tpamd.h")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-shared",
               "-std=c++17"]

PATH_STATUS = {
    0: "ok", 2: "infeasible_bounds", 3: "s_range", 4: "sd_start_negative",
    5: "lower_ge_upper", 6: "too_few_samples", 7: "no_connection", 8: "nan_sd2",
    9: "nonzero_end", 10: "crit_index_zero", 11: "no_waypoints",
}

KERNEL_SWEEP = 4


class TpamdError(RuntimeError):
    pass


# (joint count, extra rows) instances of the specialised sweep kernel: one translation unit each
# (csrc/tpamd_launch.h TPAMD_SWEEP_INSTANCES must list the same pairs)
SWEEP_INSTANCES = [(3, 0), (4, 0), (5, 0), (6, 0), (7, 0), (8, 0), (14, 0), (6, 2), (7, 2)]


def _compile(target, extra_flags, force, verbose):
    """hipcc -c every translation unit (in parallel: the sweep instances take 10-18 s each), then
    link. Objects are kept per target under build/ so that a rebuild recompiles everything only
    when a source changed."""
    deps = [os.path.join(_CSRC, s) for s in _SOURCES] + [_HEADER]
    stale = force or not os.path.exists(target) or any(
        os.path.getmtime(d) > os.path.getmtime(target) for d in deps)
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


def build_library(force=False, verbose=False, extra_flags=(), output=None):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    global _SO
    if output is not None:
        _SO = output
    return _compile(_SO, extra_flags, force, verbose)


MULTI_SO = os.path.join(_CSRC, "libtpamd_multi.so")


def build_multi_library(force=False, verbose=False):
    """libtpamd_multi.so (include/tpamd_multi.h): several devices from one process, on top of
    libtpamd.so and RCCL. Host code only."""
    src = os.path.join(_CSRC, "tpamd_multi.cc")
    deps = [src, _HEADER, os.path.join(os.path.dirname(_HEADER), "tpamd_multi.h"), _SO]
    if force or not os.path.exists(MULTI_SO) or any(
            os.path.getmtime(d) > os.path.getmtime(MULTI_SO) for d in deps if os.path.exists(d)):
        cmd = ["hipcc", "-O2", "-fPIC", "-shared", "-std=c++17", "-x", "hip", "--offload-arch=gfx950", src,
               "-o", MULTI_SO, "-L" + _CSRC, "-ltpamd", "-L/opt/rocm/lib", "-lrccl", "-lpthread",
               "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,/opt/rocm/lib"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd, cwd=_CSRC)
    return MULTI_SO


DIAG_SO = os.path.join(_CSRC, "libtpamd_diag.so")


def build_diagnostic_library(force=False, verbose=False):
    """The -DTPAMD_DIAG variant: in-kernel cycle counters and the literal cross-checks of the
    sweep kernel's shortcuts (tests/test_gpu_parity.py, tools/gpu_diag.py). Not the product."""
    return _compile(DIAG_SO, ("-DTPAMD_DIAG",), force, verbose)


class _JointBatch(C.Structure):
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("num_points", C.c_int32), ("max_solver_loops", C.c_int32),
                ("reserved", C.c_int32), ("constraint_safety", C.c_double)]


class _JointInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
        "sd_start", "sdd_start", "time_start", "num_samples_per_path")]


class _PathOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
        "max_time_increment", "status", "sd2")]


class _WaypointBatch(C.Structure):
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("max_solver_loops", C.c_int32), ("constraint_safety", C.c_double)]


class _WaypointInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "waypoint_offsets", "waypoints", "rounding", "max_velocity", "max_acceleration",
        "num_samples_per_path", "delta", "sd_start", "time_start")]


class _WaypointFitOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("num_points", "path_end", "delta_used", "knots", "control_points")]


class _Solution(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("sd2", "sd", "sdd", "status")]


_CHECK_OUTPUT_KEYS = ("violations", "worst_excess", "worst_sample", "worst_row", "first_sample")


class _CheckOutputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _CHECK_OUTPUT_KEYS]


class _RefineOptions(C.Structure):
    _fields_ = [("max_rounds", C.c_int32), ("max_samples", C.c_int32), ("max_refined", C.c_int32),
                ("reserved", C.c_int32), ("tolerance", C.c_double)]


class _RefineOutputs(C.Structure):
    _fields_ = [("check", _CheckOutputs), ("slot", C.c_void_p), ("slot_path", C.c_void_p),
                ("num_refined", C.c_void_p), ("rounds", C.c_void_p), ("num_samples", C.c_void_p),
                ("delta", C.c_void_p), ("refined", _PathOutputs), ("refined_check", _CheckOutputs)]


# slot[b] below 0 (include/tpamd.h tpamd_refine_outputs)
REFINE_NOTHING, REFINE_NO_SLOT, REFINE_TOO_LONG = -1, -2, -3


class _RowsBatch(C.Structure):
    _fields_ = [("num_paths", C.c_int32), ("num_samples", C.c_int32), ("num_rows", C.c_int32),
                ("max_solver_loops", C.c_int32)]


class _RowsInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "a", "b", "lower", "upper", "s_start", "s_end", "sd_start", "sdd_start", "time_start")]


class _CartesianBatch(C.Structure):
    _fields_ = [("num_paths", C.c_int32), ("num_dofs", C.c_int32), ("num_samples", C.c_int32),
                ("max_solver_loops", C.c_int32), ("constraint_safety", C.c_double)]


_CARTESIAN_INPUT_KEYS = ("ik_positions", "jacobians", "max_velocity", "max_acceleration",
                         "max_translational_velocity", "max_rotational_velocity", "path_start",
                         "delta", "sd_start", "sdd_start", "time_start")


class _CartesianInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _CARTESIAN_INPUT_KEYS]


class _ResampleArgs(C.Structure):
    _fields_ = ([("num_paths", C.c_int32), ("num_samples", C.c_int32), ("num_dofs", C.c_int32),
                 ("max_out", C.c_int32)] +
                [(n, C.c_void_p) for n in ("time", "s", "sd", "sdd", "q", "qd", "qdd",
                                           "max_acceleration", "start_sec")] +
                [("time_step", C.c_double), ("status", C.c_void_p)] +
                [(n, C.c_void_p) for n in ("out_time", "out_s", "out_sd", "out_sdd", "out_q",
                                           "out_qd", "out_qdd", "count")])


class _FastestStopArgs(C.Structure):
    _fields_ = ([("num_paths", C.c_int32), ("stride", C.c_int32), ("num_dofs", C.c_int32),
                 ("reserved", C.c_int32)] +
                [(n, C.c_void_p) for n in ("time", "s", "qd", "qdd", "count", "max_acceleration",
                                           "query_time", "stop_parameter", "stop_index", "duration",
                                           "status", "profile_time", "profile_rate2",
                                           "profile_drate2")])


class _StopTrajectoryArgs(C.Structure):
    _fields_ = ([("num_paths", C.c_int32), ("stride", C.c_int32), ("num_dofs", C.c_int32),
                 ("reserved", C.c_int32)] +
                [(n, C.c_void_p) for n in ("time", "qd", "qdd", "count", "max_acceleration")] +
                [("time_step", C.c_double)] +
                [(n, C.c_void_p) for n in ("stop_time", "stop_index", "status", "keep", "first", "last",
                                           "out_time", "out_qd", "out_qdd")])


class _PlannerSetConfig(C.Structure):
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


class _PlanDeviceInfo(C.Structure):
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


class _PlannerCheck(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in PLANNER_CHECK_DTYPE.names[:8]] +
                [(n, C.c_double) for n in PLANNER_CHECK_DTYPE.names[8:]])

_LIB = None

# every symbol include/tpamd.h declares
ABI_SYMBOLS = [
    "tpamd_engine_create", "tpamd_engine_destroy", "tpamd_version", "tpamd_error_string",
    "tpamd_device_count", "tpamd_shard_bounds", "tpamd_shard_bounds_balanced",
    "tpamd_engine_reserve", "tpamd_engine_set_pipelining", "tpamd_engine_fence",
    "tpamd_engine_workspace_bytes",
    "tpamd_time_joint_paths_device",
    "tpamd_time_joint_paths_host", "tpamd_sample_joint_paths_host",
    "tpamd_ik_table_rows", "tpamd_fit_pose_waypoints_host", "tpamd_fit_pose_waypoints_device",
    "tpamd_fit_joint_waypoints_host", "tpamd_fit_joint_waypoints_device",
    "tpamd_time_waypoint_paths_host", "tpamd_time_waypoint_paths_device",
    "tpamd_sample_ik_targets_host", "tpamd_sample_ik_targets_device",
    "tpamd_time_joint_groups_device", "tpamd_time_joint_groups_host",
    "tpamd_optimize_rows_device", "tpamd_optimize_rows_host",
    "tpamd_time_cartesian_paths_device", "tpamd_time_cartesian_paths_host",
    "tpamd_optimize_rows_ragged_device", "tpamd_optimize_rows_ragged_host",
    "tpamd_time_cartesian_paths_ragged_device", "tpamd_time_cartesian_paths_ragged_host",
    "tpamd_sample_pose_splines_device", "tpamd_sample_pose_splines_host",
    "tpamd_check_rows_device", "tpamd_check_rows_host",
    "tpamd_check_joint_paths_device", "tpamd_check_joint_paths_host",
    "tpamd_check_cartesian_paths_device", "tpamd_check_cartesian_paths_host",
    "tpamd_time_joint_paths_refined_device", "tpamd_time_joint_paths_refined_host",
    "tpamd_time_waypoint_paths_refined_device", "tpamd_time_waypoint_paths_refined_host",
    "tpamd_plan_joint_windows_host",
    "tpamd_planner_set_create", "tpamd_planner_set_destroy", "tpamd_planner_set_upload_paths",
    "tpamd_planner_set_reset", "tpamd_planner_set_plan", "tpamd_planner_set_download_trajectory",
    "tpamd_planner_set_reserve", "tpamd_planner_set_capacity", "tpamd_planner_set_plan_device",
    "tpamd_planner_set_last_plan_bytes", "tpamd_planner_set_device_bytes",
    "tpamd_planner_set_stop_parameters", "tpamd_planner_set_upload_paths_ragged",
    "tpamd_planner_set_set_checking", "tpamd_planner_set_checking",
    "tpamd_planner_set_check_results", "tpamd_planner_set_check_results_device",
    "tpamd_planner_set_download_path", "tpamd_planner_set_switch_paths", "tpamd_fastest_stop_device", "tpamd_fastest_stop_host",
    "tpamd_planner_set_sample_at_ticks", "tpamd_planner_set_sample_at_ticks_device",
    "tpamd_planner_set_download_trajectories", "tpamd_planner_set_download_trajectories_device",
    "tpamd_planner_set_stop_trajectories", "tpamd_planner_set_stop_trajectories_device",
    "tpamd_planner_set_set_waypoints", "tpamd_planner_set_set_waypoints_device",
    "tpamd_planner_set_switch_paths_rounded", "tpamd_planner_set_retarget", "tpamd_planner_set_retarget_device",
    "tpamd_compute_stopping_points_host", "tpamd_compute_stopping_points_device",
    "tpamd_project_points_on_paths_host", "tpamd_project_points_on_paths_device",
    "tpamd_planner_set_create_cartesian", "tpamd_planner_set_upload_ik_tables",
    "tpamd_planner_set_upload_ik_tables_device", "tpamd_planner_set_download_ik_table",
    "tpamd_planner_set_append_ik_rows", "tpamd_planner_set_append_ik_rows_device",
    "tpamd_planner_set_plan_streaming", "tpamd_planner_set_plan_resume",
    "tpamd_planner_set_discard_ik_rows", "tpamd_planner_set_ik_table_info",
    "tpamd_planner_set_download_ik_rows", "tpamd_planner_set_ik_table_device_pointers",
    "tpamd_sample_ik_target_rows_host", "tpamd_sample_ik_target_rows_device",
    "tpamd_stop_trajectories_device", "tpamd_stop_trajectories_host",
    "tpamd_planner_set_state_info", "tpamd_planner_set_state_bytes_bound",
    "tpamd_planner_set_export_state_host", "tpamd_planner_set_export_state_device",
    "tpamd_planner_set_import_state_host", "tpamd_planner_set_import_state_device",
    "tpamd_planner_set_copy_planners",
    "tpamd_buffer_set_create", "tpamd_buffer_set_destroy", "tpamd_buffer_set_reserve", "tpamd_buffer_set_capacity",
    "tpamd_buffer_set_device_bytes",
    "tpamd_buffer_set_insert", "tpamd_buffer_set_insert_device",
    "tpamd_buffer_set_insert_from_planner_set", "tpamd_buffer_set_insert_from_planner_set_device",
    "tpamd_buffer_set_append_sample", "tpamd_buffer_set_append_sample_device",
    "tpamd_buffer_set_discard_before", "tpamd_buffer_set_discard_before_device",
    "tpamd_buffer_set_stop_before_time", "tpamd_buffer_set_stop_before_time_device",
    "tpamd_buffer_set_sample_at_ticks", "tpamd_buffer_set_sample_at_ticks_device",
    "tpamd_buffer_set_add_offset", "tpamd_buffer_set_add_offset_device",
    "tpamd_buffer_set_clear", "tpamd_buffer_set_clear_device",
    "tpamd_buffer_set_info", "tpamd_buffer_set_info_device",
    "tpamd_buffer_set_download", "tpamd_buffer_set_download_device",
    "tpamd_find_max_sd2_host", "tpamd_query_device", "tpamd_resample_uniform_device",
    "tpamd_resample_uniform_host", "tpamd_resample_skip_device", "tpamd_resample_skip_host",
    "tpamd_debug_copy_boundary", "tpamd_debug_keep_boundary", "tpamd_debug_copy_diag", "tpamd_debug_copy_diag_ext",
    "tpamd_debug_kernel_vgprs",
    "tpamd_rebuild_time_device", "tpamd_profile_reset", "tpamd_profile_enable",
    "tpamd_profile_mean_ms", "tpamd_profile_kernel_name", "tpamd_profile_num_kernels",
]


def load_library():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise TpamdError(
            "libtpamd.so is not built (%s). Run __graft_entry__.build(); there is no CPU "
            "fallback for the engine." % _SO)
    # PyTorch ships its own HIP runtime; two runtimes in one process do not share devices.
    # Import torch first so that libtpamd.so binds to the runtime torch uses, whatever the
    # order the caller imports things in.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(_SO)
    vp, i = C.c_void_p, C.c_int
    L.tpamd_engine_create.restype = i
    L.tpamd_engine_create.argtypes = [i, C.POINTER(vp)]
    L.tpamd_engine_destroy.argtypes = [vp]
    L.tpamd_version.restype = i
    L.tpamd_error_string.restype = C.c_char_p
    L.tpamd_error_string.argtypes = [i]
    L.tpamd_device_count.restype = i
    L.tpamd_shard_bounds.restype = None
    L.tpamd_shard_bounds.argtypes = [i, i, vp]
    L.tpamd_shard_bounds_balanced.restype = None
    L.tpamd_shard_bounds_balanced.argtypes = [i, vp, i, vp]
    L.tpamd_engine_reserve.restype = i
    L.tpamd_engine_reserve.argtypes = [vp, i, i, i]
    L.tpamd_engine_set_pipelining.restype = i
    L.tpamd_engine_set_pipelining.argtypes = [vp, i]
    L.tpamd_engine_fence.restype = i
    L.tpamd_engine_fence.argtypes = [vp, vp]
    L.tpamd_engine_workspace_bytes.restype = C.c_size_t
    L.tpamd_engine_workspace_bytes.argtypes = [vp]
    L.tpamd_time_joint_paths_device.restype = i
    L.tpamd_time_joint_paths_device.argtypes = [vp, C.POINTER(_JointBatch),
                                                C.POINTER(_JointInputs),
                                                C.POINTER(_PathOutputs), vp]
    L.tpamd_time_joint_paths_host.restype = i
    L.tpamd_time_joint_paths_host.argtypes = [vp, C.POINTER(_JointBatch),
                                              C.POINTER(_JointInputs), C.POINTER(_PathOutputs)]
    L.tpamd_time_joint_groups_device.restype = i
    L.tpamd_time_joint_groups_device.argtypes = [vp, i, C.POINTER(_JointBatch), C.POINTER(_JointInputs),
                                                 C.POINTER(_PathOutputs), vp]
    L.tpamd_time_joint_groups_host.restype = i
    L.tpamd_time_joint_groups_host.argtypes = [vp, i, C.POINTER(_JointBatch), C.POINTER(_JointInputs),
                                               C.POINTER(_PathOutputs)]
    L.tpamd_sample_joint_paths_host.restype = i
    L.tpamd_sample_joint_paths_host.argtypes = [vp, i, i, i, i] + [vp] * 7
    L.tpamd_optimize_rows_device.restype = i
    L.tpamd_optimize_rows_device.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs),
                                             C.POINTER(_PathOutputs), vp]
    L.tpamd_optimize_rows_host.restype = i
    L.tpamd_optimize_rows_host.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs),
                                           C.POINTER(_PathOutputs)]
    L.tpamd_time_cartesian_paths_device.restype = i
    L.tpamd_time_cartesian_paths_device.argtypes = [vp, C.POINTER(_CartesianBatch),
                                                    C.POINTER(_CartesianInputs),
                                                    C.POINTER(_PathOutputs), vp]
    L.tpamd_time_cartesian_paths_host.restype = i
    L.tpamd_time_cartesian_paths_host.argtypes = [vp, C.POINTER(_CartesianBatch),
                                                  C.POINTER(_CartesianInputs),
                                                  C.POINTER(_PathOutputs)]
    sol, cko = C.POINTER(_Solution), C.POINTER(_CheckOutputs)
    L.tpamd_check_rows_device.restype = i
    L.tpamd_check_rows_device.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs), vp, sol, cko, vp]
    L.tpamd_check_rows_host.restype = i
    L.tpamd_check_rows_host.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs), vp, sol, cko]
    L.tpamd_check_joint_paths_device.restype = i
    L.tpamd_check_joint_paths_device.argtypes = [vp, C.POINTER(_JointBatch), C.POINTER(_JointInputs), vp, sol, cko,
                                                 vp]
    L.tpamd_check_joint_paths_host.restype = i
    L.tpamd_check_joint_paths_host.argtypes = [vp, C.POINTER(_JointBatch), C.POINTER(_JointInputs), vp, sol, cko]
    L.tpamd_check_cartesian_paths_device.restype = i
    L.tpamd_check_cartesian_paths_device.argtypes = [vp, C.POINTER(_CartesianBatch), C.POINTER(_CartesianInputs),
                                                     vp, vp, sol, cko, vp]
    L.tpamd_check_cartesian_paths_host.restype = i
    L.tpamd_check_cartesian_paths_host.argtypes = [vp, C.POINTER(_CartesianBatch), C.POINTER(_CartesianInputs),
                                                   vp, vp, C.c_int64, sol, cko]
    L.tpamd_optimize_rows_ragged_device.restype = i
    L.tpamd_optimize_rows_ragged_device.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs), vp,
                                                    C.POINTER(_PathOutputs), vp]
    L.tpamd_optimize_rows_ragged_host.restype = i
    L.tpamd_optimize_rows_ragged_host.argtypes = [vp, C.POINTER(_RowsBatch), C.POINTER(_RowsInputs), vp,
                                                  C.POINTER(_PathOutputs)]
    L.tpamd_time_cartesian_paths_ragged_device.restype = i
    L.tpamd_time_cartesian_paths_ragged_device.argtypes = [vp, C.POINTER(_CartesianBatch),
                                                           C.POINTER(_CartesianInputs), vp, vp,
                                                           C.POINTER(_PathOutputs), vp]
    L.tpamd_time_cartesian_paths_ragged_host.restype = i
    L.tpamd_time_cartesian_paths_ragged_host.argtypes = [vp, C.POINTER(_CartesianBatch),
                                                         C.POINTER(_CartesianInputs), vp, vp, C.c_int64,
                                                         C.POINTER(_PathOutputs)]
    L.tpamd_sample_pose_splines_host.restype = i
    L.tpamd_sample_pose_splines_host.argtypes = [vp, i, i, i] + [vp] * 6
    L.tpamd_sample_pose_splines_device.restype = i
    L.tpamd_sample_pose_splines_device.argtypes = [vp, i, i, i] + [vp] * 6 + [vp]
    L.tpamd_ik_table_rows.restype = i
    L.tpamd_ik_table_rows.argtypes = [C.c_double, C.c_double, i]
    for name in ("tpamd_fit_pose_waypoints_host", "tpamd_fit_pose_waypoints_device",
                 "tpamd_sample_ik_targets_host", "tpamd_sample_ik_targets_device"):
        getattr(L, name).restype = i
    L.tpamd_fit_pose_waypoints_host.argtypes = [vp, i, i] + [vp] * 13
    L.tpamd_fit_pose_waypoints_device.argtypes = [vp, i, i] + [vp] * 13 + [vp]
    L.tpamd_sample_ik_targets_host.argtypes = [vp, i, i] + [vp] * 9
    L.tpamd_sample_ik_targets_device.argtypes = [vp, i, i] + [vp] * 9 + [vp]
    for name in ("tpamd_fit_joint_waypoints_host", "tpamd_fit_joint_waypoints_device",
                 "tpamd_time_waypoint_paths_host", "tpamd_time_waypoint_paths_device"):
        getattr(L, name).restype = i
    L.tpamd_fit_joint_waypoints_host.argtypes = [vp, i, i] + [vp] * 9
    L.tpamd_fit_joint_waypoints_device.argtypes = [vp, i, i] + [vp] * 9 + [vp]
    L.tpamd_time_waypoint_paths_host.argtypes = [vp] * 5
    L.tpamd_time_waypoint_paths_device.argtypes = [vp] * 5 + [vp]
    for name in ("tpamd_time_joint_paths_refined_device", "tpamd_time_joint_paths_refined_host",
                 "tpamd_time_waypoint_paths_refined_device", "tpamd_time_waypoint_paths_refined_host"):
        getattr(L, name).restype = i
    L.tpamd_time_joint_paths_refined_device.argtypes = [vp] * 6 + [vp]
    L.tpamd_time_joint_paths_refined_host.argtypes = [vp] * 6
    L.tpamd_time_waypoint_paths_refined_device.argtypes = [vp] * 7 + [vp]
    L.tpamd_time_waypoint_paths_refined_host.argtypes = [vp] * 7
    L.tpamd_find_max_sd2_host.restype = i
    L.tpamd_find_max_sd2_host.argtypes = [vp, i, i] + [vp] * 7
    L.tpamd_query_device.restype = i
    L.tpamd_query_device.argtypes = [vp, i, i, i] + [vp] * 10 + [vp]
    L.tpamd_resample_uniform_device.restype = i
    L.tpamd_resample_uniform_device.argtypes = [vp, C.POINTER(_ResampleArgs), vp]
    L.tpamd_resample_uniform_host.restype = i
    L.tpamd_resample_uniform_host.argtypes = [vp, C.POINTER(_ResampleArgs)]
    L.tpamd_resample_skip_device.restype = i
    L.tpamd_resample_skip_device.argtypes = [vp, C.POINTER(_ResampleArgs), vp]
    L.tpamd_resample_skip_host.restype = i
    L.tpamd_resample_skip_host.argtypes = [vp, C.POINTER(_ResampleArgs)]
    L.tpamd_fastest_stop_device.restype = i
    L.tpamd_fastest_stop_device.argtypes = [vp, C.POINTER(_FastestStopArgs), vp]
    L.tpamd_fastest_stop_host.restype = i
    L.tpamd_fastest_stop_host.argtypes = [vp, C.POINTER(_FastestStopArgs)]
    L.tpamd_planner_set_stop_parameters.restype = i
    L.tpamd_planner_set_stop_parameters.argtypes = [vp, i] + [vp] * 5
    for name in ("tpamd_planner_set_set_checking", "tpamd_planner_set_checking", "tpamd_planner_set_check_results",
                 "tpamd_planner_set_check_results_device"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_set_checking.argtypes = [vp, i]
    L.tpamd_planner_set_checking.argtypes = [vp]
    L.tpamd_planner_set_check_results.argtypes = [vp, i, vp, vp]
    L.tpamd_planner_set_check_results_device.argtypes = [vp, i, vp, vp, vp]
    i64 = C.c_int64
    for name in ("tpamd_planner_set_sample_at_ticks", "tpamd_planner_set_sample_at_ticks_device",
                 "tpamd_planner_set_download_trajectories", "tpamd_planner_set_download_trajectories_device"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_sample_at_ticks.argtypes = [vp, i, vp, vp, i64, i] + [vp] * 4
    L.tpamd_planner_set_sample_at_ticks_device.argtypes = [vp, i, vp, vp, i64, i] + [vp] * 4 + [vp]
    L.tpamd_planner_set_download_trajectories.argtypes = [vp, i, vp, vp, i64] + [vp] * 7
    L.tpamd_planner_set_download_trajectories_device.argtypes = [vp, i, vp, vp, i64] + [vp] * 7 + [vp]
    for name in ("tpamd_planner_set_stop_trajectories", "tpamd_planner_set_stop_trajectories_device",
                 "tpamd_stop_trajectories_device", "tpamd_stop_trajectories_host"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_stop_trajectories.argtypes = [vp, i, vp, vp, vp, C.c_double, vp, vp, vp, i64] + [vp] * 4
    L.tpamd_planner_set_stop_trajectories_device.argtypes = (
        [vp, i, vp, vp, vp, C.c_double, vp, vp, vp, i64] + [vp] * 4 + [vp])
    L.tpamd_stop_trajectories_device.argtypes = [vp, vp, vp]
    dbl = C.c_double
    for name, args in (
            ("create", [vp, i, i, i, dbl, C.POINTER(vp)]), ("reserve", [vp, i]), ("capacity", [vp]),
            ("insert", [vp, i] + [vp] * 7), ("insert_device", [vp, i, vp, vp, i64] + [vp] * 6),
            ("insert_from_planner_set", [vp, vp, i, vp, vp, vp]),
            ("insert_from_planner_set_device", [vp, vp, i, vp, vp, vp, vp]),
            ("append_sample", [vp, i] + [vp] * 6), ("append_sample_device", [vp, i] + [vp] * 7),
            ("discard_before", [vp, i, vp, vp, vp]), ("discard_before_device", [vp, i] + [vp] * 5),
            ("stop_before_time", [vp, i, vp, vp, vp, vp, dbl, vp]),
            ("stop_before_time_device", [vp, i, vp, vp, vp, vp, dbl, vp, vp]),
            ("sample_at_ticks", [vp, i, vp, vp, i64, i] + [vp] * 4),
            ("sample_at_ticks_device", [vp, i, vp, vp, i64, i] + [vp] * 5),
            ("add_offset", [vp, i, vp, vp, vp]), ("add_offset_device", [vp, i] + [vp] * 5),
            ("clear", [vp, i, vp]), ("clear_device", [vp, i, vp, vp, vp]),
            ("info", [vp, i] + [vp] * 7), ("info_device", [vp, i] + [vp] * 8),
            ("download", [vp, i, vp, vp, i64] + [vp] * 4), ("download_device", [vp, i, vp, vp, i64] + [vp] * 5)):
        f = getattr(L, "tpamd_buffer_set_" + name)
        f.restype = i
        f.argtypes = args
    L.tpamd_buffer_set_destroy.restype = None
    L.tpamd_buffer_set_destroy.argtypes = [vp]
    L.tpamd_buffer_set_device_bytes.restype = C.c_size_t
    L.tpamd_buffer_set_device_bytes.argtypes = [vp]
    L.tpamd_stop_trajectories_host.argtypes = [vp, vp]
    # planner sets (PlannerSet)
    for name in ("tpamd_planner_set_create", "tpamd_planner_set_upload_paths",
                 "tpamd_planner_set_upload_paths_ragged", "tpamd_planner_set_download_path",
                 "tpamd_planner_set_reset", "tpamd_planner_set_plan",
                 "tpamd_planner_set_download_trajectory", "tpamd_planner_set_switch_paths",
                 "tpamd_planner_set_set_waypoints", "tpamd_planner_set_set_waypoints_device",
                 "tpamd_planner_set_create_cartesian", "tpamd_planner_set_upload_ik_tables",
                 "tpamd_planner_set_upload_ik_tables_device", "tpamd_planner_set_download_ik_table"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_create_cartesian.argtypes = [vp, C.POINTER(_PlannerSetConfig), i, C.POINTER(vp)]
    L.tpamd_planner_set_upload_ik_tables.argtypes = [vp, i] + [vp] * 12
    L.tpamd_planner_set_upload_ik_tables_device.argtypes = [vp, i] + [vp] * 12 + [vp]
    L.tpamd_planner_set_download_ik_table.argtypes = [vp, i, vp, vp, vp, i]
    for name in ("tpamd_planner_set_append_ik_rows", "tpamd_planner_set_append_ik_rows_device",
                 "tpamd_planner_set_plan_streaming", "tpamd_planner_set_plan_resume",
                 "tpamd_sample_ik_target_rows_host", "tpamd_sample_ik_target_rows_device"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_append_ik_rows.argtypes = [vp, i] + [vp] * 4
    L.tpamd_planner_set_append_ik_rows_device.argtypes = [vp, i] + [vp] * 4 + [vp]
    L.tpamd_planner_set_plan_streaming.argtypes = [vp] + [vp] * 6
    L.tpamd_planner_set_plan_resume.argtypes = [vp] + [vp] * 4
    for name in ("tpamd_planner_set_discard_ik_rows", "tpamd_planner_set_ik_table_info",
                 "tpamd_planner_set_download_ik_rows", "tpamd_planner_set_ik_table_device_pointers"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_discard_ik_rows.argtypes = [vp, i, vp, vp, vp]
    L.tpamd_planner_set_ik_table_info.argtypes = [vp, i, vp, vp, vp]
    L.tpamd_planner_set_download_ik_rows.argtypes = [vp, i, vp, vp, vp, vp, i]
    L.tpamd_planner_set_ik_table_device_pointers.argtypes = [vp, vp, vp]
    L.tpamd_sample_ik_target_rows_host.argtypes = [vp, i, i] + [vp] * 10
    L.tpamd_sample_ik_target_rows_device.argtypes = [vp, i, i] + [vp] * 10 + [vp]
    L.tpamd_planner_set_create.argtypes = [vp, C.POINTER(_PlannerSetConfig), C.POINTER(vp)]
    L.tpamd_planner_set_destroy.restype = None
    L.tpamd_planner_set_destroy.argtypes = [vp]
    L.tpamd_planner_set_upload_paths.argtypes = [vp, i] + [vp] * 8
    L.tpamd_planner_set_upload_paths_ragged.argtypes = [vp, i] + [vp] * 9
    L.tpamd_planner_set_download_path.argtypes = [vp, i, vp, vp, vp, i]
    L.tpamd_planner_set_reset.argtypes = [vp, i, vp]
    L.tpamd_planner_set_plan.argtypes = [vp, vp, vp, vp]
    for name in ("tpamd_planner_set_reserve", "tpamd_planner_set_capacity", "tpamd_planner_set_plan_device"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_reserve.argtypes = [vp, i, i]
    L.tpamd_planner_set_capacity.argtypes = [vp, vp, vp]
    L.tpamd_planner_set_plan_device.argtypes = [vp, vp, vp, i, vp, vp, vp]
    L.tpamd_planner_set_download_trajectory.argtypes = [vp, i, i, i] + [vp] * 7
    L.tpamd_planner_set_switch_paths.argtypes = [vp, i] + [vp] * 8
    L.tpamd_planner_set_set_waypoints.argtypes = [vp, i, vp, vp, vp, C.c_double] + [vp] * 6
    L.tpamd_planner_set_set_waypoints_device.argtypes = [vp, i, vp, vp, vp, C.c_double] + [vp] * 6 + [vp]
    for name in ("tpamd_planner_set_switch_paths_rounded", "tpamd_planner_set_retarget",
                 "tpamd_planner_set_retarget_device", "tpamd_compute_stopping_points_host",
                 "tpamd_compute_stopping_points_device", "tpamd_project_points_on_paths_host",
                 "tpamd_project_points_on_paths_device"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_switch_paths_rounded.argtypes = [vp, i] + [vp] * 5 + [C.c_double] + [vp] * 3
    L.tpamd_planner_set_retarget.argtypes = [vp, i] + [vp] * 4 + [C.c_double] + [vp] * 9
    L.tpamd_planner_set_retarget_device.argtypes = [vp, i] + [vp] * 4 + [C.c_double] + [vp] * 9 + [vp]
    L.tpamd_compute_stopping_points_host.argtypes = [vp, i, i] + [vp] * 6
    L.tpamd_compute_stopping_points_device.argtypes = [vp, i, i] + [vp] * 6 + [vp]
    L.tpamd_project_points_on_paths_host.argtypes = [vp, i, i] + [vp] * 8
    L.tpamd_project_points_on_paths_device.argtypes = [vp, i, i] + [vp] * 8 + [vp]
    for name in ("tpamd_planner_set_state_info", "tpamd_planner_set_export_state_host",
                 "tpamd_planner_set_export_state_device", "tpamd_planner_set_import_state_host",
                 "tpamd_planner_set_import_state_device", "tpamd_planner_set_copy_planners"):
        getattr(L, name).restype = i
    L.tpamd_planner_set_state_info.argtypes = [vp, i, vp, vp]
    L.tpamd_planner_set_state_bytes_bound.restype = C.c_size_t
    L.tpamd_planner_set_state_bytes_bound.argtypes = [vp]
    L.tpamd_planner_set_export_state_host.argtypes = [vp, i] + [vp] * 4
    L.tpamd_planner_set_export_state_device.argtypes = [vp, i] + [vp] * 4 + [vp]
    L.tpamd_planner_set_import_state_host.argtypes = [vp, i] + [vp] * 5
    L.tpamd_planner_set_import_state_device.argtypes = [vp, i] + [vp] * 5 + [vp]
    L.tpamd_planner_set_copy_planners.argtypes = [vp, vp, vp, vp, i, vp, vp]
    L.tpamd_planner_set_last_plan_bytes.restype = None
    L.tpamd_planner_set_last_plan_bytes.argtypes = [vp, vp, vp]
    L.tpamd_planner_set_device_bytes.restype = C.c_size_t
    L.tpamd_planner_set_device_bytes.argtypes = [vp]
    L.tpamd_debug_copy_boundary.restype = i
    L.tpamd_debug_copy_boundary.argtypes = [vp, i, i] + [vp] * 6
    L.tpamd_debug_keep_boundary.argtypes = [vp, i]
    L.tpamd_debug_copy_diag.restype = i
    L.tpamd_debug_copy_diag.argtypes = [vp, i, vp]
    L.tpamd_debug_copy_diag_ext.restype = i
    L.tpamd_debug_copy_diag_ext.argtypes = [vp, i, vp]
    L.tpamd_debug_kernel_vgprs.restype = i
    L.tpamd_debug_kernel_vgprs.argtypes = [vp, i]
    L.tpamd_rebuild_time_device.restype = i
    L.tpamd_rebuild_time_device.argtypes = [vp, i, i, i, C.c_size_t, vp, vp, vp, vp, vp, vp]
    L.tpamd_profile_reset.argtypes = [vp]
    L.tpamd_profile_enable.argtypes = [vp, i]
    L.tpamd_profile_mean_ms.restype = C.c_double
    L.tpamd_profile_mean_ms.argtypes = [vp, i, C.POINTER(i)]
    L.tpamd_profile_kernel_name.restype = C.c_char_p
    L.tpamd_profile_kernel_name.argtypes = [i]
    L.tpamd_profile_num_kernels.restype = i
    _LIB = L
    return L


def _check(rc, what):
    if rc != 0:
        raise TpamdError("%s failed: %d (%s)" % (what, rc,
                                                load_library().tpamd_error_string(rc).decode()))


def _ptr(t):
    """Device/host pointer of a torch tensor or numpy array (None -> NULL)."""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        assert t.flags["C_CONTIGUOUS"]
        return t.ctypes.data
    assert t.is_contiguous()
    return t.data_ptr()


def _int32_array(t, n, name):
    """A contiguous int32 array of n entries (torch tensor or numpy array), as the C-ABI reads it."""
    if isinstance(t, np.ndarray):
        if t.dtype != np.int32:
            raise TpamdError("%s must be int32" % name)
        t = np.ascontiguousarray(t)
    else:
        import torch
        if t.dtype != torch.int32:
            raise TpamdError("%s must be int32" % name)
        t = t.contiguous()
    if tuple(t.shape) != (n,):
        raise TpamdError("%s must have shape (%d,)" % (name, n))
    return t


class Engine:
    """One engine per GPU (tpamd_engine_create/destroy)."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.tpamd_engine_create(int(device), C.byref(h)), "tpamd_engine_create")
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tpamd_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reserve(self, num_paths, num_samples, num_rows):
        _check(self._lib.tpamd_engine_reserve(self._h, num_paths, num_samples, num_rows),
               "tpamd_engine_reserve")

    def set_pipelining(self, mode=1):
        """0 off; 1: the sampling/LP kernel of a joint solve overlaps the previous solve's sweep;
        2: sweeps of consecutive solves overlap as well, outputs ordered by the next call or
        fence() (include/tpamd.h tpamd_engine_set_pipelining: inputs must be ready at call time)."""
        _check(self._lib.tpamd_engine_set_pipelining(self._h, int(mode)),
               "tpamd_engine_set_pipelining")

    def fence(self, stream=None):
        """Order `stream` (default: torch's current stream) behind every solve issued so far."""
        _check(self._lib.tpamd_engine_fence(self._h, _stream_ptr(stream)), "tpamd_engine_fence")

    @property
    def workspace_bytes(self):
        return self._lib.tpamd_engine_workspace_bytes(self._h)

    # ------------------------------------------------------------ joint paths
    def time_joint_paths(self, inputs, outputs, num_samples, safety=0.8, max_solver_loops=0,
                         stream=None, host=False):
        """inputs: dict with knots [B][P+3], control_points [B][P][D], max_velocity,
        max_acceleration [B][D], path_start, delta, sd_start, time_start [B] (+ optional
        sdd_start). outputs: dict with time, s, sd, sdd [B][N], status [B] int32 and optional
        q, qd, qdd [B][N][D], last_extremal_index [B] int32, max_time_increment [B].
        Torch CUDA tensors (host=False) or numpy arrays (host=True)."""
        cp = inputs["control_points"]
        B, P, D = cp.shape
        bt = _JointBatch(B, D, int(num_samples), P, int(max_solver_loops), 0, float(safety))
        ji = _JointInputs(*[_ptr(inputs.get(k)) for k in (
            "knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
            "sd_start", "sdd_start", "time_start", "num_samples_per_path")])
        po = _PathOutputs(*[_ptr(outputs.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
            "max_time_increment", "status", "sd2")])
        if host:
            _check(self._lib.tpamd_time_joint_paths_host(self._h, C.byref(bt), C.byref(ji),
                                                         C.byref(po)),
                   "tpamd_time_joint_paths_host")
        else:
            _check(self._lib.tpamd_time_joint_paths_device(self._h, C.byref(bt), C.byref(ji),
                                                           C.byref(po), _stream_ptr(stream)),
                   "tpamd_time_joint_paths_device")

    def time_joint_groups(self, groups, stream=None, host=False):
        """Several joint batches side by side (tpamd_time_joint_groups_*): `groups` is a list of
        dicts with keys inputs, outputs, num_samples and optional safety, max_solver_loops -- each
        what time_joint_paths takes."""
        G = len(groups)
        bts, jis, pos = (_JointBatch * G)(), (_JointInputs * G)(), (_PathOutputs * G)()
        for g, grp in enumerate(groups):
            cp = grp["inputs"]["control_points"]
            B, P, D = cp.shape
            bts[g] = _JointBatch(B, D, int(grp["num_samples"]), P, int(grp.get("max_solver_loops", 0)),
                                 0, float(grp.get("safety", 0.8)))
            jis[g] = _JointInputs(*[_ptr(grp["inputs"].get(k)) for k in (
                "knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
                "sd_start", "sdd_start", "time_start", "num_samples_per_path")])
            pos[g] = _PathOutputs(*[_ptr(grp["outputs"].get(k)) for k in (
                "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
                "max_time_increment", "status", "sd2")])
        if host:
            _check(self._lib.tpamd_time_joint_groups_host(self._h, G, bts, jis, pos),
                   "tpamd_time_joint_groups_host")
        else:
            _check(self._lib.tpamd_time_joint_groups_device(self._h, G, bts, jis, pos,
                                                            _stream_ptr(stream)),
                   "tpamd_time_joint_groups_device")

    def sample_joint_paths(self, knots, control_points, path_start, delta, num_samples):
        """Host numpy arrays -> (q, q1, q2) [B][N][D]."""
        cp = np.ascontiguousarray(control_points, dtype=np.float64)
        kn = np.ascontiguousarray(knots, dtype=np.float64)
        B, P, D = cp.shape
        ps = np.ascontiguousarray(np.broadcast_to(path_start, (B,)), dtype=np.float64)
        dl = np.ascontiguousarray(np.broadcast_to(delta, (B,)), dtype=np.float64)
        out = [np.zeros((B, num_samples, D)) for _ in range(3)]
        _check(self._lib.tpamd_sample_joint_paths_host(
            self._h, B, D, int(num_samples), P, _ptr(kn), _ptr(cp), _ptr(ps), _ptr(dl),
            _ptr(out[0]), _ptr(out[1]), _ptr(out[2])), "tpamd_sample_joint_paths_host")
        return tuple(out)

    # ------------------------------------------------------- constraint rows
    def optimize_rows(self, inputs, outputs, max_solver_loops=0, stream=None, host=False,
                      num_samples_per_path=None):
        """num_samples_per_path [B] int32 (a tensor on the device, or a numpy array with host=True):
        a ragged batch, path b has that many samples in arrays of stride N
        (tpamd_optimize_rows_ragged_*)."""
        a = inputs["a"]
        B, N, Cn = a.shape
        bt = _RowsBatch(B, N, Cn, int(max_solver_loops))
        ri = _RowsInputs(*[_ptr(inputs.get(k)) for k in (
            "a", "b", "lower", "upper", "s_start", "s_end", "sd_start", "sdd_start",
            "time_start")])
        po = _PathOutputs(*[_ptr(outputs.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
            "max_time_increment", "status", "sd2")])
        if num_samples_per_path is not None:
            ns = _int32_array(num_samples_per_path, B, "num_samples_per_path")
            if host:
                _check(self._lib.tpamd_optimize_rows_ragged_host(self._h, C.byref(bt), C.byref(ri), _ptr(ns),
                                                                 C.byref(po)),
                       "tpamd_optimize_rows_ragged_host")
            else:
                _check(self._lib.tpamd_optimize_rows_ragged_device(self._h, C.byref(bt), C.byref(ri), _ptr(ns),
                                                                   C.byref(po), _stream_ptr(stream)),
                       "tpamd_optimize_rows_ragged_device")
            return
        if host:
            _check(self._lib.tpamd_optimize_rows_host(self._h, C.byref(bt), C.byref(ri),
                                                      C.byref(po)), "tpamd_optimize_rows_host")
        else:
            _check(self._lib.tpamd_optimize_rows_device(self._h, C.byref(bt), C.byref(ri),
                                                        C.byref(po), _stream_ptr(stream)),
                   "tpamd_optimize_rows_device")

    # ------------------------------------------------------- Cartesian paths
    def time_cartesian_paths(self, inputs, outputs, safety=0.8, max_solver_loops=0, stream=None,
                             host=False, num_samples_per_path=None, first_row=None):
        """inputs: ik_positions [B][N][D], jacobians [B][N][6][D], max_velocity,
        max_acceleration [B][D], max_translational_velocity, max_rotational_velocity,
        path_start, delta, sd_start, time_start [B] (+ optional sdd_start). outputs as for
        time_joint_paths (q, if given, receives the IK positions).

        Ragged batches (tpamd_time_cartesian_paths_ragged_*): num_samples_per_path [B] int32 gives
        path b its own sample count in arrays of stride N. With first_row [B] int32 the inputs are
        packed row tables, ik_positions [rows][D] and jacobians [rows][6][D], path b reading rows
        first_row[b] .. first_row[b] + n[b] - 1 (what sample_ik_targets writes, first_row =
        row_offsets[:B]); B and the stride N are then those of outputs["time"] [B][N]. first_row
        alone means every path has N samples. Both are device tensors, or numpy arrays with
        host=True."""
        ik = inputs["ik_positions"]
        if num_samples_per_path is not None or first_row is not None:
            if first_row is None:
                B, N, D = ik.shape
            else:
                if len(ik.shape) != 2:
                    raise TpamdError("packed inputs: ik_positions must be [rows][D]")
                rows, D = ik.shape
                B, N = outputs["time"].shape
                if inputs["jacobians"].shape[0] != rows:
                    raise TpamdError("packed inputs: jacobians must have one [6][D] block per row")
            if num_samples_per_path is None:
                if host:
                    num_samples_per_path = np.full(B, N, dtype=np.int32)
                else:
                    import torch
                    num_samples_per_path = torch.full((B,), N, dtype=torch.int32, device=ik.device)
            ns = _int32_array(num_samples_per_path, B, "num_samples_per_path")
            fr = None if first_row is None else _int32_array(first_row, B, "first_row")
            bt = _CartesianBatch(B, D, N, int(max_solver_loops), float(safety))
            ci = _CartesianInputs(*[_ptr(inputs.get(k)) for k in _CARTESIAN_INPUT_KEYS])
            po = _PathOutputs(*[_ptr(outputs.get(k)) for k in (
                "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
                "max_time_increment", "status", "sd2")])
            if host:
                _check(self._lib.tpamd_time_cartesian_paths_ragged_host(
                    self._h, C.byref(bt), C.byref(ci), _ptr(ns), _ptr(fr),
                    int(ik.shape[0]) if fr is not None else 0, C.byref(po)),
                    "tpamd_time_cartesian_paths_ragged_host")
            else:
                _check(self._lib.tpamd_time_cartesian_paths_ragged_device(
                    self._h, C.byref(bt), C.byref(ci), _ptr(ns), _ptr(fr), C.byref(po), _stream_ptr(stream)),
                    "tpamd_time_cartesian_paths_ragged_device")
                # the engine reads the two arrays until the stream has run the call
                self._ragged_keepalive = (ns, fr)
            return
        B, N, D = ik.shape
        bt = _CartesianBatch(B, D, N, int(max_solver_loops), float(safety))
        ci = _CartesianInputs(*[_ptr(inputs.get(k)) for k in _CARTESIAN_INPUT_KEYS])
        po = _PathOutputs(*[_ptr(outputs.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
            "max_time_increment", "status", "sd2")])
        if host:
            _check(self._lib.tpamd_time_cartesian_paths_host(self._h, C.byref(bt), C.byref(ci),
                                                             C.byref(po)),
                   "tpamd_time_cartesian_paths_host")
        else:
            _check(self._lib.tpamd_time_cartesian_paths_device(self._h, C.byref(bt), C.byref(ci),
                                                               C.byref(po), _stream_ptr(stream)),
                   "tpamd_time_cartesian_paths_device")

    def sample_pose_splines(self, knots, translation_points, rotation_points, path_start, delta,
                            num_samples):
        """Host numpy arrays: knots [B][P+3], translation [B][P][3], rotation [B][P][4] (w, x, y,
        z) -> poses [B][N][7] (tpamd_sample_pose_splines_host)."""
        kn = np.ascontiguousarray(knots, dtype=np.float64)
        tr = np.ascontiguousarray(translation_points, dtype=np.float64)
        ro = np.ascontiguousarray(rotation_points, dtype=np.float64)
        B, P, _ = tr.shape
        ps = np.ascontiguousarray(np.broadcast_to(path_start, (B,)), dtype=np.float64)
        dl = np.ascontiguousarray(np.broadcast_to(delta, (B,)), dtype=np.float64)
        out = np.zeros((B, int(num_samples), 7))
        _check(self._lib.tpamd_sample_pose_splines_host(self._h, B, int(num_samples), P, _ptr(kn),
                                                        _ptr(tr), _ptr(ro), _ptr(ps), _ptr(dl),
                                                        _ptr(out)), "tpamd_sample_pose_splines_host")
        return out

    # ------------------------------------------------------------ Cartesian goals
    def fit_pose_waypoints(self, pose_waypoints, joint_waypoints, offsets, translation_rounding=0.05,
                           rotation_rounding=0.2, stream=None):
        """TimeableCartesianSplinePath::SetWaypoints for B paths (tpamd_fit_pose_waypoints_*): path k
        takes rows offsets[k]:offsets[k + 1] of pose_waypoints [rows][7] (translation, then the
        quaternion w, x, y, z) and joint_waypoints [rows][D]; the roundings are [B] (or one number).
        Returns a dict: knots, translation_points [sum P][3], rotation_points [sum P][4],
        joint_control_points [sum P][D] (packed raggedly), num_points, path_end, status [B] and
        point_offsets [B + 1] (always a numpy array). CUDA inputs go through the _device entry on
        `stream` (default: torch's current stream) and give CUDA tensors; numpy arrays go through
        the host entry, which synchronises, and give numpy arrays."""
        import torch
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        B = off.shape[0] - 1
        if B < 0:
            raise TpamdError("waypoint offsets need at least one entry")
        W = np.diff(off.astype(np.int64))
        npts = np.where(W < 1, 0, np.where(W == 1, 4, 3 * W - 2))
        P, K = int(npts.sum()), int((npts + 3 * (npts > 0)).sum())
        rows = int(off[-1])
        point_offsets = np.zeros(B + 1, dtype=np.int32)
        if _is_cuda(pose_waypoints):
            dev = pose_waypoints.device
            f = lambda x, shape, what: PlannerSet._cuda(x, torch.float64, dev, shape, what)
            per = lambda x, what: f(x if hasattr(x, "shape") else torch.full((B,), float(x), dtype=torch.float64),
                                    (B,), what)
            pw = f(pose_waypoints, (rows, 7), "pose_waypoints")
            D = int(joint_waypoints.shape[-1])
            jw = f(joint_waypoints, (rows, D), "joint_waypoints")
            tr, rr = per(translation_rounding, "translation_rounding"), per(rotation_rounding, "rotation_rounding")
            new = lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
            out = dict(knots=new((K,)), translation_points=new((P, 3)), rotation_points=new((P, 4)),
                       joint_control_points=new((P, D)), num_points=new((B,), torch.int32), path_end=new((B,)),
                       status=torch.full((B,), -1, dtype=torch.int32, device=dev))
            _check(self._lib.tpamd_fit_pose_waypoints_device(
                self._h, B, D, _ptr(off), _ptr(pw), _ptr(jw), _ptr(tr), _ptr(rr), _ptr(out["knots"]),
                _ptr(out["translation_points"]), _ptr(out["rotation_points"]), _ptr(out["joint_control_points"]),
                _ptr(out["num_points"]), _ptr(point_offsets), _ptr(out["path_end"]), _ptr(out["status"]),
                _stream_ptr(stream)), "tpamd_fit_pose_waypoints_device")
        else:
            pw = _host(pose_waypoints, np.float64, (rows, 7), "pose_waypoints")
            jw = _host(joint_waypoints, np.float64, what="joint_waypoints")
            if jw.ndim != 2 or jw.shape[0] != rows:
                raise TpamdError("joint_waypoints has shape %s, expected (%d, D)" % (jw.shape, rows))
            D = jw.shape[1]
            per = lambda x, what: _host(np.broadcast_to(_host(x, np.float64), (B,)), np.float64, (B,), what)
            tr, rr = per(translation_rounding, "translation_rounding"), per(rotation_rounding, "rotation_rounding")
            out = dict(knots=np.zeros(K), translation_points=np.zeros((P, 3)), rotation_points=np.zeros((P, 4)),
                       joint_control_points=np.zeros((P, D)), num_points=np.zeros(B, dtype=np.int32),
                       path_end=np.zeros(B), status=np.full(B, -1, dtype=np.int32))
            _check(self._lib.tpamd_fit_pose_waypoints_host(
                self._h, B, D, _ptr(off), _ptr(pw), _ptr(jw), _ptr(tr), _ptr(rr), _ptr(out["knots"]),
                _ptr(out["translation_points"]), _ptr(out["rotation_points"]), _ptr(out["joint_control_points"]),
                _ptr(out["num_points"]), _ptr(point_offsets), _ptr(out["path_end"]), _ptr(out["status"])),
                "tpamd_fit_pose_waypoints_host")
        out["point_offsets"] = point_offsets
        return out

    # ------------------------------------------------------------ waypoint batches
    def fit_joint_waypoints(self, waypoints, offsets, rounding=None, stream=None):
        """TimeableJointSplinePath::SetWaypoints for B paths (tpamd_fit_joint_waypoints_*): path k takes
        rows offsets[k]:offsets[k + 1] of waypoints [rows][D]; rounding is [B], one number, or None
        (0.2). Returns a dict: knots, control_points [sum P][D] (packed raggedly), num_points,
        path_end, status [B] (TPAMD_PLAN_*) and point_offsets [B + 1] (always a numpy array). CUDA
        waypoints go through the _device entry on `stream` (default: torch's current stream) and give
        CUDA tensors; numpy arrays go through the host entry, which synchronises, and give numpy
        arrays."""
        import torch
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        B = off.shape[0] - 1
        if B < 0:
            raise TpamdError("waypoint offsets need at least one entry")
        W = np.diff(off.astype(np.int64))
        npts = np.where(W < 1, 0, np.where(W == 1, 4, 3 * W - 2))
        P, K = int(npts.sum()), int((npts + 3 * (npts > 0)).sum())
        rows = int(off[-1])
        if waypoints.ndim != 2 or waypoints.shape[0] != rows:
            raise TpamdError("waypoints has shape %s, expected (%d, D)" % (tuple(waypoints.shape), rows))
        D = int(waypoints.shape[1])
        point_offsets = np.zeros(B + 1, dtype=np.int32)
        if _is_cuda(waypoints):
            dev = waypoints.device
            w = PlannerSet._cuda(waypoints, torch.float64, dev, (rows, D), "waypoints")
            r = None
            if rounding is not None:
                r = PlannerSet._cuda(rounding if hasattr(rounding, "shape") and len(rounding.shape) else
                                     torch.full((B,), float(rounding), dtype=torch.float64), torch.float64, dev, (B,),
                                     "rounding")
            new = lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
            out = dict(knots=new((K,)), control_points=new((P, D)), num_points=new((B,), torch.int32),
                       path_end=new((B,)), status=torch.full((B,), -1, dtype=torch.int32, device=dev))
            _check(self._lib.tpamd_fit_joint_waypoints_device(
                self._h, B, D, _ptr(off), _ptr(w), _ptr(r), _ptr(out["knots"]), _ptr(out["control_points"]),
                _ptr(out["num_points"]), _ptr(point_offsets), _ptr(out["path_end"]), _ptr(out["status"]),
                _stream_ptr(stream)), "tpamd_fit_joint_waypoints_device")
        else:
            w = _host(waypoints, np.float64, (rows, D), "waypoints")
            r = None if rounding is None else _host(np.broadcast_to(_host(rounding, np.float64), (B,)), np.float64,
                                                    (B,), "rounding")
            out = dict(knots=np.zeros(K), control_points=np.zeros((P, D)), num_points=np.zeros(B, dtype=np.int32),
                       path_end=np.zeros(B), status=np.full(B, -1, dtype=np.int32))
            _check(self._lib.tpamd_fit_joint_waypoints_host(
                self._h, B, D, _ptr(off), _ptr(w), _ptr(r), _ptr(out["knots"]), _ptr(out["control_points"]),
                _ptr(out["num_points"]), _ptr(point_offsets), _ptr(out["path_end"]), _ptr(out["status"])),
                "tpamd_fit_joint_waypoints_host")
        out["point_offsets"] = point_offsets
        return out

    def _waypoint_io(self, waypoints, offsets, max_velocity, max_acceleration, num_samples, num_samples_per_path,
                     delta, rounding, sd_start, time_start, safety, outputs, host):
        """The C structs of one waypoint timing call (plain or refined), the dict it returns, the
        device of the arrays (None with host=True) and what must stay alive until the call is made."""
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        B = off.shape[0] - 1
        if B < 0:
            raise TpamdError("waypoint offsets need at least one entry")
        N, D = int(num_samples), int(max_velocity.shape[-1])
        out = dict(outputs) if outputs else {}
        if host:
            f = lambda x, shape, what, dt=np.float64: _host(x, dt, shape, what)
            new = lambda shape, dt=np.float64: np.zeros(shape, dtype=dt)
            i32 = np.int32
            dev = None
        else:
            import torch
            dev = max_velocity.device
            f = lambda x, shape, what, dt=torch.float64: None if x is None else PlannerSet._cuda(x, dt, dev, shape, what)
            new = lambda shape, dt=torch.float64: torch.zeros(shape, dtype=dt, device=dev)
            i32 = torch.int32
        rows = int(off[-1])
        w = f(waypoints, (rows, D), "waypoints")
        vm, am = f(max_velocity, (B, D), "max_velocity"), f(max_acceleration, (B, D), "max_acceleration")
        ns = f(num_samples_per_path, (B,), "num_samples_per_path", i32)
        dl, rd = f(delta, (B,), "delta"), f(rounding, (B,), "rounding")
        sd0, t0 = f(sd_start, (B,), "sd_start"), f(time_start, (B,), "time_start")
        for k in ("time", "s", "sd", "sdd"):
            out.setdefault(k, new((B, N)))
        for k in ("q", "qd", "qdd"):
            out.setdefault(k, new((B, N, D)))
        for k in ("status", "last_extremal_index", "num_points"):
            out.setdefault(k, new((B,), i32))
        for k in ("max_time_increment", "path_end", "delta_used"):
            out.setdefault(k, new((B,)))
        bt = _WaypointBatch(B, D, N, 0, float(safety))
        wi = _WaypointInputs(_ptr(off), _ptr(w), _ptr(rd), _ptr(vm), _ptr(am), _ptr(ns), _ptr(dl), _ptr(sd0),
                             _ptr(t0))
        po = _PathOutputs(*[_ptr(out.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index", "max_time_increment", "status",
            "sd2")])
        fo = _WaypointFitOutputs(*[_ptr(out.get(k)) for k in (
            "num_points", "path_end", "delta_used", "knots", "control_points")])
        return bt, wi, po, fo, out, B, D, dev, (off, w, vm, am, ns, dl, rd, sd0, t0)

    def time_waypoint_paths(self, waypoints, offsets, max_velocity, max_acceleration, num_samples,
                            num_samples_per_path=None, delta=None, rounding=None, sd_start=None, time_start=None,
                            safety=0.8, outputs=None, stream=None, host=False):
        """Waypoints in, trajectories out (tpamd_time_waypoint_paths_*): path k takes rows
        offsets[k]:offsets[k + 1] of waypoints [rows][D] (offsets: host int32 [B + 1]), is fitted on the
        device and timed from path parameter 0 with num_samples_per_path[k] samples (None: num_samples
        each) at delta[k] (None: the samples cover exactly the whole path). max_velocity and
        max_acceleration are [B][D]; rounding, sd_start and time_start [B] or None (0.2, 0, 0).
        Torch CUDA tensors on `stream` (host=False; nothing synchronises unless the engine's scratch
        grows) or numpy arrays (host=True). Returns a dict with time, s, sd, sdd [B][N], q, qd, qdd
        [B][N][D], status, last_extremal_index, num_points [B] int32 and max_time_increment, path_end,
        delta_used [B] -- the arrays of `outputs` where it has them (also knots [B][S + 3] and
        control_points [B][S][D], S = max(3 max W - 2, 4), filled only if given), new ones otherwise.
        A path without waypoints gets status 11 (PATH_STATUS) and nothing else of it is written."""
        bt, wi, po, fo, out, B, D, dev, keep = self._waypoint_io(
            waypoints, offsets, max_velocity, max_acceleration, num_samples, num_samples_per_path, delta, rounding,
            sd_start, time_start, safety, outputs, host)
        if host:
            _check(self._lib.tpamd_time_waypoint_paths_host(self._h, C.byref(bt), C.byref(wi), C.byref(po),
                                                            C.byref(fo)), "tpamd_time_waypoint_paths_host")
        else:
            _check(self._lib.tpamd_time_waypoint_paths_device(self._h, C.byref(bt), C.byref(wi), C.byref(po),
                                                              C.byref(fo), _stream_ptr(stream)),
                   "tpamd_time_waypoint_paths_device")
        return out

    # ------------------------------------------- refining violating paths on the device
    def _refine_io(self, B, D, max_rounds, max_samples, max_refined, tolerance, refined, device, host):
        """The tpamd_refine_options / tpamd_refine_outputs of one refined call and the dict it
        returns: check and refined_check (dicts of violations, worst_excess, worst_sample, worst_row,
        first_sample, [B] and [M]), slot [B], slot_path, rounds, num_samples, delta [M], num_refined
        [1], and refined (a dict as time_joint_paths fills, [M][max_samples](..[D]), with sd2). The
        arrays of `refined` (the same nesting) where it has them, new zero-filled ones otherwise
        (refined status: -1). Unused slots and the entries behind a slot's num_samples are not written:
        read slot_path[k] >= 0 and num_samples[k] before anything of slot k."""
        M, NS = int(max_refined), int(max_samples)
        if host:
            new = lambda shape, real=True: np.zeros(shape, dtype=np.float64 if real else np.int32)
        else:
            import torch
            new = lambda shape, real=True: torch.zeros(shape, dtype=torch.float64 if real else torch.int32,
                                                       device=device)
        src = refined or {}
        out = {k: v for k, v in src.items() if k not in ("check", "refined", "refined_check")}
        for name, n in (("check", B), ("refined_check", M)):
            rec = dict(src.get(name) or {})
            for k in _CHECK_OUTPUT_KEYS:
                rec.setdefault(k, new((n,), k == "worst_excess"))
            out[name] = rec
        out.setdefault("slot", new((B,), False))
        for k in ("slot_path", "rounds", "num_samples"):
            out.setdefault(k, new((M,), False))
        out.setdefault("num_refined", new((1,), False))
        out.setdefault("delta", new((M,)))
        sol = dict(src.get("refined") or {})
        for k in ("time", "s", "sd", "sdd", "sd2"):
            sol.setdefault(k, new((M, NS)))
        for k in ("q", "qd", "qdd"):
            sol.setdefault(k, new((M, NS, D)))
        if "status" not in sol:
            sol["status"] = new((M,), False) - 1    # an unused slot is not written: -1, not TPAMD_PATH_OK
        sol.setdefault("last_extremal_index", new((M,), False))
        sol.setdefault("max_time_increment", new((M,)))
        out["refined"] = sol
        ro = _RefineOutputs()
        ro.check = _CheckOutputs(*[_ptr(out["check"].get(k)) for k in _CHECK_OUTPUT_KEYS])
        for k in ("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta"):
            setattr(ro, k, _ptr(out.get(k)))
        ro.refined = _PathOutputs(*[_ptr(sol.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index", "max_time_increment", "status",
            "sd2")])
        ro.refined_check = _CheckOutputs(*[_ptr(out["refined_check"].get(k)) for k in _CHECK_OUTPUT_KEYS])
        opt = _RefineOptions(int(max_rounds), NS, M, 0, float(tolerance))
        return opt, ro, out

    def time_joint_paths_refined(self, inputs, outputs, num_samples, max_rounds, max_samples, max_refined,
                                 tolerance=0.0, safety=0.8, refined=None, stream=None, host=False):
        """time_joint_paths, its check, and up to max_rounds re-timings of the violating paths at
        doubled sample counts, in one call (tpamd_time_joint_paths_refined_*). `outputs` receives
        exactly what time_joint_paths writes. A path with violated rows whose worst excess lies above
        `tolerance` and whose 2 n - 1 samples fit max_samples takes one of max_refined slots, in
        ascending path order; slot[b] is the slot, or -1 (nothing to refine), -2 (no slot left), -3
        (too long). Returns the dict _refine_io describes. Refinement may end with violations left:
        read refined_check."""
        cp = inputs["control_points"]
        B, P, D = cp.shape
        bt = _JointBatch(B, D, int(num_samples), P, 0, 0, float(safety))
        ji = _JointInputs(*[_ptr(inputs.get(k)) for k in (
            "knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
            "sd_start", "sdd_start", "time_start", "num_samples_per_path")])
        po = _PathOutputs(*[_ptr(outputs.get(k)) for k in (
            "time", "s", "sd", "sdd", "q", "qd", "qdd", "last_extremal_index",
            "max_time_increment", "status", "sd2")])
        opt, ro, out = self._refine_io(B, D, max_rounds, max_samples, max_refined, tolerance, refined,
                                       None if host else cp.device, host)
        if host:
            _check(self._lib.tpamd_time_joint_paths_refined_host(self._h, C.byref(bt), C.byref(ji), C.byref(po),
                                                                 C.byref(opt), C.byref(ro)),
                   "tpamd_time_joint_paths_refined_host")
        else:
            _check(self._lib.tpamd_time_joint_paths_refined_device(self._h, C.byref(bt), C.byref(ji), C.byref(po),
                                                                   C.byref(opt), C.byref(ro), _stream_ptr(stream)),
                   "tpamd_time_joint_paths_refined_device")
        return out

    def time_waypoint_paths_refined(self, waypoints, offsets, max_velocity, max_acceleration, num_samples,
                                    max_rounds, max_samples, max_refined, tolerance=0.0, num_samples_per_path=None,
                                    delta=None, rounding=None, sd_start=None, time_start=None, safety=0.8,
                                    outputs=None, refined=None, stream=None, host=False):
        """time_waypoint_paths with the refinement of time_joint_paths_refined
        (tpamd_time_waypoint_paths_refined_*). Returns (what time_waypoint_paths returns, the refine
        outputs)."""
        bt, wi, po, fo, out, B, D, dev, keep = self._waypoint_io(
            waypoints, offsets, max_velocity, max_acceleration, num_samples, num_samples_per_path, delta, rounding,
            sd_start, time_start, safety, outputs, host)
        opt, ro, ref = self._refine_io(B, D, max_rounds, max_samples, max_refined, tolerance, refined, dev, host)
        if host:
            _check(self._lib.tpamd_time_waypoint_paths_refined_host(
                self._h, C.byref(bt), C.byref(wi), C.byref(po), C.byref(fo), C.byref(opt), C.byref(ro)),
                "tpamd_time_waypoint_paths_refined_host")
        else:
            _check(self._lib.tpamd_time_waypoint_paths_refined_device(
                self._h, C.byref(bt), C.byref(wi), C.byref(po), C.byref(fo), C.byref(opt), C.byref(ro),
                _stream_ptr(stream)), "tpamd_time_waypoint_paths_refined_device")
        return out, ref

    # ------------------------------------------- checking solutions against their rows
    def _check_io(self, solution, outputs, B, like, host):
        """The tpamd_solution / tpamd_check_outputs of one check call and the dict it returns: the
        arrays of `outputs` where it has them, new ones (on the device of `like`, or numpy arrays
        with host=True) otherwise."""
        out = dict(outputs) if outputs else {}
        for k in _CHECK_OUTPUT_KEYS:
            if k in out:
                continue
            real = k == "worst_excess"
            if host:
                out[k] = np.zeros(B, dtype=np.float64 if real else np.int32)
            else:
                import torch
                out[k] = torch.zeros(B, dtype=torch.float64 if real else torch.int32, device=like.device)
        sol = _Solution(*[_ptr(solution.get(k)) for k in ("sd2", "sd", "sdd", "status")])
        cko = _CheckOutputs(*[_ptr(out.get(k)) for k in _CHECK_OUTPUT_KEYS])
        return sol, cko, out

    def check_rows(self, inputs, solution, outputs=None, num_samples_per_path=None, stream=None, host=False):
        """SolutionSatisfiesConstraints for a rows batch (tpamd_check_rows_*). inputs: the dict
        optimize_rows took (a, b, lower, upper [B][N][C] are read); solution: the outputs dict of the
        solve (sd2 or sd, sdd [B][N], status [B] or absent). Returns a dict with violations,
        worst_sample, worst_row, first_sample [B] int32 and worst_excess [B]: the arrays of `outputs`
        where it has them (an entry that is None is not computed), new ones otherwise. -1 violations:
        the path was not checked (status not ok, or a sample count the solve refuses)."""
        a = inputs["a"]
        B, N, Cn = a.shape
        bt = _RowsBatch(B, N, Cn, 0)
        ri = _RowsInputs(*[_ptr(inputs.get(k)) for k in (
            "a", "b", "lower", "upper", "s_start", "s_end", "sd_start", "sdd_start", "time_start")])
        ns = None if num_samples_per_path is None else _int32_array(num_samples_per_path, B, "num_samples_per_path")
        sol, cko, out = self._check_io(solution, outputs, B, a, host)
        if host:
            _check(self._lib.tpamd_check_rows_host(self._h, C.byref(bt), C.byref(ri), _ptr(ns), C.byref(sol),
                                                   C.byref(cko)), "tpamd_check_rows_host")
        else:
            _check(self._lib.tpamd_check_rows_device(self._h, C.byref(bt), C.byref(ri), _ptr(ns), C.byref(sol),
                                                     C.byref(cko), _stream_ptr(stream)), "tpamd_check_rows_device")
            self._check_keepalive = (ns,)
        return out

    def check_joint_paths(self, inputs, solution, num_samples, safety=0.8, num_points_per_path=None, outputs=None,
                          stream=None, host=False):
        """The same for a joint batch (tpamd_check_joint_paths_*): inputs and num_samples as
        time_joint_paths took them, ragged through inputs["num_samples_per_path"]. With
        num_points_per_path [B] int32 the knots [B][S + 3] and control_points [B][S][D] are slots of
        which path k uses its first num_points_per_path[k] entries (what time_waypoint_paths
        returns; see check_waypoint_paths)."""
        cp = inputs["control_points"]
        B, P, D = cp.shape
        bt = _JointBatch(B, D, int(num_samples), P, 0, 0, float(safety))
        ji = _JointInputs(*[_ptr(inputs.get(k)) for k in (
            "knots", "control_points", "max_velocity", "max_acceleration", "path_start", "delta",
            "sd_start", "sdd_start", "time_start", "num_samples_per_path")])
        npp = None if num_points_per_path is None else _int32_array(num_points_per_path, B, "num_points_per_path")
        sol, cko, out = self._check_io(solution, outputs, B, cp, host)
        if host:
            _check(self._lib.tpamd_check_joint_paths_host(self._h, C.byref(bt), C.byref(ji), _ptr(npp),
                                                          C.byref(sol), C.byref(cko)),
                   "tpamd_check_joint_paths_host")
        else:
            _check(self._lib.tpamd_check_joint_paths_device(self._h, C.byref(bt), C.byref(ji), _ptr(npp),
                                                            C.byref(sol), C.byref(cko), _stream_ptr(stream)),
                   "tpamd_check_joint_paths_device")
            self._check_keepalive = (npp,)
        return out

    def check_waypoint_paths(self, got, max_velocity, max_acceleration, num_samples, safety=0.8,
                             num_samples_per_path=None, outputs=None, stream=None, host=False):
        """The same for a waypoint batch, from what time_waypoint_paths returned (`got`, which must
        hold knots and control_points: pass them in its `outputs`): the slot splines with num_points,
        delta_used as delta, path_start 0, and got's sd2 (or sd), sdd and status as the solution.
        A path without waypoints is not checked."""
        for k in ("knots", "control_points", "num_points", "delta_used"):
            if got.get(k) is None:
                raise TpamdError("check_waypoint_paths needs got[%r] (ask time_waypoint_paths for it)" % k)
        dl = got["delta_used"]
        zero = np.zeros_like(dl) if isinstance(dl, np.ndarray) else dl.new_zeros(dl.shape)
        inputs = {"knots": got["knots"], "control_points": got["control_points"], "max_velocity": max_velocity,
                  "max_acceleration": max_acceleration, "path_start": zero, "delta": dl,
                  "num_samples_per_path": num_samples_per_path}
        out = self.check_joint_paths(inputs, got, num_samples, safety=safety, num_points_per_path=got["num_points"],
                                     outputs=outputs, stream=stream, host=host)
        if not host:
            self._check_keepalive += (zero,)
        return out

    def check_cartesian_paths(self, inputs, solution, safety=0.8, num_samples_per_path=None, first_row=None,
                              outputs=None, stream=None, host=False):
        """The same for a Cartesian batch (tpamd_check_cartesian_paths_*): inputs, num_samples_per_path
        and first_row as time_cartesian_paths took them. With first_row the inputs are packed row
        tables, and B and the stride N are those of solution["sdd"] [B][N]."""
        ik = inputs["ik_positions"]
        if first_row is None:
            B, N, D = ik.shape
        else:
            if len(ik.shape) != 2:
                raise TpamdError("packed inputs: ik_positions must be [rows][D]")
            rows, D = ik.shape
            B, N = solution["sdd"].shape
            if inputs["jacobians"].shape[0] != rows:
                raise TpamdError("packed inputs: jacobians must have one [6][D] block per row")
        ns = None if num_samples_per_path is None else _int32_array(num_samples_per_path, B, "num_samples_per_path")
        fr = None if first_row is None else _int32_array(first_row, B, "first_row")
        bt = _CartesianBatch(B, D, N, 0, float(safety))
        ci = _CartesianInputs(*[_ptr(inputs.get(k)) for k in _CARTESIAN_INPUT_KEYS])
        sol, cko, out = self._check_io(solution, outputs, B, ik, host)
        if host:
            _check(self._lib.tpamd_check_cartesian_paths_host(
                self._h, C.byref(bt), C.byref(ci), _ptr(ns), _ptr(fr), int(ik.shape[0]) if fr is not None else 0,
                C.byref(sol), C.byref(cko)), "tpamd_check_cartesian_paths_host")
        else:
            _check(self._lib.tpamd_check_cartesian_paths_device(
                self._h, C.byref(bt), C.byref(ci), _ptr(ns), _ptr(fr), C.byref(sol), C.byref(cko),
                _stream_ptr(stream)), "tpamd_check_cartesian_paths_device")
            self._check_keepalive = (ns, fr)
        return out

    # ------------------------------------------------------------ path_tools
    def compute_stopping_points(self, position, velocity, acceleration_limit, corner_rounding=0.2, stream=None):
        """ComputeStoppingPoint for a batch (tpamd_compute_stopping_points_*): position, velocity and
        acceleration_limit [count][D] float64, corner_rounding [count] (or one number). Returns
        (point [count][D], status [count] int32): where each robot can come to rest on the straight
        line along its velocity within the limits, shifted by the corner rounding; a row with a
        non-positive limit has status INVALID_ARGUMENT and a NaN point. CUDA inputs go through the
        _device entry on `stream` (default: torch's current stream), which only enqueues, and give
        CUDA tensors; anything else goes through the host entry, which synchronises, and gives
        numpy arrays."""
        import torch
        if _is_cuda(position):
            dev = position.device
            f = lambda x, shape, what: PlannerSet._cuda(x, torch.float64, dev, shape, what)
            pos = f(position, None, "position")
            if pos.dim() != 2:
                raise TpamdError("position has shape %s, expected (count, D)" % (tuple(pos.shape),))
            n, D = pos.shape
            vel, acc = f(velocity, (n, D), "velocity"), f(acceleration_limit, (n, D), "acceleration_limit")
            rnd = f(corner_rounding if hasattr(corner_rounding, "shape") else
                    torch.full((n,), float(corner_rounding), dtype=torch.float64), (n,), "corner_rounding")
            point = torch.full((n, D), float("nan"), dtype=torch.float64, device=dev)
            status = torch.full((n,), -1, dtype=torch.int32, device=dev)
            _check(self._lib.tpamd_compute_stopping_points_device(
                self._h, n, D, _ptr(pos), _ptr(vel), _ptr(acc), _ptr(rnd), _ptr(point), _ptr(status),
                _stream_ptr(stream)), "tpamd_compute_stopping_points_device")
            return point, status
        pos = _host(position, np.float64, what="position")
        if pos.ndim != 2:
            raise TpamdError("position has shape %s, expected (count, D)" % (pos.shape,))
        n, D = pos.shape
        vel = _host(velocity, np.float64, (n, D), "velocity")
        acc = _host(acceleration_limit, np.float64, (n, D), "acceleration_limit")
        rnd = _host(np.broadcast_to(_host(corner_rounding, np.float64), (n,)), np.float64, (n,), "corner_rounding")
        point, status = np.full((n, D), np.nan), np.full(n, -1, dtype=np.int32)
        _check(self._lib.tpamd_compute_stopping_points_host(
            self._h, n, D, _ptr(pos), _ptr(vel), _ptr(acc), _ptr(rnd), _ptr(point), _ptr(status)),
            "tpamd_compute_stopping_points_host")
        return point, status

    def project_points_on_paths(self, waypoints, offsets, point, stream=None):
        """ProjectPointOnPath for a ragged batch (tpamd_project_points_on_paths_*): list k is
        waypoints[offsets[k]:offsets[k + 1]] ([rows][D] float64), point [count][D]. Returns a dict:
        waypoint_index, status [count] int32, distance_to_path, line_parameter [count] and
        projected_point [count][D]; an empty list has status INVALID_ARGUMENT and NaN / -1 outputs.
        offsets is a host array in both forms. CUDA waypoints go through the _device entry on
        `stream`, which only enqueues, and give CUDA tensors; anything else goes through the host
        entry, which synchronises, and gives numpy arrays."""
        import torch
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        n = off.shape[0] - 1
        if n < 0:
            raise TpamdError("waypoint offsets need at least one entry")
        if _is_cuda(point):
            dev = point.device
            f = lambda x, shape, what: PlannerSet._cuda(x, torch.float64, dev, shape, what)
            pt = f(point, None, "point")
            if pt.dim() != 2 or pt.shape[0] != n:
                raise TpamdError("point has shape %s, expected (%d, D)" % (tuple(pt.shape), n))
            D = pt.shape[1]
            w = f(waypoints, (int(off[-1]), D), "waypoints")
            out = dict(waypoint_index=torch.full((n,), -1, dtype=torch.int32, device=dev),
                       distance_to_path=torch.full((n,), float("nan"), dtype=torch.float64, device=dev),
                       line_parameter=torch.full((n,), float("nan"), dtype=torch.float64, device=dev),
                       projected_point=torch.full((n, D), float("nan"), dtype=torch.float64, device=dev),
                       status=torch.full((n,), -1, dtype=torch.int32, device=dev))
            _check(self._lib.tpamd_project_points_on_paths_device(
                self._h, n, D, _ptr(off), w.data_ptr() if w.numel() else None, _ptr(pt), _ptr(out["waypoint_index"]),
                _ptr(out["distance_to_path"]), _ptr(out["line_parameter"]), _ptr(out["projected_point"]),
                _ptr(out["status"]), _stream_ptr(stream)), "tpamd_project_points_on_paths_device")
            return out
        pt = _host(point, np.float64, what="point")
        if pt.ndim != 2 or pt.shape[0] != n:
            raise TpamdError("point has shape %s, expected (%d, D)" % (pt.shape, n))
        D = pt.shape[1]
        w = _host(waypoints, np.float64, what="waypoints").reshape(-1, D)
        if w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        out = dict(waypoint_index=np.full(n, -1, dtype=np.int32), distance_to_path=np.full(n, np.nan),
                   line_parameter=np.full(n, np.nan), projected_point=np.full((n, D), np.nan),
                   status=np.full(n, -1, dtype=np.int32))
        _check(self._lib.tpamd_project_points_on_paths_host(
            self._h, n, D, _ptr(off), _ptr(w) if w.size else None, _ptr(pt), _ptr(out["waypoint_index"]),
            _ptr(out["distance_to_path"]), _ptr(out["line_parameter"]), _ptr(out["projected_point"]),
            _ptr(out["status"])), "tpamd_project_points_on_paths_host")
        return out

    def sample_ik_targets(self, fit, delta, row_offsets, stream=None, first_row=None):
        """The IK callback's inputs for a ragged batch (tpamd_sample_ik_targets_*): `fit` holds knots,
        translation_points, rotation_points, joint_control_points (packed, as fit_pose_waypoints
        returns them; every path needs at least 3 control points) and point_offsets [B + 1] or
        num_points [B]; row r of path k, rows row_offsets[k]:row_offsets[k + 1], belongs to parameter
        r * delta[k]. With first_row [B] (host int32; tpamd_sample_ik_target_rows_*) path k's output
        rows are table rows first_row[k] .. of its path: (first_row[k] + r) * delta[k], bit-equal to
        the same rows of a whole-path call. Returns (pose_targets [rows][7], joint_targets [rows][D])
        on the side the spline arrays are on."""
        import torch
        off = _host(row_offsets, np.int32, what="row offsets").reshape(-1)
        B = off.shape[0] - 1
        fr = None if first_row is None else _host(first_row, np.int32, (B,), "first_row")
        if fit.get("point_offsets") is not None:
            npts = np.diff(_host(fit["point_offsets"], np.int32).reshape(-1)).astype(np.int32)
        else:
            npts = _host(fit["num_points"], np.int32).reshape(-1)
        npts = np.ascontiguousarray(npts)
        if npts.shape[0] != B:
            raise TpamdError("row offsets need one entry per path plus one")
        rows = int(off[-1]) if B else 0
        jc = fit["joint_control_points"]
        D = int(jc.shape[-1])
        if _is_cuda(jc):
            dev = jc.device
            f = lambda x, what: PlannerSet._cuda(x, torch.float64, dev, None, what)
            dl = f(delta if hasattr(delta, "shape") else torch.full((B,), float(delta), dtype=torch.float64), "delta")
            if tuple(dl.shape) != (B,):
                raise TpamdError("delta has shape %s, expected (%d,)" % (tuple(dl.shape), B))
            pose = torch.zeros((rows, 7), dtype=torch.float64, device=dev)
            joint = torch.zeros((rows, D), dtype=torch.float64, device=dev)
            splines = (_ptr(f(fit["knots"], "knots")), _ptr(f(fit["translation_points"], "translation_points")),
                       _ptr(f(fit["rotation_points"], "rotation_points")), _ptr(f(jc, "joint_control_points")), _ptr(dl),
                       _ptr(pose), _ptr(joint), _stream_ptr(stream))
            if fr is not None:
                _check(self._lib.tpamd_sample_ik_target_rows_device(self._h, B, D, _ptr(npts), _ptr(off), _ptr(fr),
                                                                    *splines), "tpamd_sample_ik_target_rows_device")
            else:
                _check(self._lib.tpamd_sample_ik_targets_device(self._h, B, D, _ptr(npts), _ptr(off), *splines),
                       "tpamd_sample_ik_targets_device")
            return pose, joint
        h = lambda x, what: _host(x, np.float64, what=what)
        dl = _host(np.broadcast_to(_host(delta, np.float64), (B,)), np.float64, (B,), "delta")
        pose, joint = np.zeros((rows, 7)), np.zeros((rows, D))
        splines = (_ptr(h(fit["knots"], "knots")), _ptr(h(fit["translation_points"], "translation_points")),
                   _ptr(h(fit["rotation_points"], "rotation_points")), _ptr(h(jc, "joint_control_points")), _ptr(dl),
                   _ptr(pose), _ptr(joint))
        if fr is not None:
            _check(self._lib.tpamd_sample_ik_target_rows_host(self._h, B, D, _ptr(npts), _ptr(off), _ptr(fr), *splines),
                   "tpamd_sample_ik_target_rows_host")
        else:
            _check(self._lib.tpamd_sample_ik_targets_host(self._h, B, D, _ptr(npts), _ptr(off), *splines),
                   "tpamd_sample_ik_targets_host")
        return pose, joint

    def ik_table_rows(self, path_end, delta, num_samples):
        """BuildIkTable's row count round(path_end / delta) + num_samples + 1 (tpamd_ik_table_rows)."""
        return self._lib.tpamd_ik_table_rows(float(path_end), float(delta), int(num_samples))

    def find_max_sd2(self, a, b, lower, upper):
        """Host numpy [num][C] -> (sd2max, sddmax, sd2zero) [num]."""
        a, b, lower, upper = (np.ascontiguousarray(x, dtype=np.float64)
                              for x in (a, b, lower, upper))
        num, Cn = a.shape
        o = [np.zeros(num) for _ in range(3)]
        _check(self._lib.tpamd_find_max_sd2_host(self._h, num, Cn, _ptr(a), _ptr(b), _ptr(lower),
                                                 _ptr(upper), _ptr(o[0]), _ptr(o[1]), _ptr(o[2])),
               "tpamd_find_max_sd2_host")
        return tuple(o)

    def query(self, time, s, sd, status, t_query, out_s, out_sd, out_sdd, ok=None, stream=None,
              sd2=None):
        """sd2: the solve's squared velocities (outputs["sd2"]); None = the engine's copy from
        its last solve (TpamdError "stale" if time is not that solve's output)."""
        B, N = time.shape
        K = t_query.shape[1]
        _check(self._lib.tpamd_query_device(self._h, B, N, K, _ptr(time), _ptr(s), _ptr(sd),
                                            _ptr(sd2), _ptr(status), _ptr(t_query), _ptr(out_s),
                                            _ptr(out_sd), _ptr(out_sdd), _ptr(ok),
                                            _stream_ptr(stream)), "tpamd_query_device")

    def resample_uniform(self, sol, max_acceleration, start_sec, time_step, out, stream=None,
                         skip=False):
        """sol: dict time,s,sd,sdd [B][N], q,qd,qdd [B][N][D], status. out: dict out_time..
        [B][max_out], out_q.. [B][max_out][D], count [B] int32. skip=True: the
        kSkipSamplesCloserThanTimeStep method instead of the uniform one (any N: the kernel
        keeps no per-sample table; count reports every output, slots below max_out are written)."""
        B, N, D = sol["q"].shape
        max_out = out["out_time"].shape[1]
        args = _ResampleArgs(
            B, N, D, max_out,
            *[_ptr(sol[k]) for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd")],
            _ptr(max_acceleration), _ptr(start_sec), float(time_step), _ptr(sol.get("status")),
            *[_ptr(out[k]) for k in ("out_time", "out_s", "out_sd", "out_sdd", "out_q",
                                     "out_qd", "out_qdd", "count")])
        fn = self._lib.tpamd_resample_skip_device if skip else self._lib.tpamd_resample_uniform_device
        _check(fn(self._h, C.byref(args), _stream_ptr(stream)),
               "tpamd_resample_skip_device" if skip else "tpamd_resample_uniform_device")

    def fastest_stop(self, time, s, qd, qdd, max_acceleration, query_time, count=None,
                     profile=False, stream=None, host=False):
        """GetPathStopParameter for a batch (tpamd_fastest_stop_*): time, s [B][stride], qd, qdd
        [B][stride][D], max_acceleration [B][D], query_time [B] seconds, count [B] int32 or None
        (every row has stride samples) -- e.g. a solve's outputs or resample_uniform's out_* and
        count as they are. Returns a dict stop_parameter, duration [B] float64, stop_index,
        status [B] int32 (TPAMD_PLAN_*), and with profile=True profile_time, profile_rate2,
        profile_drate2 [B][stride] (entries 0 .. stop_index - start of each row are written).
        host=False: CUDA tensors, outputs on their device, enqueued on `stream`; host=True: CPU
        arrays (numpy or torch), numpy outputs, synchronous."""
        B, M, D = qd.shape
        if host:
            cv = lambda x, dt: None if x is None else np.ascontiguousarray(
                x.numpy() if hasattr(x, "numpy") else x, dtype=dt)
            time, s, qd, qdd, max_acceleration, query_time = (
                cv(x, np.float64) for x in (time, s, qd, qdd, max_acceleration, query_time))
            count = cv(count, np.int32)
            new = lambda shape, dt: np.zeros(shape, dtype=dt)
            f64, i32 = np.float64, np.int32
        else:
            import torch
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=qd.device)
            f64, i32 = torch.float64, torch.int32
        out = dict(stop_parameter=new((B,), f64), stop_index=new((B,), i32),
                   duration=new((B,), f64), status=new((B,), i32))
        if profile:
            for k in ("profile_time", "profile_rate2", "profile_drate2"):
                out[k] = new((B, M), f64)
        args = _FastestStopArgs(
            B, M, D, 0, _ptr(time), _ptr(s), _ptr(qd), _ptr(qdd), _ptr(count),
            _ptr(max_acceleration), _ptr(query_time),
            *[_ptr(out.get(k)) for k in ("stop_parameter", "stop_index", "duration", "status",
                                         "profile_time", "profile_rate2", "profile_drate2")])
        if host:
            _check(self._lib.tpamd_fastest_stop_host(self._h, C.byref(args)),
                   "tpamd_fastest_stop_host")
        else:
            _check(self._lib.tpamd_fastest_stop_device(self._h, C.byref(args), _stream_ptr(stream)),
                   "tpamd_fastest_stop_device")
        return out

    def stop_trajectories(self, time, qd, qdd, max_acceleration, time_step, stop_time=None, stop_index=None,
                          count=None, out=None, stream=None, host=False):
        """StopBeforeTime / StopAtIndex for a batch (tpamd_stop_trajectories_*): time [B][stride],
        qd, qdd [B][stride][D], max_acceleration [B][D], and per row either stop_time [B] seconds or
        stop_index [B] int32; count [B] int32 or None (every row has stride samples). Returns a dict
        status, keep, first, last [B] int32 and out_time [B][stride], out_qd, out_qdd
        [B][stride][D], written at rows [first, last] only; `out` may bring these three arrays
        (to see what a call leaves untouched), else they start as zeros. host=False: CUDA tensors,
        enqueued on `stream`; host=True: CPU arrays (numpy or torch), numpy outputs, synchronous."""
        if (stop_time is None) == (stop_index is None):
            raise TpamdError("give either stop_time or stop_index")
        B, M, D = qd.shape
        if host:
            cv = lambda x, dt: None if x is None else np.ascontiguousarray(
                x.numpy() if hasattr(x, "numpy") else x, dtype=dt)
            time, qd, qdd, max_acceleration, stop_time = (
                cv(x, np.float64) for x in (time, qd, qdd, max_acceleration, stop_time))
            count, stop_index = cv(count, np.int32), cv(stop_index, np.int32)
            new = lambda shape, dt: np.zeros(shape, dtype=dt)
            f64, i32 = np.float64, np.int32
        else:
            import torch
            new = lambda shape, dt: torch.zeros(shape, dtype=dt, device=qd.device)
            f64, i32 = torch.float64, torch.int32
        res = {k: new((B,), i32) for k in ("status", "keep", "first", "last")}
        for k, shape in (("out_time", (B, M)), ("out_qd", (B, M, D)), ("out_qdd", (B, M, D))):
            res[k] = out[k] if out is not None else new(shape, f64)
            if tuple(res[k].shape) != shape:
                raise TpamdError("%s has shape %s, expected %s" % (k, tuple(res[k].shape), shape))
        args = _StopTrajectoryArgs(
            B, M, D, 0, _ptr(time), _ptr(qd), _ptr(qdd), _ptr(count), _ptr(max_acceleration), float(time_step),
            _ptr(stop_time), _ptr(stop_index),
            *[_ptr(res[k]) for k in ("status", "keep", "first", "last", "out_time", "out_qd", "out_qdd")])
        if host:
            _check(self._lib.tpamd_stop_trajectories_host(self._h, C.byref(args)), "tpamd_stop_trajectories_host")
        else:
            _check(self._lib.tpamd_stop_trajectories_device(self._h, C.byref(args), _stream_ptr(stream)),
                   "tpamd_stop_trajectories_device")
        return res

    def debug_boundary(self, B, N):
        arr = {k: np.zeros((B, N)) for k in ("sd2_max", "sdd_max", "sdd_min", "sd2_zero", "sd2")}
        arr["type"] = np.zeros((B, N), dtype=np.uint8)
        _check(self._lib.tpamd_debug_copy_boundary(
            self._h, B, N, _ptr(arr["sd2_max"]), _ptr(arr["sdd_max"]), _ptr(arr["sdd_min"]),
            _ptr(arr["sd2_zero"]), _ptr(arr["type"]), _ptr(arr["sd2"])),
            "tpamd_debug_copy_boundary")
        return arr

    def debug_keep_boundary(self, on=True):
        """Have the fused joint sweep store sdd_max/sdd_min/type for debug_boundary()."""
        self._lib.tpamd_debug_keep_boundary(self._h, 1 if on else 0)

    def rebuild_time(self, sd, ds, time_start, out, num_shards, paths_per_shard, num_samples,
                     shard_stride, num_samples_per_path=None, stream=None):
        """time [num_shards * paths_per_shard][N] from sd (tpamd_rebuild_time_device). sd, ds and
        time_start are tensors (views) that start at shard 0's data; shard r lies shard_stride
        doubles further."""
        _check(self._lib.tpamd_rebuild_time_device(
            self._h, num_shards, paths_per_shard, num_samples, shard_stride, _ptr(sd), _ptr(ds),
            _ptr(time_start), _ptr(num_samples_per_path), _ptr(out), _stream_ptr(stream)),
            "tpamd_rebuild_time_device")

    def debug_kernel_vgprs(self, which):
        """Registers per lane of the 7-joint sampling/LP kernel (0) / sweep kernel (1)."""
        n = self._lib.tpamd_debug_kernel_vgprs(self._h, which)
        _check(min(n, 0), "tpamd_debug_kernel_vgprs")
        return n

    def debug_diag(self, B):
        out = np.zeros((B, 64), dtype=np.int64)
        _check(self._lib.tpamd_debug_copy_diag(self._h, B, _ptr(out)), "tpamd_debug_copy_diag")
        return out

    def debug_diag_ext(self, B):
        out = np.zeros((B, 32), dtype=np.int64)
        _check(self._lib.tpamd_debug_copy_diag_ext(self._h, B, _ptr(out)), "tpamd_debug_copy_diag_ext")
        return out

    # ---------------------------------------------------------------- timing
    def profile_enable(self, on=True):
        """True / 1: events around every kernel; 2: around the sweep kernel only; False: off."""
        self._lib.tpamd_profile_enable(self._h, int(on) if on in (1, 2) else (1 if on else 0))

    def profile_reset(self):
        self._lib.tpamd_profile_reset(self._h)

    def profile_mean_ms(self, kernel_index):
        n = C.c_int(0)
        ms = self._lib.tpamd_profile_mean_ms(self._h, int(kernel_index), C.byref(n))
        return ms, n.value

    def profile_summary(self):
        out = {}
        for k in range(self._lib.tpamd_profile_num_kernels()):
            ms, n = self.profile_mean_ms(k)
            out[self._lib.tpamd_profile_kernel_name(k).decode()] = (ms, n)
        return out


def _is_cuda(t):
    return hasattr(t, "is_cuda") and t.is_cuda


def _host(x, dtype, shape=None, what="argument"):
    """A C-contiguous numpy copy of a host (or CUDA) array-like; None stays None."""
    if x is None:
        return None
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x, dtype=dtype))
    if shape is not None and a.shape != tuple(shape):
        raise TpamdError("%s has shape %s, expected %s" % (what, a.shape, tuple(shape)))
    return a


class PlannerSet:
    """B receding-horizon planners with joint-space spline paths whose whole state stays on the
    device between calls (include/tpamd.h tpamd_planner_set_*). The typical loop keeps its goals,
    limits and setpoints in CUDA tensors:

        with PlannerSet(engine, B, D, N) as ps:
            ps.set_waypoints(wps, offsets, vmax, amax, delta)     # wps: CUDA [rows][D]
            summary = ps.plan(start_ns, horizon_ns)
            ps.sample_at_ticks(t0_ns, step_ns, T, q=q, qd=qd)     # CUDA [B][T][D]

    CUDA tensors go through the _device entries on torch's current stream (or `stream`); CPU
    tensors and numpy arrays through the host entries, which synchronise. ids (int32, each listed
    once where a call changes planners; None: planners 0..count-1) and waypoint offsets are host
    arrays in every call (a CUDA tensor is copied to the host first). Errors raise TpamdError.

    cartesian=True makes a set of the second kind: every planner's path is the IK table of a
    Cartesian path (set_ik_tables; table_capacity rows per planner to start with, it grows). The
    joint-spline calls (set_waypoints, set_paths, download_path, switch_paths, retarget) fail on such a set,
    set_ik_tables / download_ik_table on a joint set; everything else works on both kinds."""

    def __init__(self, engine, num_planners, num_dofs, num_samples, num_points=16, time_step_ns=4_000_000,
                 sampling_method=0, max_planning_iterations=200, constraint_safety=0.8,
                 max_initial_velocity_error=1e-2, history_capacity=0, trajectory_capacity=0, cartesian=False,
                 table_capacity=0):
        self._lib = load_library()
        self.B, self.D, self.N = int(num_planners), int(num_dofs), int(num_samples)
        self.device = engine.device
        cfg = _PlannerSetConfig(self.B, self.D, self.N, int(num_points), int(history_capacity),
                                int(trajectory_capacity), int(sampling_method), int(max_planning_iterations),
                                float(constraint_safety), float(max_initial_velocity_error), int(time_step_ns))
        h = C.c_void_p()
        self.cartesian = bool(cartesian)
        if self.cartesian:
            rows = int(table_capacity) if table_capacity else 4 * self.N
            _check(self._lib.tpamd_planner_set_create_cartesian(engine._h, C.byref(cfg), rows, C.byref(h)),
                   "tpamd_planner_set_create_cartesian")
        else:
            _check(self._lib.tpamd_planner_set_create(engine._h, C.byref(cfg), C.byref(h)), "tpamd_planner_set_create")
        self._engine = engine          # the set must not outlive its engine
        self._h = h
        self._num_samples = np.zeros(self.B, dtype=np.int64)    # GetNumTimeSamples after the last plan
        self._pending = None           # the PlanHandle of a plan_async whose result() has not run yet
        self._imports = []             # device imports whose summaries have not been read yet

    def close(self):
        if getattr(self, "_h", None):
            if getattr(self, "_pending", None) is not None:
                self._pending._stream.synchronize()      # the call writes the handle's tensors
                self._pending = None
            self._lib.tpamd_planner_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not getattr(self, "_h", None):
            raise TpamdError("the planner set is closed")
        return self._h

    def _sample_counts(self):
        """The sample counts of the last plan; they are unknown while a plan_async is in flight."""
        if self._pending is not None:
            raise TpamdError("a plan_async call is in flight: its sample counts are on the device until "
                             "PlanHandle.result()")
        self._settle_imports()
        return self._num_samples

    def _settle_imports(self):
        """The sample counts of planners that a device import_state changed, from the summaries
        the call left on the device: synchronises those calls' streams, once."""
        pending, self._imports = self._imports, []
        for stream, summary, status, ids in pending:
            stream.synchronize()
            got = summary.cpu().numpy().view(PLANNER_SUMMARY_DTYPE)[:, 0]
            ok = status.cpu().numpy() == 0
            self._num_samples[ids[ok]] = got["num_samples"][ok]

    def _ids(self, ids, count=None):
        if ids is None:
            return None, (self.B if count is None else int(count))
        a = _host(ids, np.int32, what="ids").reshape(-1)
        return a, a.shape[0]

    @property
    def device_bytes(self):
        return self._lib.tpamd_planner_set_device_bytes(self._handle())

    # ------------------------------------------------------------ paths
    def set_waypoints(self, waypoints, offsets, max_velocity, max_acceleration, delta, initial_velocity=None,
                      ids=None, rounding=0.2, stream=None):
        """New waypoint paths, fitted on the device (tpamd_planner_set_set_waypoints*):
        listed planner k (ids[k], or k) gets waypoints[offsets[k]:offsets[k + 1]] ([rows][D]
        float64), max_velocity / max_acceleration / initial_velocity [count][D] (initial_velocity
        None: zero), delta [count] (or one number) and the PathOptions rounding radius `rounding`.
        Returns (status, num_points) int32 [count]: TPAMD_PLAN_* per planner (no waypoints:
        INVALID_ARGUMENT, the planner keeps its state) and the control points after the call. With
        a CUDA `waypoints` every array is taken on its device and the call only enqueues on
        `stream` (default: torch's current stream); results are CUDA tensors. Otherwise the host
        entry runs and synchronises; results are CPU tensors."""
        import torch
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("waypoint offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        D = self.D
        if _is_cuda(waypoints):
            dev = waypoints.device
            f = lambda x, shape, what: self._cuda(x, torch.float64, dev, shape, what)
            w = f(waypoints, None, "waypoints").reshape(-1, D) if waypoints.numel() else \
                torch.zeros((0, D), dtype=torch.float64, device=dev)
            if n and w.shape[0] != off[-1]:
                raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
            vm, am = f(max_velocity, (n, D), "max_velocity"), f(max_acceleration, (n, D), "max_acceleration")
            dl = f(delta if hasattr(delta, "shape") else torch.full((n,), float(delta), dtype=torch.float64),
                   (n,), "delta")
            iv = None if initial_velocity is None else f(initial_velocity, (n, D), "initial_velocity")
            status = torch.full((n,), -1, dtype=torch.int32, device=dev)
            num_points = torch.zeros((n,), dtype=torch.int32, device=dev)
            _check(self._lib.tpamd_planner_set_set_waypoints_device(
                self._handle(), n, _ptr(ida), _ptr(off), w.data_ptr() if w.numel() else None, float(rounding),
                _ptr(vm), _ptr(am), _ptr(dl), _ptr(iv), _ptr(num_points), _ptr(status),
                _stream_ptr(stream)), "tpamd_planner_set_set_waypoints_device")
            return status, num_points
        w = _host(waypoints, np.float64, what="waypoints").reshape(-1, D)
        if w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        vm = _host(max_velocity, np.float64, (n, D), "max_velocity")
        am = _host(max_acceleration, np.float64, (n, D), "max_acceleration")
        dl = _host(np.broadcast_to(_host(delta, np.float64), (n,)), np.float64, (n,), "delta")
        iv = _host(initial_velocity, np.float64, (n, D), "initial_velocity")
        status = np.full(n, -1, dtype=np.int32)
        num_points = np.zeros(n, dtype=np.int32)
        _check(self._lib.tpamd_planner_set_set_waypoints(
            self._handle(), n, _ptr(ida), _ptr(off), _ptr(w) if w.size else None, float(rounding), _ptr(vm),
            _ptr(am), _ptr(dl), _ptr(iv), _ptr(num_points), _ptr(status)), "tpamd_planner_set_set_waypoints")
        return torch.from_numpy(status), torch.from_numpy(num_points)

    def retarget(self, time_ns, waypoints, offsets, max_velocity, max_acceleration, delta, ids=None, rounding=0.2,
                 stopping_acceleration=None, stream=None):
        """Redirects moving planners onto new waypoints, abandoning the old path at time_ns [count]
        (tpamd_planner_set_retarget*): per listed planner the position and velocity at that time on
        the resident trajectory, ComputeStoppingPoint with stopping_acceleration [count][D] (None:
        max_acceleration), the fit of [position, stopping point, waypoints[offsets[k]:offsets[k + 1]]...]
        (a planner at rest: without the stopping point; no waypoints is allowed) and the commit of
        set_waypoints with that velocity as initial velocity. The next plan(time_ns, ...) continues
        from there. Returns a dict: status, num_points int32 [count], position, velocity,
        stopping_point [count][D] (NaN rows for a planner that failed: it keeps its state). With a
        CUDA `waypoints` (or, without waypoints, a CUDA time_ns) every array is taken on its device
        and the call only enqueues on `stream` (default: torch's current stream); results are CUDA
        tensors. Otherwise the host entry runs and synchronises; results are CPU tensors."""
        import torch
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("waypoint offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        D = self.D
        if _is_cuda(waypoints) or (_is_cuda(time_ns) and int(off[-1]) == 0):
            dev = waypoints.device if _is_cuda(waypoints) else time_ns.device
            f = lambda x, shape, what: self._cuda(x, torch.float64, dev, shape, what)
            w = f(waypoints, None, "waypoints").reshape(-1, D) if int(off[-1]) else \
                torch.zeros((0, D), dtype=torch.float64, device=dev)
            if w.shape[0] != off[-1]:
                raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
            t = self._cuda(time_ns, torch.int64, dev, (n,), "time_ns")
            vm, am = f(max_velocity, (n, D), "max_velocity"), f(max_acceleration, (n, D), "max_acceleration")
            dl = f(delta if hasattr(delta, "shape") else torch.full((n,), float(delta), dtype=torch.float64),
                   (n,), "delta")
            sa = None if stopping_acceleration is None else f(stopping_acceleration, (n, D), "stopping_acceleration")
            nan = lambda: torch.full((n, D), float("nan"), dtype=torch.float64, device=dev)
            out = dict(status=torch.full((n,), -1, dtype=torch.int32, device=dev),
                       num_points=torch.zeros((n,), dtype=torch.int32, device=dev),
                       position=nan(), velocity=nan(), stopping_point=nan())
            _check(self._lib.tpamd_planner_set_retarget_device(
                self._handle(), n, _ptr(ida), _ptr(t), _ptr(off), w.data_ptr() if w.numel() else None,
                float(rounding), _ptr(vm), _ptr(am), _ptr(dl), _ptr(sa), _ptr(out["num_points"]), _ptr(out["status"]),
                _ptr(out["position"]), _ptr(out["velocity"]), _ptr(out["stopping_point"]), _stream_ptr(stream)),
                "tpamd_planner_set_retarget_device")
            return out
        w = _host(waypoints, np.float64, what="waypoints").reshape(-1, D)
        if w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        t = _host(time_ns, np.int64, (n,), "time_ns")
        vm = _host(max_velocity, np.float64, (n, D), "max_velocity")
        am = _host(max_acceleration, np.float64, (n, D), "max_acceleration")
        dl = _host(np.broadcast_to(_host(delta, np.float64), (n,)), np.float64, (n,), "delta")
        sa = _host(stopping_acceleration, np.float64, (n, D), "stopping_acceleration")
        out = dict(status=np.full(n, -1, dtype=np.int32), num_points=np.zeros(n, dtype=np.int32),
                   position=np.full((n, D), np.nan), velocity=np.full((n, D), np.nan),
                   stopping_point=np.full((n, D), np.nan))
        _check(self._lib.tpamd_planner_set_retarget(
            self._handle(), n, _ptr(ida), _ptr(t), _ptr(off), _ptr(w) if w.size else None, float(rounding), _ptr(vm),
            _ptr(am), _ptr(dl), _ptr(sa), _ptr(out["num_points"]), _ptr(out["status"]), _ptr(out["position"]),
            _ptr(out["velocity"]), _ptr(out["stopping_point"])), "tpamd_planner_set_retarget")
        return {k: torch.from_numpy(v) for k, v in out.items()}

    @staticmethod
    def _cuda(x, dtype, device, shape, what):
        import torch
        t = torch.as_tensor(x, dtype=dtype, device=device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise TpamdError("%s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t

    def set_paths(self, knots, control_points, num_points, max_velocity, max_acceleration, delta,
                  initial_velocity=None, ids=None, path_state=None):
        """Fitted splines of any size (tpamd_planner_set_upload_paths_ragged): planner k's
        num_points[k] control points [P][D] and P + 3 knots packed behind planner k - 1's in
        control_points / knots; limits [count][D], delta [count], path_state [count] (1 kNewPath,
        default, or 2 kModifiedPath). Host arrays; synchronises."""
        npts = _host(num_points, np.int32, what="num_points").reshape(-1)
        ida, n = self._ids(ids, npts.shape[0])
        if npts.shape[0] != n:
            raise TpamdError("one num_points per listed planner")
        D = self.D
        k = _host(knots, np.float64, what="knots").reshape(-1)
        c = _host(control_points, np.float64, what="control_points").reshape(-1)
        if k.shape[0] != int(npts.sum()) + 3 * n or c.shape[0] != int(npts.sum()) * D:
            raise TpamdError("knots / control_points do not hold the listed paths")
        vm = _host(max_velocity, np.float64, (n, D), "max_velocity")
        am = _host(max_acceleration, np.float64, (n, D), "max_acceleration")
        dl = _host(np.broadcast_to(_host(delta, np.float64), (n,)), np.float64, (n,), "delta")
        iv = _host(initial_velocity, np.float64, (n, D), "initial_velocity")
        ps = np.ones(n, dtype=np.int32) if path_state is None else _host(path_state, np.int32, (n,), "path_state")
        _check(self._lib.tpamd_planner_set_upload_paths_ragged(
            self._handle(), n, _ptr(ida), _ptr(npts), _ptr(k), _ptr(c), _ptr(vm), _ptr(am), _ptr(dl), _ptr(iv),
            _ptr(ps)), "tpamd_planner_set_upload_paths_ragged")

    def set_ik_tables(self, ik_positions, jacobians, row_offsets, path_end, max_velocity, max_acceleration,
                      max_translational_velocity, max_rotational_velocity, delta, initial_velocity=None, ids=None,
                      path_state=None, stream=None):
        """The IK tables of a Cartesian set's planners (tpamd_planner_set_upload_ik_tables*): listed
        planner k (ids[k], or k) gets rows row_offsets[k]:row_offsets[k + 1] of ik_positions
        [rows][D] and jacobians [rows][6][D]; row r belongs to path parameter r * delta[k]. path_end,
        max_translational_velocity, max_rotational_velocity, delta [count] (or one number each),
        max_velocity / max_acceleration / initial_velocity [count][D] (initial_velocity None: zero),
        path_state [count] int32 (1 kNewPath, the default, or 2 kModifiedPath). With a CUDA
        `ik_positions` every array is taken on its device and the call only enqueues on `stream`
        (default: torch's current stream); otherwise the host entry runs and synchronises."""
        import torch
        off = _host(row_offsets, np.int32, what="row offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("row offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        D = self.D
        rows = int(off[-1]) if n else 0
        if _is_cuda(ik_positions):
            dev = ik_positions.device
            f = lambda x, shape, what: self._cuda(x, torch.float64, dev, shape, what)
            per = lambda x, what: f(x if hasattr(x, "shape") else torch.full((n,), float(x), dtype=torch.float64),
                                    (n,), what)
            q, J = f(ik_positions, (rows, D), "ik_positions"), f(jacobians, (rows, 6, D), "jacobians")
            pe, vt, vr, dl = (per(path_end, "path_end"), per(max_translational_velocity, "max_translational_velocity"),
                              per(max_rotational_velocity, "max_rotational_velocity"), per(delta, "delta"))
            vm, am = f(max_velocity, (n, D), "max_velocity"), f(max_acceleration, (n, D), "max_acceleration")
            iv = None if initial_velocity is None else f(initial_velocity, (n, D), "initial_velocity")
            ps = self._cuda(torch.ones(n, dtype=torch.int32) if path_state is None else path_state, torch.int32, dev,
                            (n,), "path_state")
            _check(self._lib.tpamd_planner_set_upload_ik_tables_device(
                self._handle(), n, _ptr(ida), _ptr(off), _ptr(q), _ptr(J), _ptr(pe), _ptr(vm), _ptr(am), _ptr(vt),
                _ptr(vr), _ptr(dl), _ptr(iv), _ptr(ps), _stream_ptr(stream)),
                "tpamd_planner_set_upload_ik_tables_device")
            return
        per = lambda x, what: _host(np.broadcast_to(_host(x, np.float64), (n,)), np.float64, (n,), what)
        q = _host(ik_positions, np.float64, (rows, D), "ik_positions")
        J = _host(jacobians, np.float64, (rows, 6, D), "jacobians")
        pe, vt, vr, dl = (per(path_end, "path_end"), per(max_translational_velocity, "max_translational_velocity"),
                          per(max_rotational_velocity, "max_rotational_velocity"), per(delta, "delta"))
        vm = _host(max_velocity, np.float64, (n, D), "max_velocity")
        am = _host(max_acceleration, np.float64, (n, D), "max_acceleration")
        iv = _host(initial_velocity, np.float64, (n, D), "initial_velocity")
        ps = np.ones(n, dtype=np.int32) if path_state is None else _host(path_state, np.int32, (n,), "path_state")
        _check(self._lib.tpamd_planner_set_upload_ik_tables(
            self._handle(), n, _ptr(ida), _ptr(off), _ptr(q), _ptr(J), _ptr(pe), _ptr(vm), _ptr(am), _ptr(vt),
            _ptr(vr), _ptr(dl), _ptr(iv), _ptr(ps)), "tpamd_planner_set_upload_ik_tables")

    def set_pose_waypoints(self, pose_waypoints, joint_waypoints, offsets, ik, max_velocity, max_acceleration,
                           max_translational_velocity, max_rotational_velocity, delta, translation_rounding=0.05,
                           rotation_rounding=0.2, initial_velocity=None, ids=None, stream=None, streaming=False):
        """New Cartesian goals for the listed planners of a Cartesian set, without the host touching
        per-row data: listed planner k (ids[k], or k) takes rows offsets[k]:offsets[k + 1] of
        pose_waypoints [rows][7] (translation, then quaternion w, x, y, z) and joint_waypoints
        [rows][D], CUDA tensors (host arrays are copied up). The chain:
          1. Engine.fit_pose_waypoints on the device (TimeableCartesianSplinePath::SetWaypoints with
             CartesianPathOptions' roundings; translation_rounding defaults to its 0.05);
          2. path_end comes down (count doubles) and sizes each table with tpamd_ik_table_rows;
          3. Engine.sample_ik_targets;
          4. ik(pose_targets [rows][7], joint_targets [rows][D], row_offsets) -> (ik_positions
             [rows][D], jacobians [rows][6][D]) as CUDA tensors: the caller's IK;
          5. set_ik_tables with those tensors, path_end of the fit and path_state 1 (kNewPath).
        A planner whose fit failed (no waypoints: TPAMD_PLAN_INVALID_ARGUMENT) is left out of steps 3-5
        and keeps its path and plan. Limits and delta as for set_ik_tables ([count][D], [count] or one
        number). Returns (status int32 [count], rows int32 [count]) as CPU tensors; rows is 0 where the
        fit failed. Raises TpamdError on a joint set, as set_ik_tables does.
        With streaming=True only rows 0 .. N-1 of every table are sampled, solved and uploaded
        (`rows` reports N); the fitted splines stay on the device with the set, and plan_streaming
        extends the tables as the windows reach past them. The listed planners must then be all of
        the set's (ids None)."""
        import torch
        if not self.cartesian:
            _check(-1, "tpamd_planner_set_upload_ik_tables_device")      # what the entry returns on a joint set
        off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("waypoint offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        D = self.D
        dev = pose_waypoints.device if _is_cuda(pose_waypoints) else torch.device("cuda", self.device)
        f = lambda x, shape, what: self._cuda(x, torch.float64, dev, shape, what)
        per = lambda x, what: f(x if hasattr(x, "shape") else torch.full((n,), float(x), dtype=torch.float64),
                                (n,), what)
        rows_w = int(off[-1]) if n else 0
        pw, jw = f(pose_waypoints, (rows_w, 7), "pose_waypoints"), f(joint_waypoints, (rows_w, D), "joint_waypoints")
        dl = per(delta, "delta")
        vm, am = f(max_velocity, (n, D), "max_velocity"), f(max_acceleration, (n, D), "max_acceleration")
        vt, vr = per(max_translational_velocity, "max_translational_velocity"), per(max_rotational_velocity,
                                                                                    "max_rotational_velocity")
        iv = None if initial_velocity is None else f(initial_velocity, (n, D), "initial_velocity")
        E = self._engine
        fit = E.fit_pose_waypoints(pw, jw, off, per(translation_rounding, "translation_rounding"),
                                   per(rotation_rounding, "rotation_rounding"), stream=stream)
        if stream is not None:                                    # the copies below run on torch's stream
            stream.synchronize() if hasattr(stream, "synchronize") else torch.cuda.synchronize(dev)
        path_end = fit["path_end"].cpu().numpy()                  # count doubles; orders after the fit
        status = fit["status"].cpu().numpy()
        dl_h = dl.cpu().numpy()
        ok = np.flatnonzero(status == 0)
        rows = np.zeros(n, dtype=np.int32)
        if streaming and (ida is not None or ok.size != n or n != self.B):
            raise TpamdError("streaming=True takes a goal for every planner of the set")
        for k in ok:
            r = self._lib.tpamd_ik_table_rows(float(path_end[k]), float(dl_h[k]), self.N)
            if r < 0:
                raise TpamdError("delta[%d] = %r is not positive" % (k, float(dl_h[k])))
            rows[k] = self.N if streaming else r
        # streaming: the fit stays on the device; the whole-table row counts bound every extension
        self._stream_fit = dict(fit=fit, delta=dl, full_rows=np.array(
            [self._lib.tpamd_ik_table_rows(float(path_end[k]), float(dl_h[k]), self.N) for k in range(n)],
            dtype=np.int64)) if streaming else None
        if ok.size:
            sel = torch.as_tensor(ok, device=dev)
            row_offsets = np.concatenate([[0], np.cumsum(rows[ok])]).astype(np.int32)
            # the spline arrays hold exactly the fitted paths: a path without waypoints has no slots
            sub = dict(fit, point_offsets=np.concatenate([[0], np.cumsum(fit["point_offsets"][1:][ok]
                                                                         - fit["point_offsets"][:-1][ok])]))
            pose_t, joint_t = E.sample_ik_targets(sub, dl[sel].contiguous(), row_offsets, stream=stream)
            q, J = ik(pose_t, joint_t, row_offsets)
            if streaming:      # the last resident row of every table: the seed of its next extension
                self._stream_last = q[torch.as_tensor(row_offsets[1:].astype(np.int64) - 1, device=dev)].clone()
            all_ids = np.arange(n, dtype=np.int32) if ida is None else ida
            take = lambda x: None if x is None else x[sel].contiguous()
            self.set_ik_tables(q, J, row_offsets, fit["path_end"][sel].contiguous(), take(vm), take(am), take(vt),
                               take(vr), take(dl), initial_velocity=take(iv), ids=all_ids[ok], stream=stream)
        return torch.from_numpy(status.astype(np.int32)), torch.from_numpy(rows)

    def download_ik_table(self, planner):
        """The resident IK table of one planner of a Cartesian set: (ik_positions [rows][D],
        jacobians [rows][6][D]) numpy; rows = 0: no table."""
        R = C.c_int32(0)
        _check(self._lib.tpamd_planner_set_download_ik_table(self._handle(), int(planner), C.byref(R), None, None, 0),
               "tpamd_planner_set_download_ik_table")
        q, J = np.zeros((R.value, self.D)), np.zeros((R.value, 6, self.D))
        if R.value:
            _check(self._lib.tpamd_planner_set_download_ik_table(self._handle(), int(planner), C.byref(R), _ptr(q),
                                                                 _ptr(J), R.value),
                   "tpamd_planner_set_download_ik_table")
        return q, J

    def discard_ik_rows(self, keep_from=None, ids=None):
        """Discard the consumed rows at the front of the listed planners' IK tables (None: all) of a
        Cartesian set (tpamd_planner_set_discard_ik_rows): planner k keeps path rows from
        keep_from[k] on; keep_from None: from its safe floor on, the lowest row any later Plan of
        that planner can read, computed on the device. Returns the new first resident rows
        [count] int32 numpy. Up: the ids (and keep_from); down: 4 bytes per listed planner."""
        ida, n = self._ids(ids)
        keep = None
        if keep_from is not None:
            keep = _host(np.broadcast_to(_host(keep_from, np.int32), (n,)), np.int32)
        out = np.zeros(n, dtype=np.int32)
        _check(self._lib.tpamd_planner_set_discard_ik_rows(self._handle(), n, _ptr(ida), _ptr(keep), _ptr(out)),
               "tpamd_planner_set_discard_ik_rows")
        return out

    def ik_table_info(self, planner):
        """Host bookkeeping of one planner's IK table (tpamd_planner_set_ik_table_info):
        (first_row, rows, capacity): the path row in slot 0, the path rows supplied so far (0: no
        table) and the table rows allocated per planner."""
        f, r, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        _check(self._lib.tpamd_planner_set_ik_table_info(self._handle(), int(planner), C.byref(f), C.byref(r), C.byref(c)),
               "tpamd_planner_set_ik_table_info")
        return int(f.value), int(r.value), int(c.value)

    def download_ik_rows(self, planner):
        """The live rows of one planner's IK table (tpamd_planner_set_download_ik_rows):
        (first_row, ik_positions [live][D], jacobians [live][6][D]) numpy, path rows first_row ..
        first_row + live - 1."""
        f, R = C.c_int32(0), C.c_int32(0)
        _check(self._lib.tpamd_planner_set_download_ik_rows(self._handle(), int(planner), C.byref(f), C.byref(R), None,
                                                            None, 0), "tpamd_planner_set_download_ik_rows")
        q, J = np.zeros((R.value, self.D)), np.zeros((R.value, 6, self.D))
        if R.value:
            _check(self._lib.tpamd_planner_set_download_ik_rows(self._handle(), int(planner), C.byref(f), C.byref(R),
                                                                _ptr(q), _ptr(J), R.value),
                   "tpamd_planner_set_download_ik_rows")
        return int(f.value), q, J

    def download_path(self, planner):
        """The resident spline of one planner: (knots [P + 3], control_points [P][D]) numpy; P = 0:
        no path."""
        P = C.c_int32(0)
        _check(self._lib.tpamd_planner_set_download_path(self._handle(), int(planner), C.byref(P), None, None, 0),
               "tpamd_planner_set_download_path")
        k, c = np.zeros(P.value + 3 if P.value else 0), np.zeros((P.value, self.D))
        if P.value:
            _check(self._lib.tpamd_planner_set_download_path(self._handle(), int(planner), C.byref(P), _ptr(k),
                                                             _ptr(c), P.value), "tpamd_planner_set_download_path")
        return k, c

    def reset(self, ids=None):
        """TrajectoryPlanner::Reset for the listed planners (None: all)."""
        ida, n = self._ids(ids)
        _check(self._lib.tpamd_planner_set_reset(self._handle(), n, _ptr(ida)), "tpamd_planner_set_reset")
        self._settle_imports()
        if ida is None:
            self._num_samples[:] = 0
        else:
            self._num_samples[ida] = 0

    # ------------------------------------------------------------ planning
    def plan(self, start_ns, horizon_ns):
        """Plan(start, time_horizon) for every planner (one number or [B] int64 nanoseconds each).
        Returns the summary records as a dict of CPU tensors [B] (status, num_samples, end_time_ns,
        final_decel_start_ns, start_time_ns, target_reached, planned_to_end, windows, path_state,
        history_count)."""
        import torch
        if self._pending is not None:
            raise TpamdError("a plan_async call is in flight (PlanHandle.result())")
        s = _host(np.broadcast_to(_host(start_ns, np.int64), (self.B,)), np.int64)
        h = _host(np.broadcast_to(_host(horizon_ns, np.int64), (self.B,)), np.int64)
        out = np.zeros(self.B, dtype=PLANNER_SUMMARY_DTYPE)
        _check(self._lib.tpamd_planner_set_plan(self._handle(), _ptr(s), _ptr(h), out.ctypes.data),
               "tpamd_planner_set_plan")
        return self._summary(out)

    def last_plan_bytes(self):
        """(host to device, device to host) bytes the last plan / plan_streaming / plan_resume moved."""
        up, down = C.c_size_t(0), C.c_size_t(0)
        self._lib.tpamd_planner_set_last_plan_bytes(self._handle(), C.byref(up), C.byref(down))
        return int(up.value), int(down.value)

    def reserve(self, history=0, trajectory=0):
        """Capacity ahead of time (tpamd_planner_set_reserve): the history and trajectory buffers
        grow to at least this many samples per planner (never shrink; planner state is kept bit for
        bit) and the engine's workspace is sized for this set, so that plan_async allocates nothing."""
        if self._pending is not None:
            raise TpamdError("a plan_async call is in flight (PlanHandle.result())")
        _check(self._lib.tpamd_planner_set_reserve(self._handle(), int(history), int(trajectory)),
               "tpamd_planner_set_reserve")

    def capacity(self):
        """(history, trajectory) samples per planner the buffers hold."""
        h, t = C.c_int32(0), C.c_int32(0)
        _check(self._lib.tpamd_planner_set_capacity(self._handle(), C.byref(h), C.byref(t)),
               "tpamd_planner_set_capacity")
        return int(h.value), int(t.value)

    def plan_async(self, start_ns, horizon_ns, max_windows=2, stream=None):
        """Plan, enqueued only (tpamd_planner_set_plan_device): start_ns / horizon_ns are CUDA
        int64 tensors [B], exactly max_windows window iterations are enqueued on `stream` (torch's
        current stream if None) and every planner ends as plan() leaves it on a set with
        max_planning_iterations = min(its value, max_windows - 1). Nothing comes to the host and
        nothing blocks: retargets, readouts into CUDA tensors and BufferSet.insert_from can be
        enqueued behind it on the same stream. Returns a PlanHandle holding the summary and info
        tensors on the device; its result() synchronises the stream and returns plan()'s dict plus
        `info`. Until then the sample counts of this plan are unknown on the host: methods that
        size their outputs from them (download_trajectories, stop_trajectories without a capacity)
        raise TpamdError. A planner without room in its history or for its trajectory gets status
        PLAN_RESOURCE_EXHAUSTED; info says what reserve() needs (then reset and a new path)."""
        import torch
        if self._pending is not None:
            raise TpamdError("a plan_async call is in flight (PlanHandle.result())")
        dev = torch.device("cuda", self.device)
        for name, a in (("start_ns", start_ns), ("horizon_ns", horizon_ns)):
            if not _is_cuda(a) or a.dtype != torch.int64 or tuple(a.shape) != (self.B,) or not a.is_contiguous():
                raise TpamdError("%s must be a contiguous CUDA int64 tensor [%d]" % (name, self.B))
        if int(max_windows) < 1:
            raise TpamdError("max_windows must be at least 1")
        st = torch.cuda.current_stream(dev) if stream is None else stream
        summary = torch.zeros(self.B * PLANNER_SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        info = torch.zeros(C.sizeof(_PlanDeviceInfo) // 4, dtype=torch.int32, device=dev)
        if st != torch.cuda.current_stream(dev):      # the zero fills ran on the current stream
            st.wait_stream(torch.cuda.current_stream(dev))
        _check(self._lib.tpamd_planner_set_plan_device(self._handle(), _ptr(start_ns), _ptr(horizon_ns),
                                                       int(max_windows), _ptr(summary), _ptr(info),
                                                       _stream_ptr(st)), "tpamd_planner_set_plan_device")
        self._pending = PlanHandle(self, st, summary, info, (start_ns, horizon_ns))
        return self._pending

    def _summary(self, out):
        import torch
        self._imports = []             # a Plan of every planner supersedes them
        self._num_samples[:] = out["num_samples"]
        return {name: torch.from_numpy(np.ascontiguousarray(out[name]))
                for name in PLANNER_SUMMARY_DTYPE.names if name != "reserved"}

    def append_ik_rows(self, ik_positions, jacobians, row_offsets, ids=None, stream=None):
        """More rows behind the resident IK tables of the listed planners of a Cartesian set
        (tpamd_planner_set_append_ik_rows*): listed planner k gets rows row_offsets[k]:row_offsets[k + 1]
        of ik_positions [rows][D] and jacobians [rows][6][D] behind its last row; limits, delta and
        path state stay. CUDA tensors take the _device entry and only enqueue on `stream`."""
        import torch
        off = _host(row_offsets, np.int32, what="row offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("row offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        rows, D = (int(off[-1]) if n else 0), self.D
        if _is_cuda(ik_positions):
            dev = ik_positions.device
            q = self._cuda(ik_positions, torch.float64, dev, (rows, D), "ik_positions")
            J = self._cuda(jacobians, torch.float64, dev, (rows, 6, D), "jacobians")
            _check(self._lib.tpamd_planner_set_append_ik_rows_device(
                self._handle(), n, _ptr(ida), _ptr(off), _ptr(q), _ptr(J), _stream_ptr(stream)),
                "tpamd_planner_set_append_ik_rows_device")
            return
        q = _host(ik_positions, np.float64, (rows, D), "ik_positions")
        J = _host(jacobians, np.float64, (rows, 6, D), "jacobians")
        _check(self._lib.tpamd_planner_set_append_ik_rows(self._handle(), n, _ptr(ida), _ptr(off), _ptr(q), _ptr(J)),
               "tpamd_planner_set_append_ik_rows")

    def _plan_streaming(self, start_ns, horizon_ns):
        s = _host(np.broadcast_to(_host(start_ns, np.int64), (self.B,)), np.int64)
        h = _host(np.broadcast_to(_host(horizon_ns, np.int64), (self.B,)), np.int64)
        out = np.zeros(self.B, dtype=PLANNER_SUMMARY_DTYPE)
        need = np.zeros((2, self.B), dtype=np.int32)
        _check(self._lib.tpamd_planner_set_plan_streaming(self._handle(), _ptr(s), _ptr(h), out.ctypes.data,
                                                          _ptr(need[0]), _ptr(need[1]), None),
               "tpamd_planner_set_plan_streaming")
        return self._summary(out), need[0], need[1]

    def plan_resume(self):
        """tpamd_planner_set_plan_resume: the planners that wait for rows re-enter the window loop.
        Returns (summary dict as plan(), need_first [B], need_count [B] int32 numpy)."""
        out = np.zeros(self.B, dtype=PLANNER_SUMMARY_DTYPE)
        need = np.zeros((2, self.B), dtype=np.int32)
        _check(self._lib.tpamd_planner_set_plan_resume(self._handle(), out.ctypes.data, _ptr(need[0]), _ptr(need[1]),
                                                       None), "tpamd_planner_set_plan_resume")
        return self._summary(out), need[0], need[1]

    def plan_streaming(self, start_ns, horizon_ns, ik=None, lookahead_rows=0, discard=False):
        """Plan with IK tables that grow as TimeableCartesianSplinePath::SamplePath grows them. Returns
        (summary, need_first, need_count) as plan_resume does. Without `ik` this is one
        tpamd_planner_set_plan_streaming call; the caller appends and resumes while need_count > 0.
        With `ik` (after set_pose_waypoints(..., streaming=True)) the whole loop runs here and the
        completed Plan is returned (need_count all zero): while planners wait, the targets of table
        rows need_first - 1 .. need_first + need_count + lookahead_rows - 1 (never past the whole
        table's tpamd_ik_table_rows) are sampled on the device from the resident fit,
        ik(pose_targets, joint_targets, row_offsets, seed_rows) solves them (the first row of every
        planner's run is the re-evaluated last resident row, as in the reference's callback;
        seed_rows [waiting][D] is that resident row, its initial value), everything but that first
        row is appended, and the plan resumes. Per-row data stays on the device; the host sends the
        two time arrays and, per round, the row offsets of the waiting planners (ints), and reads the
        summaries and need_*. Counters of the last call: self.last_stream_stats.
        discard=True: once the Plan is complete (nobody waits), every planner that has a table
        discards the rows below its safe floor (discard_ik_rows()), so the tables stop growing with
        the distance travelled; last_stream_stats gains discard_h2d (the ids, 4 B per planner),
        discard_d2h (the new first rows, 4 B per planner) and first_row [B]."""
        import torch
        summary, nf, nc = self._plan_streaming(start_ns, horizon_ns)
        h2d, d2h = self.last_plan_bytes()
        stats = dict(suspensions=0, appended_rows=0, h2d=[h2d], d2h=[d2h])
        self.last_stream_stats = stats
        if ik is None:
            if discard and not (nc > 0).any():
                self._discard_after_plan(stats)
            return summary, nf, nc
        if getattr(self, "_stream_fit", None) is None:
            raise TpamdError("plan_streaming with an IK needs set_pose_waypoints(..., streaming=True) first")
        fit, dl, full = self._stream_fit["fit"], self._stream_fit["delta"], self._stream_fit["full_rows"]
        while (nc > 0).any():
            wait = np.flatnonzero(nc > 0)
            cnt = np.minimum(nc[wait] + int(lookahead_rows), np.maximum(full[wait] - nf[wait], nc[wait])).astype(np.int64)
            # the fit is sampled in place: the planners that do not wait take no rows
            per = np.zeros(self.B, dtype=np.int64)
            per[wait] = cnt + 1
            first = np.zeros(self.B, dtype=np.int32)
            first[wait] = nf[wait] - 1
            pose_t, joint_t = self._engine.sample_ik_targets(
                fit, dl, np.concatenate([[0], np.cumsum(per)]).astype(np.int32), first_row=first)
            row_offsets = np.concatenate([[0], np.cumsum(cnt + 1)]).astype(np.int32)
            q, J = ik(pose_t, joint_t, row_offsets, torch.stack([self._stream_last[int(b)] for b in wait]))
            runs = [(int(row_offsets[k]) + 1, int(row_offsets[k + 1])) for k in range(wait.size)]
            for k, b in enumerate(wait):
                self._stream_last[int(b)] = q[runs[k][1] - 1]
            self.append_ik_rows(torch.cat([q[a:e] for a, e in runs]), torch.cat([J[a:e] for a, e in runs]),
                                np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32), ids=wait.astype(np.int32))
            stats["suspensions"] += int(wait.size)
            stats["appended_rows"] += int(cnt.sum())
            summary, nf, nc = self.plan_resume()
            h2d, d2h = self.last_plan_bytes()
            stats["h2d"].append(h2d)
            stats["d2h"].append(d2h)
        if discard:
            self._discard_after_plan(stats)
        return summary, nf, nc

    def _discard_after_plan(self, stats):
        has = np.array([b for b in range(self.B) if self.ik_table_info(b)[1] > 0], dtype=np.int32)
        first = np.zeros(self.B, dtype=np.int32)
        if has.size:
            first[has] = self.discard_ik_rows(ids=has)
        stats["discard_h2d"], stats["discard_d2h"] = 4 * int(has.size), 4 * int(has.size)
        stats["first_row"] = first

    def stop_parameters(self, time_ns, ids=None):
        """GetPathStopParameter(time) on the resident trajectories (tpamd_planner_set_stop_parameters):
        dict stop_parameter, duration [count] float64 and status [count] int32, CPU tensors."""
        import torch
        t = _host(time_ns, np.int64).reshape(-1)
        ida, n = self._ids(ids, t.shape[0])
        if t.shape[0] != n:
            raise TpamdError("one time per listed planner")
        s, dur, st = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
        _check(self._lib.tpamd_planner_set_stop_parameters(self._handle(), n, _ptr(ida), _ptr(t), _ptr(s), _ptr(dur),
                                                           _ptr(st)), "tpamd_planner_set_stop_parameters")
        return dict(stop_parameter=torch.from_numpy(s), duration=torch.from_numpy(dur), status=torch.from_numpy(st))

    def switch_paths(self, time_ns, waypoints, offsets, ids=None, keep_path_until=None, rounding=0.2):
        """The online path switch (tpamd_planner_set_switch_paths_rounded) at time_ns [count] onto
        waypoints[offsets[k]:offsets[k + 1]], the new control polygon rounded with the PathOptions
        radius `rounding`: dict stop_parameter, num_points, status (CPU tensors)."""
        import torch
        off = _host(offsets, np.int32).reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        t = _host(time_ns, np.int64).reshape(-1)
        if off.shape[0] != n + 1 or t.shape[0] != n:
            raise TpamdError("one time and count + 1 offsets for the listed planners")
        w = _host(waypoints, np.float64).reshape(-1, self.D)
        if w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        if not w.size:
            w = np.zeros((1, self.D))    # the entry takes a non-NULL array even without rows
        keep = _host(keep_path_until, np.float64, (n,), "keep_path_until")
        s, npts, st = np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        _check(self._lib.tpamd_planner_set_switch_paths_rounded(
            self._handle(), n, _ptr(ida), _ptr(t), _ptr(keep), _ptr(off), _ptr(w), float(rounding), _ptr(s), _ptr(npts),
            _ptr(st)), "tpamd_planner_set_switch_paths_rounded")
        return dict(stop_parameter=torch.from_numpy(s), num_points=torch.from_numpy(npts), status=torch.from_numpy(st))

    # ------------------------------------------------------------ checking the windows
    def set_checking(self, on=True):
        """Check every window the Plan calls solve against its constraint rows
        (tpamd_planner_set_set_checking; off by default)."""
        _check(self._lib.tpamd_planner_set_set_checking(self._handle(), 1 if on else 0),
               "tpamd_planner_set_set_checking")

    @property
    def checking(self):
        return bool(self._lib.tpamd_planner_set_checking(self._handle()))

    def check_results(self, ids=None):
        """The tpamd_planner_check record of each listed planner (all without ids) over the windows
        of its last Plan call: a numpy structured array of PLANNER_CHECK_DTYPE. Synchronises."""
        ida, n = self._ids(ids)
        out = np.zeros(max(n, 1), dtype=PLANNER_CHECK_DTYPE)
        _check(self._lib.tpamd_planner_set_check_results(self._handle(), n, _ptr(ida), _ptr(out)),
               "tpamd_planner_set_check_results")
        return out[:n]

    def check_results_device(self, out, ids=None, stream=None):
        """The same records into `out`, a contiguous CUDA uint8 tensor [count][48] (view it on the host
        with PLANNER_CHECK_DTYPE), enqueued on `stream` without synchronising: it can follow
        plan_async on that stream. ids: CUDA int32 [count] or None for planners 0 .. count-1."""
        import torch
        size = PLANNER_CHECK_DTYPE.itemsize
        if (not _is_cuda(out) or out.dtype != torch.uint8 or out.dim() != 2 or out.shape[1] != size or
                not out.is_contiguous()):
            raise TpamdError("out must be a contiguous CUDA uint8 tensor [count][%d]" % size)
        n = out.shape[0]
        idt = None if ids is None else self._cuda(ids, torch.int32, torch.device("cuda", self.device), (n,), "ids")
        _check(self._lib.tpamd_planner_set_check_results_device(self._handle(), n, _ptr(idt), _ptr(out),
                                                                _stream_ptr(stream)),
               "tpamd_planner_set_check_results_device")
        return out

    # ------------------------------------------------------------ readouts
    def sample_at_ticks(self, start_ns, step_ns, num_ticks, ids=None, q=None, qd=None, qdd=None, status=None,
                        stream=None, host=False):
        """Setpoints at control ticks start_ns[k] + j step_ns (tpamd_planner_set_sample_at_ticks*):
        q / qd / qdd [count][num_ticks][D] float64 and status [count][num_ticks] int32. Device
        variant (host=False): start_ns, ids and the outputs are CUDA tensors (outputs given or
        allocated; None for q / qd / qdd means not wanted unless none is given: then all three),
        enqueued on `stream`; ticks that are not OK keep their values. host=True: host arrays,
        synchronises. Returns dict q, qd, qdd, status."""
        import torch
        T = int(num_ticks)
        if not host:
            dev = torch.device("cuda", self.device)
            st0 = self._cuda(start_ns, torch.int64, dev, None, "start_ns").reshape(-1)
            n = st0.shape[0]
            idt = None if ids is None else self._cuda(ids, torch.int32, dev, (n,), "ids")
            if ids is None and n > self.B:
                raise TpamdError("more start times than planners")
            if q is None and qd is None and qdd is None:
                q, qd, qdd = (torch.full((n, T, self.D), float("nan"), dtype=torch.float64, device=dev)
                              for _ in range(3))
            for name, a in (("q", q), ("qd", qd), ("qdd", qdd)):
                if a is not None and (not _is_cuda(a) or tuple(a.shape) != (n, T, self.D) or
                                      a.dtype != torch.float64 or not a.is_contiguous()):
                    raise TpamdError("%s must be a contiguous CUDA float64 tensor [%d][%d][%d]" % (name, n, T, self.D))
            if status is None:
                status = torch.full((n, T), -1, dtype=torch.int32, device=dev)
            _check(self._lib.tpamd_planner_set_sample_at_ticks_device(
                self._handle(), n, _ptr(idt), _ptr(st0), int(step_ns), T, _ptr(q), _ptr(qd), _ptr(qdd),
                _ptr(status), _stream_ptr(stream)), "tpamd_planner_set_sample_at_ticks_device")
            return dict(q=q, qd=qd, qdd=qdd, status=status)
        st0 = _host(start_ns, np.int64).reshape(-1)
        ida, n = self._ids(ids, st0.shape[0])
        if st0.shape[0] != n:
            raise TpamdError("one start time per listed planner")
        out = {k: np.full((n, T, self.D), np.nan) for k in ("q", "qd", "qdd")}
        out["status"] = np.full((n, T), -1, dtype=np.int32)
        _check(self._lib.tpamd_planner_set_sample_at_ticks(
            self._handle(), n, _ptr(ida), _ptr(st0), int(step_ns), T, _ptr(out["q"]), _ptr(out["qd"]),
            _ptr(out["qdd"]), _ptr(out["status"])), "tpamd_planner_set_sample_at_ticks")
        return {k: torch.from_numpy(v) for k, v in out.items()}

    def download_trajectories(self, ids=None, stream=None):
        """The trajectories of the listed planners packed into CUDA tensors
        (tpamd_planner_set_download_trajectories_device, on `stream`): dict offsets [count + 1]
        int64 and time, s, sd, sdd [rows], q, qd, qdd [rows][D]; planner k's rows are
        offsets[k]:offsets[k + 1]. The rows are sized from the last plan's sample counts."""
        import torch
        dev = torch.device("cuda", self.device)
        ida, n = self._ids(ids)
        counts = self._sample_counts()
        rows = int(counts[ida].sum() if ida is not None else counts[:n].sum())
        f = dict(dtype=torch.float64, device=dev)
        out = dict(offsets=torch.zeros(n + 1, dtype=torch.int64, device=dev))
        for k in ("time", "s", "sd", "sdd"):
            out[k] = torch.empty(rows, **f)
        for k in ("q", "qd", "qdd"):
            out[k] = torch.empty(rows, self.D, **f)
        idt = None if ida is None else torch.from_numpy(ida).to(dev)
        _check(self._lib.tpamd_planner_set_download_trajectories_device(
            self._handle(), n, _ptr(idt), _ptr(out["offsets"]), rows,
            *[_ptr(out[k]) if rows else None for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd")],
            _stream_ptr(stream)), "tpamd_planner_set_download_trajectories_device")
        out["_ids"] = idt          # kept alive with the result until the stream has used it
        return out

    def stop_trajectories(self, time_ns, max_acceleration, time_step, ids=None, capacity=None, stream=None):
        """TrajectoryBuffer::StopBeforeTime on the resident trajectories
        (tpamd_planner_set_stop_trajectories_device, on `stream`), CUDA tensors: time_ns [count]
        int64, max_acceleration [count][D]. Returns dict status, keep [count] int32, offsets
        [count + 1] int64 and the segments' time [rows], q, qd, qdd [rows][D]. The rows are sized by
        `capacity` (default: the planners' sample counts plus 64 each); if the segments need more,
        the call is repeated with room for them (it changes no state)."""
        import torch
        dev = torch.device("cuda", self.device)
        t = self._cuda(time_ns, torch.int64, dev, None, "time_ns").reshape(-1)
        n = t.shape[0]
        idt = None if ids is None else self._cuda(ids, torch.int32, dev, (n,), "ids")
        if ids is None and n > self.B:
            raise TpamdError("more stop times than planners")
        am = self._cuda(max_acceleration, torch.float64, dev, (n, self.D), "max_acceleration")
        if capacity is None:
            counts = self._sample_counts()
            sel = counts[:n] if ids is None else counts[_host(ids, np.int64).reshape(-1)]
            capacity = int(sel.sum()) + 64 * n
        for _ in range(2):
            out = dict(status=torch.full((n,), -1, dtype=torch.int32, device=dev),
                       keep=torch.zeros(n, dtype=torch.int32, device=dev),
                       offsets=torch.zeros(n + 1, dtype=torch.int64, device=dev),
                       time=torch.empty(capacity, dtype=torch.float64, device=dev))
            for k in ("q", "qd", "qdd"):
                out[k] = torch.empty(capacity, self.D, dtype=torch.float64, device=dev)
            _check(self._lib.tpamd_planner_set_stop_trajectories_device(
                self._handle(), n, _ptr(idt), _ptr(t), _ptr(am), float(time_step), _ptr(out["status"]),
                _ptr(out["keep"]), _ptr(out["offsets"]), int(capacity),
                *[_ptr(out[k]) if capacity else None for k in ("time", "q", "qd", "qdd")],
                _stream_ptr(stream)), "tpamd_planner_set_stop_trajectories_device")
            rows = int(out["offsets"][-1].item()) if n else 0
            if rows <= capacity:
                break
            capacity = rows
        for k in ("time", "q", "qd", "qdd"):
            out[k] = out[k][:rows]
        return out


    # ------------------------------------------------------------ state records
    def state_info(self, ids=None):
        """The record size and the counts of each listed planner (all without ids)
        (tpamd_planner_set_state_info): a numpy structured array of PLANNER_STATE_INFO_DTYPE.
        Synchronises."""
        ida, n = self._ids(ids)
        out = np.zeros(max(n, 1), dtype=PLANNER_STATE_INFO_DTYPE)
        _check(self._lib.tpamd_planner_set_state_info(self._handle(), n, _ptr(ida), _ptr(out)),
               "tpamd_planner_set_state_info")
        return out[:n]

    @property
    def state_bytes_bound(self):
        """The largest state record the set's current capacities allow."""
        return int(self._lib.tpamd_planner_set_state_bytes_bound(self._handle()))

    def export_state(self, ids=None, out=None, offsets=None, stream=None):
        """The state records of the listed planners (all without ids) packed into a CUDA uint8
        tensor (tpamd_planner_set_export_state_device, enqueued on `stream`). Returns (blob, offsets):
        record k is blob[offsets[k]:offsets[k + 1]], offsets a CPU int64 tensor [count + 1]; the
        per-planner statuses are self.last_export_status (CUDA int32 [count]). Without `offsets` the records are sized exactly with state_info(), which
        synchronises; with `offsets` (int64 [count + 1], multiples of 16, e.g. steps of
        state_bytes_bound) nothing comes to the host and a planner whose slot is too small gets
        PLAN_RESOURCE_EXHAUSTED. `out`: a contiguous CUDA uint8 tensor of at least offsets[-1]
        bytes to write into."""
        import torch
        dev = torch.device("cuda", self.device)
        ida, n = self._ids(ids)
        if offsets is None:
            sizes = self.state_info(ida)["bytes"] if ida is not None else self.state_info()["bytes"]
            off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        else:
            off = _host(offsets, np.int64, (n + 1,), "offsets")
        total = int(off[-1]) if n else 0
        if out is None:
            out = torch.zeros(max(total, 16), dtype=torch.uint8, device=dev)
        elif (not _is_cuda(out) or out.dtype != torch.uint8 or not out.is_contiguous() or out.numel() < total or
              out.data_ptr() % 16):
            raise TpamdError("out must be a contiguous, 16-byte aligned CUDA uint8 tensor of %d bytes" % total)
        st = torch.cuda.current_stream(dev) if stream is None else stream
        if st != torch.cuda.current_stream(dev):      # the fills and copies ran on the current stream
            st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            idt = None if ida is None else torch.from_numpy(ida).to(dev)
            offt = torch.from_numpy(off).to(dev)
            status = torch.full((n,), -1, dtype=torch.int32, device=dev)
        _check(self._lib.tpamd_planner_set_export_state_device(
            self._handle(), n, _ptr(idt), _ptr(out), _ptr(offt), _ptr(status), _stream_ptr(st)),
            "tpamd_planner_set_export_state_device")
        self.last_export_status = status
        self._export_keep = (idt, offt)      # alive until the stream has read them
        return out[:total], torch.from_numpy(off)

    def import_state(self, blob, offsets, ids=None, stream=None):
        """The listed planners (0 .. count-1 without ids, each listed once) take the states of the
        records blob[offsets[k]:offsets[k + 1]]. A CUDA `blob` goes through
        tpamd_planner_set_import_state_device, enqueued on `stream`: nothing is allocated, a record
        that needs more capacity than reserve() has provided gets PLAN_RESOURCE_EXHAUSTED and its
        planner keeps its state; returns dict status (CUDA int32 [count]) and summary (CUDA uint8
        [count][56], PLANNER_SUMMARY_DTYPE); the host-side sample counts are refreshed from that
        summary tensor by the first method that needs them (download_trajectories, stop_trajectories
        without a capacity), which synchronises the import's stream then. A host `blob` (numpy uint8 or CPU tensor) goes through
        tpamd_planner_set_import_state_host, which validates every record first, grows the set as
        needed and synchronises; returns dict status (CPU int32) plus the summary fields of plan()."""
        import torch
        off = _host(offsets, np.int64, what="offsets").reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("offsets need count + 1 = %d entries, got %d" % (n + 1, off.shape[0]))
        if self._pending is not None:
            raise TpamdError("a plan_async call is in flight (PlanHandle.result())")
        total = int(off[-1]) if n else 0
        if _is_cuda(blob):
            dev = blob.device
            if blob.dtype != torch.uint8 or not blob.is_contiguous() or blob.numel() < total or blob.data_ptr() % 16:
                raise TpamdError("blob must be a contiguous, 16-byte aligned CUDA uint8 tensor of %d bytes" % total)
            st = torch.cuda.current_stream(dev) if stream is None else stream
            if st != torch.cuda.current_stream(dev):
                st.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(st):
                idt = None if ida is None else torch.from_numpy(ida).to(dev)
                offt = offsets if (_is_cuda(offsets) and offsets.dtype == torch.int64 and offsets.is_contiguous()) \
                    else torch.from_numpy(off).to(dev)
                status = torch.full((n,), -1, dtype=torch.int32, device=dev)
                summary = torch.zeros((n, PLANNER_SUMMARY_DTYPE.itemsize), dtype=torch.uint8, device=dev)
            _check(self._lib.tpamd_planner_set_import_state_device(
                self._handle(), n, _ptr(idt), _ptr(blob), _ptr(offt), _ptr(summary), _ptr(status), _stream_ptr(st)),
                "tpamd_planner_set_import_state_device")
            self._imports.append((st, summary, status, np.arange(n) if ida is None else ida.astype(np.int64)))
            return dict(status=status, summary=summary, _keep=(idt, offt, blob))
        b = _host(blob, np.uint8, what="blob").reshape(-1)
        if b.shape[0] < total:
            raise TpamdError("blob has %d bytes, offsets end at %d" % (b.shape[0], total))
        status = np.full(n, -1, dtype=np.int32)
        out = np.zeros(max(n, 1), dtype=PLANNER_SUMMARY_DTYPE)
        _check(self._lib.tpamd_planner_set_import_state_host(
            self._handle(), n, _ptr(ida), _ptr(b), _ptr(off), out.ctypes.data, _ptr(status)),
            "tpamd_planner_set_import_state_host")
        return self._state_result(out[:n], status, ida)

    def _state_result(self, out, status, ida):
        import torch
        self._settle_imports()         # an earlier device import first: this call is the later one
        sel = np.arange(out.shape[0]) if ida is None else ida
        ok = status == 0
        self._num_samples[sel[ok]] = out["num_samples"][ok]
        res = {name: torch.from_numpy(np.ascontiguousarray(out[name]))
               for name in PLANNER_SUMMARY_DTYPE.names if name != "reserved"}
        res["status"] = torch.from_numpy(status)
        return res

    def copy_from(self, other, src_ids=None, dst_ids=None):
        """Planner src_ids[k] of `other` becomes planner dst_ids[k] of this set
        (tpamd_planner_set_copy_planners; None: 0 .. count-1, count from the ids given, else the
        smaller set's size). `other` may be this set: any permutation is legal. Grows this set as
        needed; synchronises. Returns dict status (CPU int32) plus the summary fields of plan()."""
        if self._pending is not None or other._pending is not None:
            raise TpamdError("a plan_async call is in flight (PlanHandle.result())")
        src = None if src_ids is None else _host(src_ids, np.int32, what="src_ids").reshape(-1)
        dst = None if dst_ids is None else _host(dst_ids, np.int32, what="dst_ids").reshape(-1)
        n = src.shape[0] if src is not None else (dst.shape[0] if dst is not None else min(self.B, other.B))
        if (src is not None and src.shape[0] != n) or (dst is not None and dst.shape[0] != n):
            raise TpamdError("src_ids and dst_ids must list the same number of planners")
        status = np.full(n, -1, dtype=np.int32)
        out = np.zeros(max(n, 1), dtype=PLANNER_SUMMARY_DTYPE)
        _check(self._lib.tpamd_planner_set_copy_planners(
            self._handle(), _ptr(dst), other._handle(), _ptr(src), n, out.ctypes.data, _ptr(status)),
            "tpamd_planner_set_copy_planners")
        return self._state_result(out[:n], status, dst)


class PlanHandle:
    """A PlannerSet.plan_async call in flight: `summary` (the tpamd_planner_summary records as
    bytes) and `info` (tpamd_plan_device_info as int32) are CUDA tensors the stream writes."""

    def __init__(self, planner_set, stream, summary, info, keep):
        self._set, self._stream, self.summary, self.info = planner_set, stream, summary, info
        self._keep = keep              # the time arguments stay alive until the stream has read them
        self._result = None

    def result(self):
        """Synchronises the call's stream; the dict plan() returns, plus `info` (dict of ints).
        Refreshes the set's host-side sample counts."""
        if self._result is None:
            self._stream.synchronize()
            out = self.summary.cpu().numpy().view(PLANNER_SUMMARY_DTYPE).copy()
            info = self.info.cpu().numpy()
            if self._set._pending is self:
                self._set._pending = None
                self._result = self._set._summary(out)
            else:                      # the set was closed meanwhile: the records alone
                import torch
                self._result = {name: torch.from_numpy(np.ascontiguousarray(out[name]))
                                for name in PLANNER_SUMMARY_DTYPE.names if name != "reserved"}
            self._result["info"] = {k: int(info[j]) for j, k in enumerate(PLAN_DEVICE_INFO_FIELDS)}
            self._keep = None
        return self._result


class BufferSet:
    """B trajectory buffers (TrajectoryBuffer: samples of time, q, qd, qdd, a sample count and a
    sequence number each) resident on the device (include/tpamd.h tpamd_buffer_set_*). It is what
    a controller executes: after each plan the new trajectory is spliced in, consumed samples are
    discarded, setpoints are read at control ticks, and a stop changes the buffer:

        with BufferSet(engine, B, D, capacity=2048) as bs:
            ps.plan(start_ns, horizon_ns)
            bs.insert_from(ps)                                  # device to device
            bs.discard_before(now_ns)
            sp = bs.sample_at_ticks(now_ns, step_ns, 1)         # CUDA [B][1][D]

    Every array is a CUDA tensor and every call goes through the _device entry on torch's current
    stream (or `stream`); ids (int32 CUDA tensor, each buffer listed once in calls that change
    buffers; None: buffers 0..count-1). Results are dicts of CUDA tensors; per-buffer outcomes are
    TPAMD_PLAN_* codes in `status` (100, TPAMD_PLAN_MORE: no room, call reserve()). Errors of the
    call itself raise TpamdError."""

    def __init__(self, engine, num_buffers, num_dofs, capacity=0, timestep_tolerance=1e-6):
        self._lib = load_library()
        self.B, self.D = int(num_buffers), int(num_dofs)
        self.device = engine.device
        h = C.c_void_p()
        _check(self._lib.tpamd_buffer_set_create(engine._h, self.B, self.D, int(capacity), float(timestep_tolerance),
                                                 C.byref(h)), "tpamd_buffer_set_create")
        self._engine = engine          # the set must not outlive its engine
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tpamd_buffer_set_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _handle(self):
        if not getattr(self, "_h", None):
            raise TpamdError("the buffer set is closed")
        return self._h

    @property
    def device_bytes(self):
        return self._lib.tpamd_buffer_set_device_bytes(self._handle())

    @property
    def capacity(self):
        return self._lib.tpamd_buffer_set_capacity(self._handle())

    def reserve(self, capacity):
        """Room for `capacity` samples per buffer (synchronises; the other calls never allocate)."""
        _check(self._lib.tpamd_buffer_set_reserve(self._handle(), int(capacity)), "tpamd_buffer_set_reserve")

    def _dev(self):
        import torch
        return torch.device("cuda", self.device)

    def _t(self, x, dtype, shape, what):
        import torch
        if x is None:
            return None
        if not _is_cuda(x):
            x = torch.as_tensor(x).to(self._dev())
        x = x.to(dtype).contiguous()
        if shape is not None and tuple(x.shape) != tuple(shape):
            raise TpamdError("%s has shape %s, expected %s" % (what, tuple(x.shape), tuple(shape)))
        return x

    def _list(self, ids, count):
        import torch
        if ids is None:
            n = self.B if count is None else int(count)
            if n > self.B:
                raise TpamdError("more entries than buffers")
            return None, n
        idt = self._t(ids, torch.int32, None, "ids").reshape(-1)
        if count is not None and idt.shape[0] != count:
            raise TpamdError("one entry per listed buffer")
        return idt, idt.shape[0]

    def _status(self, n):
        import torch
        return torch.full((n,), -1, dtype=torch.int32, device=self._dev())

    def _times(self, time_ns, time_sec):
        import torch
        if (time_ns is None) == (time_sec is None):
            raise TpamdError("give the time either in nanoseconds or in seconds")
        if time_ns is not None:
            t = self._t(time_ns, torch.int64, None, "time_ns").reshape(-1)
            return t, None, t.shape[0]
        t = self._t(time_sec, torch.float64, None, "time_sec").reshape(-1)
        return None, t, t.shape[0]

    def insert(self, time, q, qd, qdd, offsets, ids=None, stream=None):
        """InsertSegment: buffer k receives rows offsets[k]:offsets[k + 1] of time [rows] and q, qd,
        qdd [rows][D], the packed layout of PlannerSet.download_trajectories / stop_trajectories
        (their dicts can be passed on as they are). Returns dict status."""
        import torch
        off = self._t(offsets, torch.int64, None, "offsets").reshape(-1)
        idt, n = self._list(ids, off.shape[0] - 1)
        tm = self._t(time, torch.float64, None, "time").reshape(-1)
        rows = tm.shape[0]
        arr = [self._t(a, torch.float64, (rows, self.D), k) for k, a in (("q", q), ("qd", qd), ("qdd", qdd))]
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_insert_device(
            self._handle(), n, _ptr(idt), _ptr(off), rows, *[_ptr(a) if rows else None for a in [tm] + arr],
            _ptr(st), _stream_ptr(stream)), "tpamd_buffer_set_insert_device")
        return dict(status=st, _keep=(idt, off, tm, arr))

    def insert_from(self, planner_set, ids=None, planner_ids=None, stream=None):
        """InsertSegment of the resident trajectories of a PlannerSet on the same engine, device to
        device: buffer ids[k] receives planner planner_ids[k]'s trajectory. Returns dict status."""
        import torch
        pid = None if planner_ids is None else self._t(planner_ids, torch.int32, None, "planner_ids").reshape(-1)
        idt, n = self._list(ids, None if pid is None else pid.shape[0])
        if pid is None and ids is None:
            n = min(self.B, planner_set.B)
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_insert_from_planner_set_device(
            self._handle(), planner_set._handle(), n, _ptr(idt), _ptr(pid), _ptr(st), _stream_ptr(stream)),
            "tpamd_buffer_set_insert_from_planner_set_device")
        return dict(status=st, _keep=(idt, pid))

    def append_sample(self, time, q, qd, qdd, ids=None, stream=None):
        """AppendSample: time [count], q, qd, qdd [count][D]. Returns dict status."""
        import torch
        tm = self._t(time, torch.float64, None, "time").reshape(-1)
        idt, n = self._list(ids, tm.shape[0])
        arr = [self._t(a, torch.float64, (n, self.D), k) for k, a in (("q", q), ("qd", qd), ("qdd", qdd))]
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_append_sample_device(
            self._handle(), n, _ptr(idt), _ptr(tm), *[_ptr(a) for a in arr], _ptr(st), _stream_ptr(stream)),
            "tpamd_buffer_set_append_sample_device")
        return dict(status=st, _keep=(idt, tm, arr))

    def discard_before(self, time_ns=None, time_sec=None, ids=None, stream=None):
        """DiscardSegmentBefore at time_ns [count] (int64) or time_sec [count]. Returns dict status."""
        tn, ts, n = self._times(time_ns, time_sec)
        idt, n = self._list(ids, n)
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_discard_before_device(
            self._handle(), n, _ptr(idt), _ptr(tn), _ptr(ts), _ptr(st), _stream_ptr(stream)),
            "tpamd_buffer_set_discard_before_device")
        return dict(status=st, _keep=(idt, tn, ts))

    def stop_before_time(self, max_acceleration, time_step, time_ns=None, time_sec=None, ids=None, stream=None):
        """StopBeforeTime in place: max_acceleration [count][D]. Returns dict status."""
        import torch
        tn, ts, n = self._times(time_ns, time_sec)
        idt, n = self._list(ids, n)
        am = self._t(max_acceleration, torch.float64, (n, self.D), "max_acceleration")
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_stop_before_time_device(
            self._handle(), n, _ptr(idt), _ptr(tn), _ptr(ts), _ptr(am), float(time_step), _ptr(st),
            _stream_ptr(stream)), "tpamd_buffer_set_stop_before_time_device")
        return dict(status=st, _keep=(idt, tn, ts, am))

    def sample_at_ticks(self, start_ns, step_ns, num_ticks, ids=None, stream=None):
        """Setpoints at ticks start_ns[k] + j step_ns: dict q, qd, qdd [count][num_ticks][D] (NaN
        where the tick is not OK) and status [count][num_ticks]."""
        import torch
        s0 = self._t(start_ns, torch.int64, None, "start_ns").reshape(-1)
        idt, n = self._list(ids, s0.shape[0])
        T = int(num_ticks)
        out = {k: torch.full((n, T, self.D), float("nan"), dtype=torch.float64, device=self._dev())
               for k in ("q", "qd", "qdd")}
        out["status"] = torch.full((n, T), -1, dtype=torch.int32, device=self._dev())
        _check(self._lib.tpamd_buffer_set_sample_at_ticks_device(
            self._handle(), n, _ptr(idt), _ptr(s0), int(step_ns), T, _ptr(out["q"]), _ptr(out["qd"]),
            _ptr(out["qdd"]), _ptr(out["status"]), _stream_ptr(stream)), "tpamd_buffer_set_sample_at_ticks_device")
        out["_keep"] = (idt, s0)
        return out

    def add_offset(self, offset_ns=None, offset_sec=None, ids=None, stream=None):
        """AddOffsetToTimestamps: offset_sec [count], or offset_ns [count] (a duration)."""
        tn, ts, n = self._times(offset_ns, offset_sec)
        idt, n = self._list(ids, n)
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_add_offset_device(
            self._handle(), n, _ptr(idt), _ptr(tn), _ptr(ts), _ptr(st), _stream_ptr(stream)),
            "tpamd_buffer_set_add_offset_device")
        return dict(status=st, _keep=(idt, tn, ts))

    def clear(self, ids=None, stream=None):
        idt, n = self._list(ids, None)
        st = self._status(n)
        _check(self._lib.tpamd_buffer_set_clear_device(self._handle(), n, _ptr(idt), _ptr(st), _stream_ptr(stream)),
               "tpamd_buffer_set_clear_device")
        return dict(status=st, _keep=(idt,))

    def info(self, time_ns=None, ids=None, stream=None):
        """dict num_samples, sequence (int32), start_ns, end_ns (int64) and, with time_ns,
        positions_up_to (the size of GetPositionsUpToTime) per listed buffer."""
        import torch
        tn = None if time_ns is None else self._t(time_ns, torch.int64, None, "time_ns").reshape(-1)
        idt, n = self._list(ids, None if tn is None else tn.shape[0])
        dev = self._dev()
        out = dict(num_samples=torch.zeros(n, dtype=torch.int32, device=dev),
                   sequence=torch.zeros(n, dtype=torch.int32, device=dev),
                   start_ns=torch.zeros(n, dtype=torch.int64, device=dev),
                   end_ns=torch.zeros(n, dtype=torch.int64, device=dev))
        if tn is not None:
            out["positions_up_to"] = torch.zeros(n, dtype=torch.int32, device=dev)
        _check(self._lib.tpamd_buffer_set_info_device(
            self._handle(), n, _ptr(idt), _ptr(tn), _ptr(out["num_samples"]), _ptr(out["sequence"]),
            _ptr(out["start_ns"]), _ptr(out["end_ns"]), _ptr(out.get("positions_up_to")), _stream_ptr(stream)),
            "tpamd_buffer_set_info_device")
        out["_keep"] = (idt, tn)
        return out

    def download(self, ids=None, capacity=None, stream=None):
        """The listed buffers' samples packed into CUDA tensors: dict offsets [count + 1] and time
        [rows], q, qd, qdd [rows][D]; buffer k's rows are offsets[k]:offsets[k + 1]. `capacity`
        rows are allocated (default: count x the set's capacity)."""
        import torch
        idt, n = self._list(ids, None)
        dev = self._dev()
        rows = int(capacity) if capacity is not None else n * self.capacity
        out = dict(offsets=torch.zeros(n + 1, dtype=torch.int64, device=dev),
                   time=torch.empty(rows, dtype=torch.float64, device=dev))
        for k in ("q", "qd", "qdd"):
            out[k] = torch.empty(rows, self.D, dtype=torch.float64, device=dev)
        _check(self._lib.tpamd_buffer_set_download_device(
            self._handle(), n, _ptr(idt), _ptr(out["offsets"]), rows,
            *[_ptr(out[k]) if rows else None for k in ("time", "q", "qd", "qdd")], _stream_ptr(stream)),
            "tpamd_buffer_set_download_device")
        total = int(out["offsets"][-1].item())
        if total > rows:
            raise TpamdError("the buffers hold %d rows, capacity %d" % (total, rows))
        for k in ("time", "q", "qd", "qdd"):
            out[k] = out[k][:total]
        out["_keep"] = (idt,)
        return out


def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


def alloc_joint_outputs(B, N, D, device, with_q=True, with_derivs=True):
    import torch
    f = dict(dtype=torch.float64, device=device)
    out = dict(time=torch.empty(B, N, **f), s=torch.empty(B, N, **f), sd=torch.empty(B, N, **f),
               sdd=torch.empty(B, N, **f),
               last_extremal_index=torch.zeros(B, dtype=torch.int32, device=device),
               max_time_increment=torch.zeros(B, **f),
               status=torch.full((B,), -1, dtype=torch.int32, device=device))
    if with_q:
        out["q"] = torch.empty(B, N, D, **f)
    if with_derivs:
        out["qd"] = torch.empty(B, N, D, **f)
        out["qdd"] = torch.empty(B, N, D, **f)
    return out


def upload_joint_batch(batch, device):
    import torch
    keys = ("knots", "control_points", "vmax", "amax", "path_start", "delta", "sd_start",
            "time_start")
    t = {k: torch.from_numpy(np.ascontiguousarray(batch[k])).to(device) for k in keys}
    return dict(knots=t["knots"], control_points=t["control_points"], max_velocity=t["vmax"],
                max_acceleration=t["amax"], path_start=t["path_start"], delta=t["delta"],
                sd_start=t["sd_start"], time_start=t["time_start"])

"""ctypes binding of the engine's C-ABI (include/tpamd.h -> csrc/libtpamd.so).

Plumbing only: device memory, streams and torch.distributed come from PyTorch;
all computation happens in the hand-written HIP kernels behind the C-ABI. There
is NO CPU fallback: if the shared library or a HIP device is missing, every
entry point raises.
"""
import ctypes as C
import os

import numpy as np

from . import abi as _abi
from .abi import (  # noqa: F401  (the declarations and the build: re-exported)
    ABI_SYMBOLS, DIAG_SO, HIPCC_FLAGS, MULTI_SO, PLAN_DEVICE_INFO_FIELDS, PLAN_RESOURCE_EXHAUSTED,
    PLANNER_CHECK_DTYPE, PLANNER_STATE_INFO_DTYPE, PLANNER_SUMMARY_DTYPE, REFINE_NO_SLOT, REFINE_NOTHING,
    REFINE_TOO_LONG, SWEEP_INSTANCES, TpamdError, _CartesianBatch, _CartesianInputs, _CheckOutputs,
    _FastestStopArgs, _JointBatch, _JointInputs, _PathOutputs, _PlanDeviceInfo, _PlannerCheck, _PlannerSetConfig,
    _RefineOptions, _RefineOutputs, _ResampleArgs, _RowsBatch, _RowsInputs, _Solution, _StopTrajectoryArgs,
    _WaypointBatch, _WaypointFitOutputs, _WaypointInputs, _ptr)

_SO = os.environ.get("TPAMD_LIBRARY") or os.path.join(_abi._CSRC, "libtpamd.so")   # override: A/B builds

PATH_STATUS = {
    0: "ok", 2: "infeasible_bounds", 3: "s_range", 4: "sd_start_negative",
    5: "lower_ge_upper", 6: "too_few_samples", 7: "no_connection", 8: "nan_sd2",
    9: "nonzero_end", 10: "crit_index_zero", 11: "no_waypoints", 12: "sweep_poll_expired",
}

KERNEL_SWEEP = 4

# the keys of a Cartesian inputs dict, in struct order (tests fill the struct from them)
_CARTESIAN_INPUT_KEYS = _CartesianInputs._keys_


def build_library(force=False, verbose=False, extra_flags=(), output=None):
    """Compile csrc/ for gfx950 with hipcc (cross-compiles without a GPU)."""
    global _SO
    if output is not None:
        _SO = output
    return _abi._compile(_SO, extra_flags, force, verbose)


def build_multi_library(force=False, verbose=False):
    """libtpamd_multi.so (include/tpamd_multi.h): several devices from one process, on top of
    libtpamd.so and RCCL. Host code only."""
    return _abi._compile_multi(_SO, force, verbose)


def build_diagnostic_library(force=False, verbose=False):
    """The -DTPAMD_DIAG variant: in-kernel cycle counters and the literal cross-checks of the
    sweep kernel's shortcuts (tests/test_gpu_parity.py, tools/gpu_diag.py). Not the product."""
    return _abi._compile(DIAG_SO, ("-DTPAMD_DIAG",), force, verbose)


_LIB = None


def load_library():
    """libtpamd.so with the restype and argtypes of every function include/tpamd.h declares."""
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
    _LIB = _abi.declare(C.CDLL(_SO))
    return _LIB


def _check(rc, what):
    if rc != 0:
        raise TpamdError("%s failed: %d (%s)" % (what, rc,
                                                load_library().tpamd_error_string(rc).decode()))


def _stream_ptr(stream):
    if stream is None:
        import torch
        return C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return C.c_void_p(stream)
    return C.c_void_p(stream.cuda_stream)


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


def _cpu_array(x, dtype):
    """A C-contiguous numpy array of a CPU tensor or array (host=True arguments); None stays None."""
    return None if x is None else np.ascontiguousarray(x.numpy() if hasattr(x, "numpy") else x, dtype=dtype)


# ---------------------------------------------------------------- array backends
# A method that serves host arrays through a host entry and CUDA tensors through a _device entry
# has one body; what differs -- how an argument is coerced, how an output is made and in what type
# results go back -- is behind one of these two.
class _Numpy:
    """Host arrays: C-contiguous numpy arrays, handed back as they are or as CPU tensors."""
    host = True
    device = None
    float64, int32, int64 = np.float64, np.int32, np.int64
    array = staticmethod(_host)

    def __init__(self, as_torch=False):
        self.as_torch = as_torch

    def per(self, x, n, what):
        """One float64 per entry, from [n] values or one number."""
        return _host(np.broadcast_to(_host(x, np.float64), (n,)), np.float64, (n,), what)

    def zeros(self, shape, dtype=np.float64):
        return np.zeros(shape, dtype=dtype)

    def full(self, shape, value, dtype=np.float64):
        return np.full(shape, value, dtype=dtype)

    def result(self, a):
        if self.as_torch:
            import torch
            return torch.from_numpy(a)
        return a


class _Torch:
    """Contiguous tensors on one CUDA device, handed back as they are."""
    host = False

    def __init__(self, device):
        import torch
        self.torch, self.device = torch, device
        self.float64, self.int32, self.int64 = torch.float64, torch.int32, torch.int64

    def array(self, x, dtype, shape=None, what="argument"):
        if x is None:
            return None
        t = self.torch.as_tensor(x, dtype=dtype, device=self.device).contiguous()
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise TpamdError("%s has shape %s, expected %s" % (what, tuple(t.shape), tuple(shape)))
        return t

    def per(self, x, n, what):
        x = x if hasattr(x, "shape") else self.torch.full((n,), float(x), dtype=self.float64)
        return self.array(x, self.float64, (n,), what)

    def zeros(self, shape, dtype=None):
        return self.torch.zeros(shape, dtype=dtype or self.float64, device=self.device)

    def full(self, shape, value, dtype=None):
        shape = shape if isinstance(shape, tuple) else (shape,)
        return self.torch.full(shape, value, dtype=dtype or self.float64, device=self.device)

    def result(self, t):
        return t


_NUMPY, _NUMPY_AS_TORCH = _Numpy(), _Numpy(as_torch=True)


def _backend(x, as_torch=False):
    """The backend of a call whose argument x decides the side: x's device if it is a CUDA tensor."""
    if _is_cuda(x):
        return _Torch(x.device)
    return _NUMPY_AS_TORCH if as_torch else _NUMPY


def _waypoint_offsets(offsets):
    """Host int32 waypoint offsets [B + 1] and B."""
    off = _host(offsets, np.int32, what="waypoint offsets").reshape(-1)
    if off.shape[0] < 1:
        raise TpamdError("waypoint offsets need at least one entry")
    return off, off.shape[0] - 1


def _fit_sizes(off):
    """Control points and knots of the splines fitted to W = diff(off) waypoints each: (sum P, sum P + 3)."""
    W = np.diff(off.astype(np.int64))
    npts = np.where(W < 1, 0, np.where(W == 1, 4, 3 * W - 2))
    return int(npts.sum()), int((npts + 3 * (npts > 0)).sum())


# ---------------------------------------------------------------- the objects behind a C handle
# what _Native._call hands to ctypes unchanged: numbers, struct mirrors (and arrays of them), byref()
# results and stream pointers; everything else is an array or a tensor and goes in as its address
_AS_IS = (int, float, C.Structure, C.Array, C._SimpleCData, type(C.byref(C.c_int())), np.integer, np.floating)
_AS_IS_TYPES = frozenset([type(None), int, float, C.c_void_p, _AS_IS[5]] + list(_abi.MIRRORS.values()))   # the usual


class _Native:
    """What Engine, PlannerSet and BufferSet share: the C handle with its lifecycle, and the one way
    an entry point is called."""
    _kind = _destroy = None          # "planner set", "tpamd_planner_set_destroy"
    _host_suffix = "_host"           # the host entry of a pair: tpamd_x_host (engine) or tpamd_x (sets)

    def _adopt(self, handle):
        self._h = handle
        self._keepalive = {}

    def _release(self):
        """What must happen before the handle is destroyed."""

    def close(self):
        if getattr(self, "_h", None):
            self._release()
            getattr(self._lib, self._destroy)(self._h)
            self._h = None
            self._keepalive = {}

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
            raise TpamdError("the %s is closed" % self._kind)
        return self._h

    def _device(self):
        """The torch backend of this object's GPU."""
        import torch
        return _Torch(torch.device("cuda", self.device))

    def _call(self, entry, *args, host=None, stream=None, keep=()):
        """One C-ABI call on this object's handle; a non-zero return raises TpamdError with the
        symbol's name. host None: `entry` is the symbol. host True / False: the symbol is the host /
        _device entry of the pair `entry` names, and the _device entry gets `stream` as its last
        argument. Arrays and tensors go in as they are (None: NULL), struct mirrors by reference.
        A _device call only enqueues, so what it was handed (and `keep`: what the structs point to
        that the caller does not own) stays referenced until the next call of the same entry."""
        if host is None:
            name = entry
        elif host:
            name = entry + self._host_suffix
        else:
            name = entry + "_device"
            args += (_stream_ptr(stream),)
        rc = getattr(self._lib, name)(self._h or self._handle(), *[
            a if type(a) in _AS_IS_TYPES or isinstance(a, _AS_IS) else _ptr(a) for a in args])
        if rc:
            _check(rc, name)
        if not (host is None or host):
            self._keepalive[name] = args + keep if keep else args


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


class Engine(_Native):
    """One engine per GPU (tpamd_engine_create/destroy)."""
    _destroy = "tpamd_engine_destroy"

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        _check(self._lib.tpamd_engine_create(int(device), C.byref(h)), "tpamd_engine_create")
        self._adopt(h)
        self.device = int(device)

    def _handle(self):
        return self._h               # closed: NULL, which every entry refuses

    def reserve(self, num_paths, num_samples, num_rows):
        self._call("tpamd_engine_reserve", num_paths, num_samples, num_rows)

    def set_pipelining(self, mode=1):
        """0 off; 1: the sampling/LP kernel of a joint solve overlaps the previous solve's sweep;
        2: sweeps of consecutive solves overlap as well, outputs ordered by the next call or
        fence() (include/tpamd.h tpamd_engine_set_pipelining: inputs must be ready at call time)."""
        self._call("tpamd_engine_set_pipelining", int(mode))

    def fence(self, stream=None):
        """Order `stream` (default: torch's current stream) behind every solve issued so far."""
        self._call("tpamd_engine_fence", _stream_ptr(stream))

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
        self._call("tpamd_time_joint_paths", bt, _JointInputs.from_dict(inputs), _PathOutputs.from_dict(outputs),
                   host=host, stream=stream)

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
            jis[g] = _JointInputs.from_dict(grp["inputs"])
            pos[g] = _PathOutputs.from_dict(grp["outputs"])
        self._call("tpamd_time_joint_groups", G, bts, jis, pos, host=host, stream=stream)

    def sample_joint_paths(self, knots, control_points, path_start, delta, num_samples):
        """Host numpy arrays -> (q, q1, q2) [B][N][D]."""
        cp = np.ascontiguousarray(control_points, dtype=np.float64)
        kn = np.ascontiguousarray(knots, dtype=np.float64)
        B, P, D = cp.shape
        ps = np.ascontiguousarray(np.broadcast_to(path_start, (B,)), dtype=np.float64)
        dl = np.ascontiguousarray(np.broadcast_to(delta, (B,)), dtype=np.float64)
        out = [np.zeros((B, num_samples, D)) for _ in range(3)]
        self._call("tpamd_sample_joint_paths_host", B, D, int(num_samples), P, kn, cp, ps, dl, *out)
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
        ri, po = _RowsInputs.from_dict(inputs), _PathOutputs.from_dict(outputs)
        if num_samples_per_path is not None:
            ns = _int32_array(num_samples_per_path, B, "num_samples_per_path")
            self._call("tpamd_optimize_rows_ragged", bt, ri, ns, po, host=host, stream=stream)
        else:
            self._call("tpamd_optimize_rows", bt, ri, po, host=host, stream=stream)

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
        B, N, D = self._cartesian_shape(inputs, first_row, outputs["time"] if first_row is not None else None)
        ragged = num_samples_per_path is not None or first_row is not None
        if ragged:
            if num_samples_per_path is None:
                xp = _NUMPY if host else _Torch(ik.device)
                num_samples_per_path = xp.full(B, N, xp.int32)
            ns = _int32_array(num_samples_per_path, B, "num_samples_per_path")
            fr = None if first_row is None else _int32_array(first_row, B, "first_row")
        bt = _CartesianBatch(B, D, N, int(max_solver_loops), float(safety))
        ci, po = _CartesianInputs.from_dict(inputs), _PathOutputs.from_dict(outputs)
        if ragged:
            # (the host entry also takes the row count of the packed tables)
            rows = (int(ik.shape[0]) if fr is not None else 0,) if host else ()
            self._call("tpamd_time_cartesian_paths_ragged", bt, ci, ns, fr, *rows, po, host=host, stream=stream)
        else:
            self._call("tpamd_time_cartesian_paths", bt, ci, po, host=host, stream=stream)

    @staticmethod
    def _cartesian_shape(inputs, first_row, strided):
        """B, N, D of a Cartesian batch: of ik_positions [B][N][D], or, with packed row tables
        (first_row given), D of ik_positions [rows][D] and B, N of the [B][N] array `strided`."""
        ik = inputs["ik_positions"]
        if first_row is None:
            return ik.shape
        if len(ik.shape) != 2:
            raise TpamdError("packed inputs: ik_positions must be [rows][D]")
        rows, D = ik.shape
        B, N = strided.shape
        if inputs["jacobians"].shape[0] != rows:
            raise TpamdError("packed inputs: jacobians must have one [6][D] block per row")
        return B, N, D

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
        self._call("tpamd_sample_pose_splines_host", B, int(num_samples), P, kn, tr, ro, ps, dl, out)
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
        off, B = _waypoint_offsets(offsets)
        P, K = _fit_sizes(off)
        rows = int(off[-1])
        point_offsets = np.zeros(B + 1, dtype=np.int32)
        xp = _backend(pose_waypoints)
        pw = xp.array(pose_waypoints, xp.float64, (rows, 7), "pose_waypoints")
        if xp.host:      # D is whatever the second axis holds
            jw = xp.array(joint_waypoints, xp.float64, what="joint_waypoints")
            if jw.ndim != 2 or jw.shape[0] != rows:
                raise TpamdError("joint_waypoints has shape %s, expected (%d, D)" % (jw.shape, rows))
            D = jw.shape[1]
        else:
            D = int(joint_waypoints.shape[-1])
            jw = xp.array(joint_waypoints, xp.float64, (rows, D), "joint_waypoints")
        tr, rr = xp.per(translation_rounding, B, "translation_rounding"), xp.per(rotation_rounding, B,
                                                                                 "rotation_rounding")
        out = dict(knots=xp.zeros(K), translation_points=xp.zeros((P, 3)), rotation_points=xp.zeros((P, 4)),
                   joint_control_points=xp.zeros((P, D)), num_points=xp.zeros(B, xp.int32), path_end=xp.zeros(B),
                   status=xp.full(B, -1, xp.int32))
        self._call("tpamd_fit_pose_waypoints", B, D, off, pw, jw, tr, rr, out["knots"], out["translation_points"],
                   out["rotation_points"], out["joint_control_points"], out["num_points"], point_offsets,
                   out["path_end"], out["status"], host=xp.host, stream=stream)
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
        off, B = _waypoint_offsets(offsets)
        P, K = _fit_sizes(off)
        rows = int(off[-1])
        if waypoints.ndim != 2 or waypoints.shape[0] != rows:
            raise TpamdError("waypoints has shape %s, expected (%d, D)" % (tuple(waypoints.shape), rows))
        D = int(waypoints.shape[1])
        point_offsets = np.zeros(B + 1, dtype=np.int32)
        xp = _backend(waypoints)
        w = xp.array(waypoints, xp.float64, (rows, D), "waypoints")
        r = None
        if rounding is not None:      # on the device a 0-d tensor counts as one number here
            r = xp.per(rounding if xp.host or (hasattr(rounding, "shape") and len(rounding.shape)) else
                       float(rounding), B, "rounding")
        out = dict(knots=xp.zeros(K), control_points=xp.zeros((P, D)), num_points=xp.zeros(B, xp.int32),
                   path_end=xp.zeros(B), status=xp.full(B, -1, xp.int32))
        self._call("tpamd_fit_joint_waypoints", B, D, off, w, r, out["knots"], out["control_points"],
                   out["num_points"], point_offsets, out["path_end"], out["status"], host=xp.host, stream=stream)
        out["point_offsets"] = point_offsets
        return out

    def _waypoint_io(self, waypoints, offsets, max_velocity, max_acceleration, num_samples, num_samples_per_path,
                     delta, rounding, sd_start, time_start, safety, outputs, host):
        """The C structs of one waypoint timing call (plain or refined), the dict it returns, the
        device of the arrays (None with host=True) and what must stay alive until the call is made."""
        off, B = _waypoint_offsets(offsets)
        N, D = int(num_samples), int(max_velocity.shape[-1])
        out = dict(outputs) if outputs else {}
        xp = _NUMPY if host else _Torch(max_velocity.device)
        f = lambda x, shape, what, dt=xp.float64: xp.array(x, dt, shape, what)
        new, i32, dev = xp.zeros, xp.int32, xp.device
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
        po, fo = _PathOutputs.from_dict(out), _WaypointFitOutputs.from_dict(out)
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
        self._call("tpamd_time_waypoint_paths", bt, wi, po, fo, host=host, stream=stream, keep=keep)
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
        xp = _NUMPY if host else _Torch(device)
        new = lambda shape, real=True: xp.zeros(shape, xp.float64 if real else xp.int32)
        src = refined or {}
        out = {k: v for k, v in src.items() if k not in ("check", "refined", "refined_check")}
        for name, n in (("check", B), ("refined_check", M)):
            rec = dict(src.get(name) or {})
            for k in _CheckOutputs._keys_:
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
        ro.check = _CheckOutputs.from_dict(out["check"])
        for k in ("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta"):
            setattr(ro, k, _ptr(out.get(k)))
        ro.refined = _PathOutputs.from_dict(sol)
        ro.refined_check = _CheckOutputs.from_dict(out["refined_check"])
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
        ji, po = _JointInputs.from_dict(inputs), _PathOutputs.from_dict(outputs)
        opt, ro, out = self._refine_io(B, D, max_rounds, max_samples, max_refined, tolerance, refined,
                                       None if host else cp.device, host)
        self._call("tpamd_time_joint_paths_refined", bt, ji, po, opt, ro, host=host, stream=stream)
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
        self._call("tpamd_time_waypoint_paths_refined", bt, wi, po, fo, opt, ro, host=host, stream=stream, keep=keep)
        return out, ref

    # ------------------------------------------- checking solutions against their rows
    def _check_io(self, solution, outputs, B, like, host):
        """The tpamd_solution / tpamd_check_outputs of one check call and the dict it returns: the
        arrays of `outputs` where it has them, new ones (on the device of `like`, or numpy arrays
        with host=True) otherwise."""
        out = dict(outputs) if outputs else {}
        xp = _NUMPY if host else _Torch(like.device)
        for k in _CheckOutputs._keys_:
            if k not in out:
                out[k] = xp.zeros(B, xp.float64 if k == "worst_excess" else xp.int32)
        return _Solution.from_dict(solution), _CheckOutputs.from_dict(out), out

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
        ri = _RowsInputs.from_dict(inputs)
        ns = None if num_samples_per_path is None else _int32_array(num_samples_per_path, B, "num_samples_per_path")
        sol, cko, out = self._check_io(solution, outputs, B, a, host)
        self._call("tpamd_check_rows", bt, ri, ns, sol, cko, host=host, stream=stream)
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
        ji = _JointInputs.from_dict(inputs)
        npp = None if num_points_per_path is None else _int32_array(num_points_per_path, B, "num_points_per_path")
        sol, cko, out = self._check_io(solution, outputs, B, cp, host)
        self._call("tpamd_check_joint_paths", bt, ji, npp, sol, cko, host=host, stream=stream)
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
        if not host:      # the zeros are this method's own: they live as long as the call's other arguments
            self._keepalive["tpamd_check_joint_paths_device"] += (zero,)
        return out

    def check_cartesian_paths(self, inputs, solution, safety=0.8, num_samples_per_path=None, first_row=None,
                              outputs=None, stream=None, host=False):
        """The same for a Cartesian batch (tpamd_check_cartesian_paths_*): inputs, num_samples_per_path
        and first_row as time_cartesian_paths took them. With first_row the inputs are packed row
        tables, and B and the stride N are those of solution["sdd"] [B][N]."""
        ik = inputs["ik_positions"]
        B, N, D = self._cartesian_shape(inputs, first_row, solution["sdd"] if first_row is not None else None)
        ns = None if num_samples_per_path is None else _int32_array(num_samples_per_path, B, "num_samples_per_path")
        fr = None if first_row is None else _int32_array(first_row, B, "first_row")
        bt = _CartesianBatch(B, D, N, 0, float(safety))
        ci = _CartesianInputs.from_dict(inputs)
        sol, cko, out = self._check_io(solution, outputs, B, ik, host)
        rows = (int(ik.shape[0]) if fr is not None else 0,) if host else ()      # as time_cartesian_paths
        self._call("tpamd_check_cartesian_paths", bt, ci, ns, fr, *rows, sol, cko, host=host, stream=stream)
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
        xp = _backend(position)
        pos = xp.array(position, xp.float64, what="position")
        if pos.ndim != 2:
            raise TpamdError("position has shape %s, expected (count, D)" % (tuple(pos.shape),))
        n, D = pos.shape
        vel = xp.array(velocity, xp.float64, (n, D), "velocity")
        acc = xp.array(acceleration_limit, xp.float64, (n, D), "acceleration_limit")
        rnd = xp.per(corner_rounding, n, "corner_rounding")
        point, status = xp.full((n, D), float("nan")), xp.full(n, -1, xp.int32)
        self._call("tpamd_compute_stopping_points", n, D, pos, vel, acc, rnd, point, status, host=xp.host,
                   stream=stream)
        return point, status

    def project_points_on_paths(self, waypoints, offsets, point, stream=None):
        """ProjectPointOnPath for a ragged batch (tpamd_project_points_on_paths_*): list k is
        waypoints[offsets[k]:offsets[k + 1]] ([rows][D] float64), point [count][D]. Returns a dict:
        waypoint_index, status [count] int32, distance_to_path, line_parameter [count] and
        projected_point [count][D]; an empty list has status INVALID_ARGUMENT and NaN / -1 outputs.
        offsets is a host array in both forms. CUDA waypoints go through the _device entry on
        `stream`, which only enqueues, and give CUDA tensors; anything else goes through the host
        entry, which synchronises, and gives numpy arrays."""
        off, n = _waypoint_offsets(offsets)
        xp, nan = _backend(point), float("nan")
        pt = xp.array(point, xp.float64, what="point")
        if pt.ndim != 2 or pt.shape[0] != n:
            raise TpamdError("point has shape %s, expected (%d, D)" % (tuple(pt.shape), n))
        D = pt.shape[1]
        if xp.host:      # any shape that holds rows of D
            w = xp.array(waypoints, xp.float64, what="waypoints").reshape(-1, D)
            if w.shape[0] != off[-1]:
                raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        else:
            w = xp.array(waypoints, xp.float64, (int(off[-1]), D), "waypoints")
        out = dict(waypoint_index=xp.full(n, -1, xp.int32), distance_to_path=xp.full(n, nan),
                   line_parameter=xp.full(n, nan), projected_point=xp.full((n, D), nan),
                   status=xp.full(n, -1, xp.int32))
        self._call("tpamd_project_points_on_paths", n, D, off, w if w.shape[0] * D else None, pt, out["waypoint_index"],
                   out["distance_to_path"], out["line_parameter"], out["projected_point"], out["status"],
                   host=xp.host, stream=stream)
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
        xp = _backend(jc)
        dl = xp.per(delta, B, "delta")
        pose, joint = xp.zeros((rows, 7)), xp.zeros((rows, D))
        splines = [xp.array(fit[k], xp.float64, what=k) for k in (
            "knots", "translation_points", "rotation_points", "joint_control_points")]
        if fr is not None:
            self._call("tpamd_sample_ik_target_rows", B, D, npts, off, fr, *splines, dl, pose, joint, host=xp.host,
                       stream=stream)
        else:
            self._call("tpamd_sample_ik_targets", B, D, npts, off, *splines, dl, pose, joint, host=xp.host,
                       stream=stream)
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
        self._call("tpamd_find_max_sd2_host", num, Cn, a, b, lower, upper, *o)
        return tuple(o)

    def query(self, time, s, sd, status, t_query, out_s, out_sd, out_sdd, ok=None, stream=None,
              sd2=None):
        """sd2: the solve's squared velocities (outputs["sd2"]); None = the engine's copy from
        its last solve (TpamdError "stale" if time is not that solve's output)."""
        B, N = time.shape
        K = t_query.shape[1]
        self._call("tpamd_query", B, N, K, time, s, sd, sd2, status, t_query, out_s, out_sd, out_sdd, ok,
                   host=False, stream=stream)

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
        self._call("tpamd_resample_skip" if skip else "tpamd_resample_uniform", args, host=False, stream=stream)

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
            time, s, qd, qdd, max_acceleration, query_time = (
                _cpu_array(x, np.float64) for x in (time, s, qd, qdd, max_acceleration, query_time))
            count = _cpu_array(count, np.int32)
        xp = _NUMPY if host else _Torch(qd.device)
        new, f64, i32 = xp.zeros, xp.float64, xp.int32
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
        self._call("tpamd_fastest_stop", args, host=host, stream=stream)
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
            time, qd, qdd, max_acceleration, stop_time = (
                _cpu_array(x, np.float64) for x in (time, qd, qdd, max_acceleration, stop_time))
            count, stop_index = _cpu_array(count, np.int32), _cpu_array(stop_index, np.int32)
        xp = _NUMPY if host else _Torch(qd.device)
        new, f64, i32 = xp.zeros, xp.float64, xp.int32
        res = {k: new((B,), i32) for k in ("status", "keep", "first", "last")}
        for k, shape in (("out_time", (B, M)), ("out_qd", (B, M, D)), ("out_qdd", (B, M, D))):
            res[k] = out[k] if out is not None else new(shape, f64)
            if tuple(res[k].shape) != shape:
                raise TpamdError("%s has shape %s, expected %s" % (k, tuple(res[k].shape), shape))
        args = _StopTrajectoryArgs(
            B, M, D, 0, _ptr(time), _ptr(qd), _ptr(qdd), _ptr(count), _ptr(max_acceleration), float(time_step),
            _ptr(stop_time), _ptr(stop_index),
            *[_ptr(res[k]) for k in ("status", "keep", "first", "last", "out_time", "out_qd", "out_qdd")])
        self._call("tpamd_stop_trajectories", args, host=host, stream=stream)
        return res

    def debug_boundary(self, B, N):
        arr = {k: np.zeros((B, N)) for k in ("sd2_max", "sdd_max", "sdd_min", "sd2_zero", "sd2")}
        arr["type"] = np.zeros((B, N), dtype=np.uint8)
        self._call("tpamd_debug_copy_boundary", B, N, arr["sd2_max"], arr["sdd_max"], arr["sdd_min"],
                   arr["sd2_zero"], arr["type"], arr["sd2"])
        return arr

    def debug_keep_boundary(self, on=True):
        """Have the fused joint sweep store sdd_max/sdd_min/type for debug_boundary()."""
        self._lib.tpamd_debug_keep_boundary(self._h, 1 if on else 0)

    def rebuild_time(self, sd, ds, time_start, out, num_shards, paths_per_shard, num_samples,
                     shard_stride, num_samples_per_path=None, stream=None):
        """time [num_shards * paths_per_shard][N] from sd (tpamd_rebuild_time_device). sd, ds and
        time_start are tensors (views) that start at shard 0's data; shard r lies shard_stride
        doubles further."""
        self._call("tpamd_rebuild_time", num_shards, paths_per_shard, num_samples, shard_stride, sd, ds,
                   time_start, num_samples_per_path, out, host=False, stream=stream)

    def debug_kernel_vgprs(self, which):
        """Registers per lane of the 7-joint sampling/LP kernel (0) / sweep kernel (1)."""
        n = self._lib.tpamd_debug_kernel_vgprs(self._h, which)
        _check(min(n, 0), "tpamd_debug_kernel_vgprs")
        return n

    def debug_diag(self, B):
        out = np.zeros((B, 64), dtype=np.int64)
        self._call("tpamd_debug_copy_diag", B, out)
        return out

    def debug_diag_ext(self, B):
        out = np.zeros((B, 32), dtype=np.int64)
        self._call("tpamd_debug_copy_diag_ext", B, out)
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


class PlannerSet(_Native):
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

    _kind, _destroy, _host_suffix = "planner set", "tpamd_planner_set_destroy", ""

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
        self._adopt(h)
        self._num_samples = np.zeros(self.B, dtype=np.int64)    # GetNumTimeSamples after the last plan
        self._pending = None           # the PlanHandle of a plan_async whose result() has not run yet
        self._imports = []             # device imports whose summaries have not been read yet

    def _release(self):
        if getattr(self, "_pending", None) is not None:
            self._pending._stream.synchronize()      # the call writes the handle's tensors
            self._pending = None

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
        off, ida, n = self._offsets(offsets, ids, "waypoint offsets")
        D = self.D
        xp = _backend(waypoints, as_torch=True)
        # (the device side takes an empty tensor of any shape, and no rows at all when nobody is listed)
        w = xp.array(waypoints, xp.float64, what="waypoints").reshape(-1, D) if xp.host or waypoints.numel() else \
            xp.zeros((0, D))
        if (xp.host or n) and w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        vm = xp.array(max_velocity, xp.float64, (n, D), "max_velocity")
        am = xp.array(max_acceleration, xp.float64, (n, D), "max_acceleration")
        dl = xp.per(delta, n, "delta")
        iv = xp.array(initial_velocity, xp.float64, (n, D), "initial_velocity")
        status, num_points = xp.full(n, -1, xp.int32), xp.zeros(n, xp.int32)
        self._call("tpamd_planner_set_set_waypoints", n, ida, off, w if w.shape[0] else None, float(rounding), vm, am,
                   dl, iv, num_points, status, host=xp.host, stream=stream)
        return xp.result(status), xp.result(num_points)

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
        off, ida, n = self._offsets(offsets, ids, "waypoint offsets")
        D, nan = self.D, float("nan")
        xp = _backend(waypoints if _is_cuda(waypoints) or int(off[-1]) else time_ns, as_torch=True)
        # (without waypoints the device side does not look at `waypoints`)
        w = xp.array(waypoints, xp.float64, what="waypoints").reshape(-1, D) if xp.host or int(off[-1]) else \
            xp.zeros((0, D))
        if w.shape[0] != off[-1]:
            raise TpamdError("waypoints has %d rows, offsets end at %d" % (w.shape[0], off[-1]))
        t = xp.array(time_ns, xp.int64, (n,), "time_ns")
        vm = xp.array(max_velocity, xp.float64, (n, D), "max_velocity")
        am = xp.array(max_acceleration, xp.float64, (n, D), "max_acceleration")
        dl = xp.per(delta, n, "delta")
        sa = xp.array(stopping_acceleration, xp.float64, (n, D), "stopping_acceleration")
        out = dict(status=xp.full(n, -1, xp.int32), num_points=xp.zeros(n, xp.int32), position=xp.full((n, D), nan),
                   velocity=xp.full((n, D), nan), stopping_point=xp.full((n, D), nan))
        self._call("tpamd_planner_set_retarget", n, ida, t, off, w if w.shape[0] else None, float(rounding), vm, am,
                   dl, sa, out["num_points"], out["status"], out["position"], out["velocity"], out["stopping_point"],
                   host=xp.host, stream=stream)
        return {k: xp.result(v) for k, v in out.items()}

    def _offsets(self, offsets, ids, what, dtype=np.int32):
        """Host offsets [count + 1] (`what` names them in errors) with the listed ids and their count."""
        off = _host(offsets, dtype, what=what).reshape(-1)
        ida, n = self._ids(ids, off.shape[0] - 1)
        if off.shape[0] != n + 1:
            raise TpamdError("%s need count + 1 = %d entries, got %d" % (what, n + 1, off.shape[0]))
        return off, ida, n

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
        self._call("tpamd_planner_set_upload_paths_ragged", n, ida, npts, k, c, vm, am, dl, iv, ps)

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
        off, ida, n = self._offsets(row_offsets, ids, "row offsets")
        D = self.D
        rows = int(off[-1]) if n else 0
        xp = _backend(ik_positions)
        q = xp.array(ik_positions, xp.float64, (rows, D), "ik_positions")
        J = xp.array(jacobians, xp.float64, (rows, 6, D), "jacobians")
        pe, vt, vr, dl = (xp.per(path_end, n, "path_end"),
                          xp.per(max_translational_velocity, n, "max_translational_velocity"),
                          xp.per(max_rotational_velocity, n, "max_rotational_velocity"), xp.per(delta, n, "delta"))
        vm = xp.array(max_velocity, xp.float64, (n, D), "max_velocity")
        am = xp.array(max_acceleration, xp.float64, (n, D), "max_acceleration")
        iv = xp.array(initial_velocity, xp.float64, (n, D), "initial_velocity")
        ps = xp.full(n, 1, xp.int32) if path_state is None else xp.array(path_state, xp.int32, (n,), "path_state")
        self._call("tpamd_planner_set_upload_ik_tables", n, ida, off, q, J, pe, vm, am, vt, vr, dl, iv, ps,
                   host=xp.host, stream=stream)

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
        off, ida, n = self._offsets(offsets, ids, "waypoint offsets")
        D = self.D
        dev = pose_waypoints.device if _is_cuda(pose_waypoints) else torch.device("cuda", self.device)
        xp = _Torch(dev)
        f = lambda x, shape, what: xp.array(x, xp.float64, shape, what)
        per = lambda x, what: xp.per(x, n, what)
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
        self._call("tpamd_planner_set_download_ik_table", int(planner), C.byref(R), None, None, 0)
        q, J = np.zeros((R.value, self.D)), np.zeros((R.value, 6, self.D))
        if R.value:
            self._call("tpamd_planner_set_download_ik_table", int(planner), C.byref(R), q, J, R.value)
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
        self._call("tpamd_planner_set_discard_ik_rows", n, ida, keep, out)
        return out

    def ik_table_info(self, planner):
        """Host bookkeeping of one planner's IK table (tpamd_planner_set_ik_table_info):
        (first_row, rows, capacity): the path row in slot 0, the path rows supplied so far (0: no
        table) and the table rows allocated per planner."""
        f, r, c = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._call("tpamd_planner_set_ik_table_info", int(planner), C.byref(f), C.byref(r), C.byref(c))
        return int(f.value), int(r.value), int(c.value)

    def download_ik_rows(self, planner):
        """The live rows of one planner's IK table (tpamd_planner_set_download_ik_rows):
        (first_row, ik_positions [live][D], jacobians [live][6][D]) numpy, path rows first_row ..
        first_row + live - 1."""
        f, R = C.c_int32(0), C.c_int32(0)
        self._call("tpamd_planner_set_download_ik_rows", int(planner), C.byref(f), C.byref(R), None, None, 0)
        q, J = np.zeros((R.value, self.D)), np.zeros((R.value, 6, self.D))
        if R.value:
            self._call("tpamd_planner_set_download_ik_rows", int(planner), C.byref(f), C.byref(R), q, J, R.value)
        return int(f.value), q, J

    def download_path(self, planner):
        """The resident spline of one planner: (knots [P + 3], control_points [P][D]) numpy; P = 0:
        no path."""
        P = C.c_int32(0)
        self._call("tpamd_planner_set_download_path", int(planner), C.byref(P), None, None, 0)
        k, c = np.zeros(P.value + 3 if P.value else 0), np.zeros((P.value, self.D))
        if P.value:
            self._call("tpamd_planner_set_download_path", int(planner), C.byref(P), k, c, P.value)
        return k, c

    def reset(self, ids=None):
        """TrajectoryPlanner::Reset for the listed planners (None: all)."""
        ida, n = self._ids(ids)
        self._call("tpamd_planner_set_reset", n, ida)
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
        self._call("tpamd_planner_set_plan", s, h, out)
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
        self._call("tpamd_planner_set_reserve", int(history), int(trajectory))

    def capacity(self):
        """(history, trajectory) samples per planner the buffers hold."""
        h, t = C.c_int32(0), C.c_int32(0)
        self._call("tpamd_planner_set_capacity", C.byref(h), C.byref(t))
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
        self._call("tpamd_planner_set_plan", start_ns, horizon_ns, int(max_windows), summary, info, host=False,
                   stream=st)
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
        off, ida, n = self._offsets(row_offsets, ids, "row offsets")
        rows, D = (int(off[-1]) if n else 0), self.D
        xp = _backend(ik_positions)
        q = xp.array(ik_positions, xp.float64, (rows, D), "ik_positions")
        J = xp.array(jacobians, xp.float64, (rows, 6, D), "jacobians")
        self._call("tpamd_planner_set_append_ik_rows", n, ida, off, q, J, host=xp.host, stream=stream)

    def _plan_streaming(self, start_ns, horizon_ns):
        s = _host(np.broadcast_to(_host(start_ns, np.int64), (self.B,)), np.int64)
        h = _host(np.broadcast_to(_host(horizon_ns, np.int64), (self.B,)), np.int64)
        out = np.zeros(self.B, dtype=PLANNER_SUMMARY_DTYPE)
        need = np.zeros((2, self.B), dtype=np.int32)
        self._call("tpamd_planner_set_plan_streaming", s, h, out, need[0], need[1], None)
        return self._summary(out), need[0], need[1]

    def plan_resume(self):
        """tpamd_planner_set_plan_resume: the planners that wait for rows re-enter the window loop.
        Returns (summary dict as plan(), need_first [B], need_count [B] int32 numpy)."""
        out = np.zeros(self.B, dtype=PLANNER_SUMMARY_DTYPE)
        need = np.zeros((2, self.B), dtype=np.int32)
        self._call("tpamd_planner_set_plan_resume", out, need[0], need[1], None)
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
        self._call("tpamd_planner_set_stop_parameters", n, ida, t, s, dur, st)
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
        self._call("tpamd_planner_set_switch_paths_rounded", n, ida, t, keep, off, w, float(rounding), s, npts, st)
        return dict(stop_parameter=torch.from_numpy(s), num_points=torch.from_numpy(npts), status=torch.from_numpy(st))

    # ------------------------------------------------------------ checking the windows
    def set_checking(self, on=True):
        """Check every window the Plan calls solve against its constraint rows
        (tpamd_planner_set_set_checking; off by default)."""
        self._call("tpamd_planner_set_set_checking", 1 if on else 0)

    @property
    def checking(self):
        return bool(self._lib.tpamd_planner_set_checking(self._handle()))

    def check_results(self, ids=None):
        """The tpamd_planner_check record of each listed planner (all without ids) over the windows
        of its last Plan call: a numpy structured array of PLANNER_CHECK_DTYPE. Synchronises."""
        ida, n = self._ids(ids)
        out = np.zeros(max(n, 1), dtype=PLANNER_CHECK_DTYPE)
        self._call("tpamd_planner_set_check_results", n, ida, out)
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
        idt = self._device().array(ids, torch.int32, (n,), "ids")
        self._call("tpamd_planner_set_check_results", n, idt, out, host=False, stream=stream)
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
            xp = self._device()
            dev = xp.device
            st0 = xp.array(start_ns, torch.int64, what="start_ns").reshape(-1)
            n = st0.shape[0]
            idt = xp.array(ids, torch.int32, (n,), "ids")
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
            self._call("tpamd_planner_set_sample_at_ticks", n, idt, st0, int(step_ns), T, q, qd, qdd, status,
                       host=False, stream=stream)
            return dict(q=q, qd=qd, qdd=qdd, status=status)
        st0 = _host(start_ns, np.int64).reshape(-1)
        ida, n = self._ids(ids, st0.shape[0])
        if st0.shape[0] != n:
            raise TpamdError("one start time per listed planner")
        out = {k: np.full((n, T, self.D), np.nan) for k in ("q", "qd", "qdd")}
        out["status"] = np.full((n, T), -1, dtype=np.int32)
        self._call("tpamd_planner_set_sample_at_ticks", n, ida, st0, int(step_ns), T, out["q"], out["qd"], out["qdd"],
                   out["status"])
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
        self._call("tpamd_planner_set_download_trajectories", n, idt, out["offsets"], rows,
                   *[out[k] if rows else None for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd")],
                   host=False, stream=stream)
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
        xp = self._device()
        dev = xp.device
        t = xp.array(time_ns, torch.int64, what="time_ns").reshape(-1)
        n = t.shape[0]
        idt = xp.array(ids, torch.int32, (n,), "ids")
        if ids is None and n > self.B:
            raise TpamdError("more stop times than planners")
        am = xp.array(max_acceleration, torch.float64, (n, self.D), "max_acceleration")
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
            self._call("tpamd_planner_set_stop_trajectories", n, idt, t, am, float(time_step), out["status"],
                       out["keep"], out["offsets"], int(capacity),
                       *[out[k] if capacity else None for k in ("time", "q", "qd", "qdd")], host=False, stream=stream)
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
        self._call("tpamd_planner_set_state_info", n, ida, out)
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
        self._call("tpamd_planner_set_export_state", n, idt, out, offt, status, host=False, stream=st)
        self.last_export_status = status
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
        off, ida, n = self._offsets(offsets, ids, "offsets", np.int64)
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
            self._call("tpamd_planner_set_import_state", n, idt, blob, offt, summary, status, host=False, stream=st)
            self._imports.append((st, summary, status, np.arange(n) if ida is None else ida.astype(np.int64)))
            return dict(status=status, summary=summary, _keep=(idt, offt, blob))
        b = _host(blob, np.uint8, what="blob").reshape(-1)
        if b.shape[0] < total:
            raise TpamdError("blob has %d bytes, offsets end at %d" % (b.shape[0], total))
        status = np.full(n, -1, dtype=np.int32)
        out = np.zeros(max(n, 1), dtype=PLANNER_SUMMARY_DTYPE)
        self._call("tpamd_planner_set_import_state_host", n, ida, b, off, out, status)
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
        self._call("tpamd_planner_set_copy_planners", dst, other._handle(), src, n, out, status)
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


class BufferSet(_Native):
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

    _kind, _destroy, _host_suffix = "buffer set", "tpamd_buffer_set_destroy", ""

    def __init__(self, engine, num_buffers, num_dofs, capacity=0, timestep_tolerance=1e-6):
        self._lib = load_library()
        self.B, self.D = int(num_buffers), int(num_dofs)
        self.device = engine.device
        h = C.c_void_p()
        _check(self._lib.tpamd_buffer_set_create(engine._h, self.B, self.D, int(capacity), float(timestep_tolerance),
                                                 C.byref(h)), "tpamd_buffer_set_create")
        self._engine = engine          # the set must not outlive its engine
        self._adopt(h)

    @property
    def device_bytes(self):
        return self._lib.tpamd_buffer_set_device_bytes(self._handle())

    @property
    def capacity(self):
        return self._lib.tpamd_buffer_set_capacity(self._handle())

    def reserve(self, capacity):
        """Room for `capacity` samples per buffer (synchronises; the other calls never allocate)."""
        self._call("tpamd_buffer_set_reserve", int(capacity))

    def _dev(self):
        return self._device().device

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
        self._call("tpamd_buffer_set_insert", n, idt, off, rows, *[a if rows else None for a in [tm] + arr], st,
                   host=False, stream=stream)
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
        self._call("tpamd_buffer_set_insert_from_planner_set", planner_set._handle(), n, idt, pid, st, host=False,
                   stream=stream)
        return dict(status=st, _keep=(idt, pid))

    def append_sample(self, time, q, qd, qdd, ids=None, stream=None):
        """AppendSample: time [count], q, qd, qdd [count][D]. Returns dict status."""
        import torch
        tm = self._t(time, torch.float64, None, "time").reshape(-1)
        idt, n = self._list(ids, tm.shape[0])
        arr = [self._t(a, torch.float64, (n, self.D), k) for k, a in (("q", q), ("qd", qd), ("qdd", qdd))]
        st = self._status(n)
        self._call("tpamd_buffer_set_append_sample", n, idt, tm, *arr, st, host=False, stream=stream)
        return dict(status=st, _keep=(idt, tm, arr))

    def discard_before(self, time_ns=None, time_sec=None, ids=None, stream=None):
        """DiscardSegmentBefore at time_ns [count] (int64) or time_sec [count]. Returns dict status."""
        tn, ts, n = self._times(time_ns, time_sec)
        idt, n = self._list(ids, n)
        st = self._status(n)
        self._call("tpamd_buffer_set_discard_before", n, idt, tn, ts, st, host=False, stream=stream)
        return dict(status=st, _keep=(idt, tn, ts))

    def stop_before_time(self, max_acceleration, time_step, time_ns=None, time_sec=None, ids=None, stream=None):
        """StopBeforeTime in place: max_acceleration [count][D]. Returns dict status."""
        import torch
        tn, ts, n = self._times(time_ns, time_sec)
        idt, n = self._list(ids, n)
        am = self._t(max_acceleration, torch.float64, (n, self.D), "max_acceleration")
        st = self._status(n)
        self._call("tpamd_buffer_set_stop_before_time", n, idt, tn, ts, am, float(time_step), st, host=False,
                   stream=stream)
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
        self._call("tpamd_buffer_set_sample_at_ticks", n, idt, s0, int(step_ns), T, out["q"], out["qd"], out["qdd"],
                   out["status"], host=False, stream=stream)
        out["_keep"] = (idt, s0)
        return out

    def add_offset(self, offset_ns=None, offset_sec=None, ids=None, stream=None):
        """AddOffsetToTimestamps: offset_sec [count], or offset_ns [count] (a duration)."""
        tn, ts, n = self._times(offset_ns, offset_sec)
        idt, n = self._list(ids, n)
        st = self._status(n)
        self._call("tpamd_buffer_set_add_offset", n, idt, tn, ts, st, host=False, stream=stream)
        return dict(status=st, _keep=(idt, tn, ts))

    def clear(self, ids=None, stream=None):
        idt, n = self._list(ids, None)
        st = self._status(n)
        self._call("tpamd_buffer_set_clear", n, idt, st, host=False, stream=stream)
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
        self._call("tpamd_buffer_set_info", n, idt, tn, out["num_samples"], out["sequence"], out["start_ns"],
                   out["end_ns"], out.get("positions_up_to"), host=False, stream=stream)
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
        self._call("tpamd_buffer_set_download", n, idt, out["offsets"], rows,
                   *[out[k] if rows else None for k in ("time", "q", "qd", "qdd")], host=False, stream=stream)
        total = int(out["offsets"][-1].item())
        if total > rows:
            raise TpamdError("the buffers hold %d rows, capacity %d" % (total, rows))
        for k in ("time", "q", "qd", "qdd"):
            out[k] = out[k][:total]
        out["_keep"] = (idt,)
        return out


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

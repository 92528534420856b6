"""Seeded pose-waypoint cases and a long-double restatement of the Cartesian waypoint fit (test helper).

The restatement follows the reference's definitions, not the code under test:
PolyLineToBspline3Waypoints / CornerOffset on poses (splines/spline_utils.cc:104-204) with the textbook
Pose3d algebra (a * b = (qa qb, ta + qa tb qa^-1), a^-1 = (qa^-1, -qa^-1 ta qa), q^-1 = conj(q) / |q|^2),
Eigen's quaternion -> angle-axis rule (angle = 2 atan2(|v|, |w|), axis = v / (+-|v|) with the sign of w;
|v| = 0: angle 0 about x), the vector corner rounding for the joint polygon (spline_utils.cc:47-102),
uniform clamped degree-2 knots on [0, 1], and the knot scale max(L + L, 0.1) * 10 of
TimeableCartesianSplinePath::FitSplineToWaypoints (timeable_path_cartesian_spline.cc:415-482), L the
length of the translation control polygon. Everything is numpy.longdouble (64-bit mantissa on x86).

Case families (pose waypoints [W][7] = translation, quaternion w x y z; joint waypoints [W][D]):
  random                random unit rotations, translations in [-1, 1]^3
  identical             neighbouring rotations identical (relative rotation 1: |v| = 0 or rounding dust)
  tiny                  neighbours 1e-13 rad apart
  near_pi               relative rotations of pi -/+ 1e-6 (w of the relative rotation on either side of 0)
  antipodal             neighbours q, -q
  repeated_translation  neighbouring translations identical (translation norm exactly 0)
  short                 a polygon short enough that the final knot is the floor 0.1 * 10
"""
import struct

import numpy as np

LD = np.longdouble
FAMILIES = ("random", "identical", "tiny", "near_pi", "antipodal", "repeated_translation", "short")
ROUNDINGS = ((0.1, 0.2), (1e-3, 0.5), (5.0, 5.0), (0.0, 0.2))      # (translation, rotation)
DOFS = (1, 6, 7, 16)
BOUND = 4e-15                     # tests/test_gpu_cartesian_hp.py QUAT_TOL: the bound for this libm chain


# ------------------------------------------------------------------ cases
def _qmul_d(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])


def _unit(v):
    return v / np.linalg.norm(v)


def _qaxis(angle, axis):
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * axis])


def make_case(family, W, D, rng):
    """(pose_waypoints [W][7], joint_waypoints [W][D]) of one family."""
    t = rng.uniform(-1.0, 1.0, (W, 3))
    q = np.array([_unit(rng.standard_normal(4)) for _ in range(W)]).reshape(W, 4)
    for i in range(1, W):
        ax = _unit(rng.standard_normal(3))
        if family == "identical":
            q[i] = q[i - 1]
        elif family == "tiny":
            q[i] = _unit(_qmul_d(q[i - 1], _qaxis(1e-13, ax)))
        elif family == "near_pi":
            q[i] = _unit(_qmul_d(q[i - 1], _qaxis(np.pi - (1e-6 if i % 2 else -1e-6), ax)))
        elif family == "antipodal":
            q[i] = -q[i - 1]
        elif family == "repeated_translation" and (i % 2 or W == 2):
            t[i] = t[i - 1]
    if family == "short":
        t = t[:1] + 0.004 * (t - t[:1]) / max(W, 1)        # 2 L < 0.1 however the corners are rounded
    joints = rng.uniform(-2.5, 2.5, (W, D))
    return np.ascontiguousarray(np.hstack([t, q])), np.ascontiguousarray(joints)


def all_cases(seeds=5):
    """The CPU case list: every family x W 1..6 x D x rounding pair x `seeds` seeds (3 360 cases at 5
    seeds, 480 per family), then four paths without waypoints. Entries are dicts."""
    out = []
    rng = np.random.default_rng(20261018)
    for fam in FAMILIES:
        for W in range(1, 7):
            for D in DOFS:
                for tr, rr in ROUNDINGS:
                    for _ in range(seeds):
                        pose, joints = make_case(fam, W, D, rng)
                        out.append(dict(family=fam, W=W, D=D, tr=tr, rr=rr, pose=pose, joints=joints))
    for D in DOFS:
        out.append(dict(family="empty", W=0, D=D, tr=0.1, rr=0.2, pose=np.zeros((0, 7)), joints=np.zeros((0, D))))
    return out


def write_cases(path, cases):
    """Binary case file for tests/cpp/test_pose_fit.cc: int32 count, then per case int32 W, D, family
    index, 0; double translation rounding, rotation rounding; pose waypoints; joint waypoints."""
    names = FAMILIES + ("empty", "golden")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(cases)))
        for c in cases:
            f.write(struct.pack("<iiii", c["W"], c["D"], names.index(c["family"]), 0))
            f.write(struct.pack("<dd", c["tr"], c["rr"]))
            f.write(np.ascontiguousarray(c["pose"], dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(c["joints"], dtype="<f8").tobytes())


def read_fits(path, cases):
    """The driver's dump: per case int32 P, then knots [P + 3], translation [P][3], rotation [P][4],
    joint control points [P][D] of fit_pose_waypoints."""
    raw = open(path, "rb").read()
    pos, out = 0, []
    for c in cases:
        P = struct.unpack_from("<i", raw, pos)[0]
        pos += 4
        take = lambda n: np.frombuffer(raw, dtype="<f8", count=n, offset=pos)
        k = take(P + 3 if P else 0)
        pos += 8 * k.size
        t = take(3 * P).reshape(P, 3)
        pos += 24 * P
        r = take(4 * P).reshape(P, 4)
        pos += 32 * P
        j = take(P * c["D"]).reshape(P, c["D"])
        pos += 8 * P * c["D"]
        out.append(dict(P=P, knots=k, translation=t, rotation=r, joints=j))
    assert pos == len(raw)
    return out


# ------------------------------------------------------------------ the long-double reference
def _qmul(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=LD)


def _qinv(q):
    n2 = np.sum(q * q)
    if not n2 > 0:
        return np.zeros(4, dtype=LD)
    return q * np.array([1, -1, -1, -1], dtype=LD) / n2


def _rotate(q, v):
    """q v q^-1 for any q as Eigen defines q * v: v + 2 w (u x v) + 2 u x (u x v)."""
    u = q[1:]
    uv = np.cross(u, v)
    return v + LD(2) * q[0] * uv + LD(2) * np.cross(u, uv)


def _pose_mul(a, b):
    return (a[0] + _rotate(a[1], b[0]), _qmul(a[1], b[1]))


def _pose_inv(a):
    qi = _qinv(a[1])
    return (-_rotate(qi, a[0]), qi)


def corner_offset(delta, translation_radius, rotation_radius):
    ident = (np.zeros(3, dtype=LD), np.array([1, 0, 0, 0], dtype=LD))
    if translation_radius < 1e-6 or rotation_radius < 1e-6:
        return ident
    t, q = delta
    tnorm = np.sqrt(np.sum(t * t))
    n = np.sqrt(np.sum(q[1:] ** 2))
    if n == 0:
        angle, axis = LD(0), np.array([1, 0, 0], dtype=LD)
    else:
        angle = LD(2) * np.arctan2(n, np.abs(q[0]))
        axis = q[1:] / (-n if q[0] < 0 else n)
    inf = LD(np.inf)
    pct = min(inf if tnorm == 0 else LD(translation_radius) / tnorm,
              inf if angle == 0 else LD(rotation_radius) / angle)
    pct = min(pct, LD(1) / LD(4))
    half = LD(0.5) * angle * pct
    return (t * pct, np.concatenate([[np.cos(half)], np.sin(half) * axis]).astype(LD))


def pose_control_points(pose, translation_radius, rotation_radius):
    """PolyLineToBspline3Waypoints on poses [W][7] -> (translation [P][3], rotation [P][4]) longdouble."""
    pose = np.asarray(pose, dtype=float)
    W = pose.shape[0]
    corners = [(pose[i, :3].astype(LD), pose[i, 3:].astype(LD)) for i in range(W)]
    if W == 1:
        out = [corners[0]] * 4
    else:
        out = [None] * (3 * W - 2)
        for i in range(W):
            out[3 * i] = corners[i]

        def inner(k, other):
            return _pose_mul(out[k], corner_offset(_pose_mul(_pose_inv(out[k]), out[other]), translation_radius,
                                                   rotation_radius))
        for i in range(1, W - 1):
            out[3 * i + 1] = inner(3 * i, 3 * i + 3)
            out[3 * i - 1] = inner(3 * i, 3 * i - 3)
        out[1] = inner(0, 3)
        out[-2] = inner(len(out) - 1, len(out) - 4)
    return np.array([p[0] for p in out], dtype=LD), np.array([p[1] for p in out], dtype=LD)


def joint_control_points(joints, radius):
    """The vector corner rounding (spline_utils.cc:47-102) in longdouble."""
    w = np.asarray(joints, dtype=float).astype(LD)
    W = w.shape[0]
    if W == 1:
        return np.repeat(w, 4, axis=0)
    out = np.zeros((3 * W - 2, w.shape[1]), dtype=LD)
    out[0::3] = w

    def offset(delta):
        n = np.sqrt(np.sum(delta * delta))
        if not n > 1e-6:                            # kMinNorm
            return np.zeros_like(delta)
        return delta * min(LD(radius) / n, LD(1) / LD(4))
    for i in range(1, W - 1):
        k = 3 * i
        out[k + 1] = out[k] + offset(out[k + 3] - out[k])
        out[k - 1] = out[k] + offset(out[k - 3] - out[k])
    out[1] = out[0] + offset(out[3] - out[0])
    out[-2] = out[-1] + offset(out[-4] - out[-1])
    return out


def fit(pose, joints, translation_radius, rotation_radius):
    """The whole fit in longdouble: dict knots [P + 3], translation, rotation, joints."""
    t, r = pose_control_points(pose, translation_radius, rotation_radius)
    P = t.shape[0]
    inner = P - 2                                   # knot intervals of a clamped degree-2 spline
    knots = np.concatenate([[0, 0], np.arange(inner + 1, dtype=LD) / LD(inner), [1, 1]]).astype(LD)
    length = np.sum(np.sqrt(np.sum(np.diff(t, axis=0) ** 2, axis=1)))
    scale = max(length + length, LD(0.1)) * LD(10)
    return dict(knots=knots * scale, translation=t, rotation=r, joints=joint_control_points(joints, rotation_radius))


def deviation(got, ref):
    """max |got - ref| / max(1, |ref|) over an array pair (longdouble arithmetic)."""
    ref = np.asarray(ref, dtype=LD)
    if ref.size == 0:
        return 0.0
    return float(np.max(np.abs(np.asarray(got, dtype=float).astype(LD) - ref) / np.maximum(1, np.abs(ref))))


def gpu_batch():
    """The 12 ragged D = 7 paths of the GPU fit test: W = 1, 2, 3, 4, 6, 2, 3, 5, 1, 2, 3, 0 over every
    family (the last path has no waypoints), with per-path roundings over ROUNDINGS."""
    rng = np.random.default_rng(77)
    Ws = (1, 2, 3, 4, 6, 2, 3, 5, 1, 2, 3, 0)
    fams = FAMILIES + ("random", "near_pi", "tiny", "short", "empty")
    cases = []
    for k, (W, fam) in enumerate(zip(Ws, fams)):
        tr, rr = ROUNDINGS[k % 4]
        if W == 0:
            pose, joints = np.zeros((0, 7)), np.zeros((0, 7))
        else:
            pose, joints = make_case(fam, W, 7, rng)
        cases.append(dict(family=fam, W=W, D=7, tr=tr, rr=rr, pose=pose, joints=joints))
    return cases

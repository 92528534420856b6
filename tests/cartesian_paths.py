"""Seeded Cartesian-path families (test helper), the Cartesian counterpart of structured_paths.py.

A Cartesian batch is what a TimeableCartesianSplinePath holds after its IK callback ran: the IK
positions q [B][N][D] at s_i = path_start + i delta and the Jacobian at every sample
[B][N][6][D], plus joint and Cartesian velocity limits (synthetic.make_cartesian_batch's format).
`synthetic.make_cartesian_batch` draws smooth random paths whose Cartesian rows rarely bind alone
and never vanish. Each family below reaches one regime and says which one:

  straight_trans   q linear in s (q_i = q0 + c s_i), constant J; v_trans is half of what the joint
                   velocities allow and v_rot ten times: translation binds the cruise
  straight_rot     the same with the roles of v_trans and v_rot swapped: rotation binds
  straight_joint   the same with both Cartesian limits ten times what the joints allow: a joint
                   velocity limit binds
  straight_accel   every velocity limit 1000 times what the acceleration reaches over the move:
                   a triangle profile, bound by the acceleration limit alone
  zero_jacobian    a random curved path with J = 0: both Cartesian rows vanish (B = 0)
  singular         a random curved path whose J at one interior sample m has q'_m in its null
                   space (J_m <- J_m (I - q'_m q'_m^T / |q'_m|^2)): J q' = 0 there to rounding
  idle             a random curved path whose IK rows repeat over an interior stretch and over
                   the first samples: q' = 0 there, every row but the acceleration bounds
                   vanishes (the vanishing-row class of the joint sweep's chain)

The straight families are rest to rest with path_start = 0 (their bang-bang time is known);
`with_starts` gives the others a start velocity or a start parameter past 0.
"""
import importlib

import numpy as np

from conftest import PKG_NAME

syn = importlib.import_module(PKG_NAME + ".synthetic")

STRAIGHT = ("straight_trans", "straight_rot", "straight_joint", "straight_accel")
CURVED = ("zero_jacobian", "singular", "idle")
FAMILIES = STRAIGHT + CURVED
SAMPLE_COUNTS = (3, 4, 64, 2000)

_SEED = {name: 9_000_000 + 10_000 * k for k, name in enumerate(FAMILIES)}


def _jacobian(rng, D):
    """A constant 6 x D Jacobian: a unit block plus a random part (full row rank for D >= 6)."""
    J = 0.25 * rng.standard_normal((6, D))
    for r in range(6):
        J[r, r % D] += 1.0
    return J


def _straight(name, B, D, N, rng):
    length = 1.0
    delta = np.full(B, length / (N - 1))
    q = np.zeros((B, N, D))
    J = np.zeros((B, N, 6, D))
    vmax = rng.uniform(0.8, 1.6, (B, D))
    amax = rng.uniform(2.0, 5.0, (B, D)) * (1.0 if name == "straight_accel" else 3.0)
    vt, vr = np.zeros(B), np.zeros(B)
    c = np.zeros((B, D))
    for b in range(B):
        cb = rng.uniform(0.3, 1.2, D) * rng.choice([-1.0, 1.0], D)
        q0 = rng.uniform(-1.0, 1.0, D)
        s = np.arange(N) * delta[b]
        q[b] = q0 + s[:, None] * cb
        Jb = _jacobian(rng, D)
        J[b] = Jb
        c[b] = cb
        vj = np.min(0.8 * vmax[b] / np.abs(cb))           # fastest path speed the joints allow
        nt, nr = np.linalg.norm(Jb[:3] @ cb), np.linalg.norm(Jb[3:] @ cb)
        f = dict(straight_trans=(0.5, 10.0), straight_rot=(10.0, 0.5),
                 straight_joint=(10.0, 10.0), straight_accel=(1e3, 1e3))[name]
        vt[b], vr[b] = f[0] * vj * nt, f[1] * vj * nr
        if name == "straight_accel":
            vmax[b] *= 1e3
    return dict(ik_positions=q, jacobians=J, vmax=vmax, amax=amax, vtrans=vt, vrot=vr,
                path_start=np.zeros(B), delta=delta, sd_start=np.zeros(B), time_start=np.zeros(B),
                num_samples=N, safety=0.8, direction=c, length=np.full(B, length))


def make_family(name, B, D, N, seed=0):
    """B paths of family `name` with D joints and N samples, seeded by (name, D, N, seed)."""
    first = _SEED[name] + 100 * D + 7 * N + 1000 * seed
    rng = np.random.default_rng(first)
    if name in STRAIGHT:
        b = _straight(name, B, D, N, rng)
    else:
        b = syn.make_cartesian_batch(B, D, N, num_waypoints=6, first_path_index=first)
        q, J = b["ik_positions"], b["jacobians"]
        if name == "zero_jacobian":
            J[:] = 0.0
        elif name == "singular" and N >= 3:
            m = N // 2
            for i in range(B):
                d1 = q[i, m + 1] - q[i, m]                # q'_m up to the factor 1 / delta
                proj = np.eye(D) - np.outer(d1, d1) / np.dot(d1, d1)
                J[i, m] = J[i, m] @ proj
        elif name == "idle" and N >= 4:
            a, e = N // 3, N // 3 + max(N // 5, 1)
            q[:, a:e + 1] = q[:, a:a + 1]                 # an interior stop
            q[:, :max(N // 20, 1) + 1] = q[:, :1]         # and a slow start
            # the Jacobians stay those of the original path: only J q' matters, and q' = 0 there
    for k in list(b):
        if isinstance(b[k], np.ndarray):
            b[k] = np.ascontiguousarray(b[k])
    b["family"] = name
    return b


def with_starts(b, seed=0):
    """Give some paths a start velocity or a start parameter past 0 (a shifted s grid; the IK
    table itself stays what it is), and a nonzero start time. Path 0 is left alone."""
    B = b["ik_positions"].shape[0]
    rng = np.random.default_rng(seed + 23)
    pick = np.arange(B) % 3
    b["sd_start"] = np.ascontiguousarray(np.where(pick == 1, rng.uniform(0.01, 0.05, B), 0.0))
    b["path_start"] = np.ascontiguousarray(np.where(pick == 2, rng.uniform(0.1, 2.0, B), 0.0))
    b["time_start"] = np.ascontiguousarray(np.where(pick >= 1, rng.uniform(0.5, 80.0, B), 0.0))
    return b


def concat(batches):
    """Concatenate batches of one D and one N along the path axis."""
    keys = ("ik_positions", "jacobians", "vmax", "amax", "vtrans", "vrot", "path_start", "delta",
            "sd_start", "time_start")
    out = {k: np.ascontiguousarray(np.concatenate([x[k] for x in batches])) for k in keys}
    out["num_samples"] = batches[0]["num_samples"]
    out["safety"] = batches[0]["safety"]
    return out


def oracle_solve(tpo, b, nthreads=8):
    return tpo.time_cartesian_batch(b["ik_positions"], b["jacobians"], b["vmax"], b["amax"],
                                    b["vtrans"], b["vrot"], b["path_start"], b["delta"],
                                    sd_start=b["sd_start"], time_start=b["time_start"],
                                    safety=b["safety"], nthreads=nthreads)


# ------------------------------------------------------------------ pose splines
def pose_edge_paths(P=16, N=400):
    """Pose splines (knots [B][P+3], translation [B][P][3], rotation [B][P][4], path_start [B],
    delta [B], N) that reach the edges of the quaternion B-spline, one path per edge:
      0 random rotations (the nv > 1e-12 branch everywhere), w < 0 on the last control point
      1 identical neighbours (p0^-1 p1 = 1: |v| = 0, the branch below 1e-12)
      2 neighbours 1e-13 rad apart (|v| ~ 5e-14: the branch below 1e-12, not at 0)
      3 relative rotations of pi -/+ 1e-6 (w of p0^-1 p1 = +-5e-7: either side of the flip)
      4 antipodal neighbours (p1 = -p0: w = -1 with |v| = 0, flipped to +1)
      5 parameters exactly on the knots (delta = 1/8 or 1 of a knot interval, path_start 0)
      6 the k_end - delta padding edge: delta = k_end / 64, so that sample 63 sits exactly on
        k_end - delta (padded) and sample 62 one delta before it (evaluated)
    Knots are clamped and uniform (k = 0, 0, 0, 1, ..., P-2, P-2, P-2), translations random.
    N must be at least 65 and, for P > 8, at least P - 1."""
    rng = np.random.default_rng(4242 + P)
    B = 7
    kn = np.concatenate([[0.0, 0.0], np.arange(P - 1, dtype=float), [P - 2.0, P - 2.0]])
    knots = np.tile(kn, (B, 1))
    tr = rng.uniform(-1.0, 1.0, (B, P, 3))
    rot = rng.standard_normal((B, P, 4))
    rot /= np.linalg.norm(rot, axis=2, keepdims=True)
    rot[0, -1] *= -np.sign(rot[0, -1, 0])                 # the last pose has w < 0
    axis = lambda: (lambda a: a / np.linalg.norm(a))(rng.standard_normal(3))

    def qaxis(ang, ax):
        return np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])

    for j in range(1, P, 3):
        rot[1, j] = rot[1, j - 1]
        rot[2, j] = _qmul_d(rot[2, j - 1], qaxis(1e-13, axis()))
        rot[3, j] = _qmul_d(rot[3, j - 1], qaxis(np.pi - (1e-6 if j % 2 else -1e-6), axis()))
        rot[4, j] = -rot[4, j - 1]
    rot[2:4] /= np.linalg.norm(rot[2:4], axis=2, keepdims=True)
    kend = kn[-1]
    delta = np.full(B, kend / (N - 40))                  # the last samples run past the end
    start = np.zeros(B)
    start[1::2] = 0.3 * delta[1::2]
    assert N >= 65 and N >= kend + 1
    delta[5], start[5] = (1.0 / 8 if kend * 8 + 1 <= N else 1.0), 0.0   # samples on the knots
    delta[6], start[6] = kend / 64, 0.0                  # exact in binary: i delta = k_end - delta at 63
    return dict(knots=np.ascontiguousarray(knots), translation=np.ascontiguousarray(tr),
                rotation=np.ascontiguousarray(rot), path_start=start, delta=delta, N=N)


def _qmul_d(a, b):
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])

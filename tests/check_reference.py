"""The numpy statement of the solution check (include/tpamd.h tpamd_check_*;
TimeOptimalPathProfile::SolutionSatisfiesConstraints, time_optimal_path_timing.cc:492-518), and the
rows the CPU oracle forms for a path of a synthetic joint or Cartesian batch.

For rows [N][C], sd2 [N] and sdd [N]:
    v = a * sdd + b * sd2                      two products, one sum (numpy does not contract)
    violated  <=>  (v + KT < lower) | (v - KT > upper)
    excess = max(lower - v, v - upper)         NaN if either difference is NaN
and the record is (violations, worst_excess, worst_sample, worst_row, first_sample): the count, the
largest excess that is not NaN with the first flattened index i * C + c that attains it, and the
first sample with a violated row; NaN / -1 where there is none. NOT_CHECKED is the record of a path
that is not checked."""
import numpy as np

KT = 2.220446049250313e-16 * 1e5          # kTiny, time_optimal_path_timing.h:275-279
NOT_CHECKED = (-1, np.nan, -1, -1, -1)
KEYS = ("violations", "worst_excess", "worst_sample", "worst_row", "first_sample")

# (D, N, W) of synthetic.make_joint_batch(16, D, N, W) / make_cartesian_batch(paths, D, N, W)
JOINT_SHAPES = ((1, 3, 2), (3, 64, 3), (7, 65, 4), (6, 257, 5), (14, 129, 6), (16, 33, 3), (8, 200, 10))
CARTESIAN_SHAPES = ((1, 3, 2), (3, 64, 3), (6, 65, 4), (7, 257, 5), (14, 129, 6), (16, 33, 3))


def cartesian_paths(shape):
    return 8 if shape == (1, 3, 2) else 16


def check_rows(A, B, lo, hi, sd2, sdd):
    A, B, lo, hi = (np.asarray(x, dtype=np.float64) for x in (A, B, lo, hi))
    N, C = A.shape
    sd2 = np.asarray(sd2, dtype=np.float64).reshape(N, 1)
    sdd = np.asarray(sdd, dtype=np.float64).reshape(N, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        v = A * sdd + B * sd2
        bad = (v + KT < lo) | (v - KT > hi)
        ex = np.maximum(lo - v, v - hi)
    count = int(bad.sum())
    hit = np.flatnonzero(bad.any(axis=1))
    first = int(hit[0]) if hit.size else -1
    flat = ex.reshape(-1)
    if np.isnan(flat).all():
        return (count, np.nan, -1, -1, first)
    k = int(np.nanargmax(flat))               # the first index among equal values
    return (count, float(flat[k]), k // C, k % C, first)


def same_record(got, want):
    """Bit equality of two records (NaN by position; -0.0 and 0.0 differ)."""
    if tuple(int(x) for x in (got[0], got[2], got[3], got[4])) != tuple(int(x) for x in (want[0], want[2], want[3], want[4])):
        return False
    return np.float64(got[1]).tobytes() == np.float64(want[1]).tobytes()


def record_of(out, b):
    """Record of path b from a dict of five arrays."""
    return tuple(np.asarray(out[k])[b].item() for k in KEYS)


def joint_rows(tpo, batch, b, n, safety=None, path_start=None, delta=None):
    """The oracle's rows [n][2D] of path b of a synthetic joint batch sampled at n points."""
    ps = batch["path_start"][b] if path_start is None else path_start
    dl = batch["delta"][b] if delta is None else delta
    _, q1, q2 = tpo.joint_sample_path(batch["knots"][b], batch["control_points"][b], ps, dl, n)
    return tpo.joint_constraint_setup(q1, q2, batch["vmax"][b], batch["amax"][b],
                                      batch["safety"] if safety is None else safety)


def jacobian_times_q1(J, q1):
    """J q' [n][6], the D terms added in index order starting from 0."""
    acc = np.zeros(J.shape[:2])
    for d in range(J.shape[2]):
        acc = acc + J[:, :, d] * q1[:, d:d + 1]
    return acc


def cartesian_rows(tpo, q, J, vmax, amax, vtrans, vrot, delta, safety):
    """The oracle's rows [n][2D + 2] of one Cartesian path: q [n][D], J [n][6][D]."""
    q = np.ascontiguousarray(q, dtype=np.float64)
    J = np.ascontiguousarray(J, dtype=np.float64)
    q1, q2 = tpo.cartesian_path_derivatives(q, delta)
    return tpo.cartesian_constraint_setup(q1, q2, jacobian_times_q1(J, q1), vmax, amax, vtrans, vrot, safety)


def cartesian_batch_rows(tpo, batch, b, n=None):
    n = batch["ik_positions"].shape[1] if n is None else n
    return cartesian_rows(tpo, batch["ik_positions"][b, :n], batch["jacobians"][b, :n], batch["vmax"][b],
                          batch["amax"][b], batch["vtrans"][b], batch["vrot"][b], batch["delta"][b], batch["safety"])


def oracle_profile(tpo, rows, s_start, s_end, sd_start=0.0, time_start=0.0):
    """The oracle's solve of one path on `rows`, as the planner runs it (max(100, 10 N) loops).
    Returns (status, profile)."""
    A = rows[0]
    N, C = A.shape
    p = tpo.Profile(N, C)
    p.set_max_loops(max(100, 10 * N))
    rc = p.setup(*rows, float(s_start), float(s_end), float(sd_start), 0.0, float(time_start))
    if rc == 0:
        rc = p.optimize()
    return rc, p


def oracle_counts(tpo, batch, cartesian=False):
    """Per path of a synthetic batch: (status, violations as Profile.constraint_violations() reports
    them, helper record on the oracle's own sd2 / sdd, rows)."""
    key = "ik_positions" if cartesian else "control_points"
    B = batch[key].shape[0]
    N = batch["ik_positions"].shape[1] if cartesian else int(batch["num_samples"])
    out = []
    for b in range(B):
        rows = cartesian_batch_rows(tpo, batch, b) if cartesian else joint_rows(tpo, batch, b, N)
        s0 = float(batch["path_start"][b])
        rc, p = oracle_profile(tpo, rows, s0, s0 + float(batch["delta"][b]) * (N - 1), batch["sd_start"][b],
                               batch["time_start"][b])
        rec = check_rows(*rows, p.sd2, p.sdd) if rc == 0 else NOT_CHECKED
        out.append((rc, p.constraint_violations(), rec, rows))
    return out

"""An independent high-precision reference for the joint-path solver's outputs (test helper).

The B-spline is evaluated here from its definition -- the Cox-de Boor recursion on the knot
span, with derivatives taken as the derived B-spline of degree p - 1 on the differenced
control points -- in numpy.longdouble, and cross-checked with mpmath on a few points through
the textbook recursive basis N_{i,p} and its derivative formula. Nothing here calls or restates
the oracle's spline code.

`check_profile` then asserts what a solved profile must satisfy whatever solver produced it:
the sampling, q / qd / qdd against the exact spline, the time integration, the joint velocity
limit, rest at the end, and the acceleration limit (see `check_profile` for its exact rule).
`bang_bang_time` is the analytic minimum time of a straight move that is linear in u.
"""
import numpy as np

LD = np.longdouble
KTINY = 2.220446049250313e-16 * 1e5      # the reference's kTiny


# ----------------------------------------------------------------------- B-spline
def _span(knots, degree, num_points, u):
    """Index i of the knot span [k_i, k_i+1) holding u; u at the last knot uses the last
    nonempty span (the curve is closed at its end)."""
    i = np.searchsorted(knots, u, side="right") - 1
    return np.clip(i, degree, num_points - 1)


def _eval_degree(knots, degree, points, u):
    """sum_r N_{i-p+r,p}(u) P_{i-p+r} on the span of each u (Cox-de Boor triangle)."""
    M = u.shape[0]
    n = points.shape[0]
    if n == 0:
        return np.zeros((M,) + points.shape[1:], dtype=LD)
    i = _span(knots, degree, n, u)
    N = [np.ones(M, dtype=LD)]
    left = [None] * (degree + 1)
    right = [None] * (degree + 1)
    for j in range(1, degree + 1):
        left[j] = u - knots[i + 1 - j]
        right[j] = knots[i + j] - u
        saved = np.zeros(M, dtype=LD)
        for r in range(j):
            temp = N[r] / (right[r + 1] + left[j - r])
            N[r] = saved + right[r + 1] * temp
            saved = left[j - r] * temp
        N.append(saved)
    out = np.zeros((M,) + points.shape[1:], dtype=LD)
    for r in range(degree + 1):
        out += N[r].reshape((M,) + (1,) * (points.ndim - 1)) * points[i - degree + r]
    return out


def eval_spline(knots, degree, points, u, nder=2):
    """Value and the first `nder` derivatives of a clamped B-spline at parameters u:
    returns [nder + 1][len(u)][D] in longdouble. u must lie in [knots[0], knots[-1]]."""
    k = np.asarray(knots, dtype=LD)
    P = np.asarray(points, dtype=LD)
    u = np.asarray(u, dtype=LD)
    res = []
    p = degree
    for _ in range(nder + 1):
        if p < 0:
            res.append(np.zeros((u.shape[0], P.shape[1]), dtype=LD))
            continue
        res.append(_eval_degree(k, p, P, u))
        # derivative curve: degree p - 1 on k[1:-1], Q_i = p (P_{i+1} - P_i) / (k_{i+p+1} - k_{i+1})
        if p == 0:
            p -= 1
            continue
        den = k[p + 1:p + P.shape[0]] - k[1:P.shape[0]]
        safe = np.where(den > 0, den, 1)
        Q = np.where((den > 0)[:, None], p * (P[1:] - P[:-1]) / safe[:, None], 0)
        P, k, p = Q, k[1:-1], p - 1
    return np.stack(res)


def eval_spline_mp(knots, degree, points, u, nder=2, dps=40):
    """The same quantities at one parameter u with mpmath, from the recursive definition
    N_{i,0} = [k_i <= u < k_i+1], N_{i,p} = w N_{i,p-1} + (1 - w') N_{i+1,p-1} (0/0 = 0), and
    N'_{i,p} = p N_{i,p-1} / (k_i+p - k_i) - p N_{i+1,p-1} / (k_i+p+1 - k_i+1)."""
    import mpmath
    old = mpmath.mp.dps
    mpmath.mp.dps = dps
    try:
        k = [mpmath.mpf(float(x)) for x in knots]
        u = mpmath.mpf(float(u))
        last = len(k) - 1

        def N(i, p, d):
            if d > 0:
                if p == 0:
                    return mpmath.mpf(0)
                a = k[i + p] - k[i]
                b = k[i + p + 1] - k[i + 1]
                t1 = p * N(i, p - 1, d - 1) / a if a != 0 else mpmath.mpf(0)
                t2 = p * N(i + 1, p - 1, d - 1) / b if b != 0 else mpmath.mpf(0)
                return t1 - t2
            if p == 0:
                if k[i] <= u < k[i + 1]:
                    return mpmath.mpf(1)
                # closed at the end of the curve: the last nonempty span owns u = k[-1]
                if u == k[last] and k[i] < k[i + 1] == k[last]:
                    return mpmath.mpf(1)
                return mpmath.mpf(0)
            a = k[i + p] - k[i]
            b = k[i + p + 1] - k[i + 1]
            t1 = (u - k[i]) / a * N(i, p - 1, 0) if a != 0 else mpmath.mpf(0)
            t2 = (k[i + p + 1] - u) / b * N(i + 1, p - 1, 0) if b != 0 else mpmath.mpf(0)
            return t1 + t2

        pts = np.asarray(points, dtype=float)
        out = []
        for d in range(nder + 1):
            row = []
            for c in range(pts.shape[1]):
                row.append(mpmath.fsum(N(i, degree, d) * mpmath.mpf(float(pts[i, c]))
                                       for i in range(pts.shape[0])))
            out.append(row)
        return out
    finally:
        mpmath.mp.dps = old


# ----------------------------------------------------------------- path sampling
def sample_path(knots, cps, path_start, delta, N):
    """q, q', q'' [N][D] (longdouble) at the parameters path_start + i * delta, clamped to the
    knot range; at or past knots[-1] + delta the sample is the last control point at rest
    (the reference's end padding, timeable_path_joint_spline.cc:294-318)."""
    knots = np.asarray(knots, dtype=float)
    cps = np.asarray(cps, dtype=float)
    # the parameters themselves are doubles, as the reference computes them: a sample that
    # falls on a knot in double arithmetic takes the span that starts there
    par = float(path_start) + np.arange(N) * float(delta)
    pad = ~(par < knots[-1] + float(delta))
    u = np.clip(par, knots[0], knots[-1])
    q, q1, q2 = eval_spline(knots, 2, cps, u, 2)
    q[pad] = np.asarray(cps[-1], dtype=LD)
    q1[pad] = 0
    q2[pad] = 0
    return q, q1, q2


def bang_bang_time(knots, cps, vmax, amax, safety):
    """Rest-to-rest minimum time over a path that is linear in u (q' constant, q'' = 0):
    sd <= v = min_j safety vmax_j / |q'_j|, |sdd| <= a = min_j safety amax_j / |q'_j|;
    a triangle when v^2 / a >= L, a trapezoid otherwise."""
    knots = np.asarray(knots, dtype=LD)
    L = knots[-1] - knots[0]
    q1 = eval_spline(knots, 2, cps, np.array([knots[0] + L / 2], dtype=LD), 1)[1][0]
    m = np.abs(q1) > 0
    v = np.min(LD(safety) * np.asarray(vmax, dtype=LD)[m] / np.abs(q1[m]))
    a = np.min(LD(safety) * np.asarray(amax, dtype=LD)[m] / np.abs(q1[m]))
    if v * v / a >= L:
        return float(2 * np.sqrt(L / a))
    return float(L / v + v / a)


# ---------------------------------------------------------------- property check
def accel_rule_violations(q1, q2, sd, sdd, amax, safety=0.8):
    """The acceleration rule of check_profile on a batch: q1, q2 [B][N][D], sd, sdd [B][N],
    amax [B][D]. Returns a [B][N] mask of samples where |q' sdd + q'' sd^2| exceeds
    safety amax (1 + 1e-9) on some joint and no sample within one of them has sdd == 0.0."""
    q1, q2 = np.asarray(q1, dtype=LD), np.asarray(q2, dtype=LD)
    sd, sdd = np.asarray(sd, dtype=LD)[..., None], np.asarray(sdd)
    acc = q1 * sdd.astype(LD)[..., None] + q2 * sd * sd
    bound = LD(safety) * np.asarray(amax, dtype=LD)[:, None, :]
    over = np.any(np.abs(acc) > bound * (1 + LD(1e-9)), axis=2)
    z = sdd == 0.0
    near = z.copy()
    near[:, 1:] |= z[:, :-1]
    near[:, :-1] |= z[:, 1:]
    return over & ~near


def _outputs(out):
    g = {}
    for k in ("time", "s", "sd", "sdd", "q", "qd", "qdd", "status"):
        v = out["t" if k == "time" and "t" in out else k]
        g[k] = v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)
    return g


def check_profile(batch, out, safety=0.8, paths=None, stationary_ok=False, accel_allowance=0):
    """Assert the properties of every solved path (status 0) of `out` (oracle or engine
    outputs) for the joint batch `batch`. Returns a report dict with counts.

    Per path of n samples (n = num_samples_per_path[b] for a ragged batch):
      - s_i = s_start + i ds with ds = (s_end - s_start) / (n - 1), s_end = path_start +
        (n - 1) delta exactly at the last sample, and s_i = path_start + i delta to 1e-12;
      - q equals the spline at path_start + i delta (end padding included) to 1e-12 of the
        control points' size;
      - qd = q'(s) sd to 1e-11 relative (plus the rounding of q' near its zeros);
      - qdd = clip(q' sdd + q'' sd^2, +-amax), likewise;
      - t_0 = time_start, t_i - t_{i-1} = 2 ds / (sd_{i-1} + sd_i), exactly 0 where both are
        0, to 1e-12 of |t| over the path; time never decreases;
      - |qd| <= safety vmax (1 + 1e-12), sd_{n-1} = 0;
      - acceleration: |q' sdd + q'' sd^2| <= safety amax (1 + 1e-9), except within one sample
        of a sample whose sdd is exactly 0.0 (the reference's answer when FindSdd finds no
        admissible sdd, and on a stretch where sd = 0 on both ends of a step). With
        stationary_ok, samples whose q' is below kTiny on every joint (a stretch where the path
        stands still in joint space, whose rows constrain nothing) and their neighbours are
        exempt as well.

    The acceleration rule does not hold everywhere. Measured on the oracle with the families
    of tests/structured_paths.py (4 paths per family and D = 1 .. 16; "excused" = over the
    bound next to an sdd == 0 sample, "other" = over the bound elsewhere, largest ratio):
      - N = 2000, rest to rest: 0 other in straight_*, idle_*, near_idle, tie_scaled,
        tie_mirror, velocity_bound, stop_first and out_and_back (stop_first and stop_interior
        with stationary_ok); tie_all 1 (7.3e3x), spread_up 5 (1.2x), spread_down 11 (7e5x),
        accel_bound 3 (4e4x), stop_interior 2 (1.0x), stop_last 5 (1.7x).
      - N <= 65: 2 .. 27 other per family, up to 37x: with a coarse grid the reference's sdd of a
        sample is the acceleration of the step that leaves it, not a point value.
      - with sd_start > 0 or path_start > 0: up to 286 other per family (accel_bound), the
        reference integrating a constant sdd through a stretch behind a start velocity.
    accel_allowance (None: count only) sets how many "other" samples a call tolerates; the
    tests hold it at 0 exactly where the table above has 0, and pin each family's counts and
    largest ratio elsewhere (test_structured_paths_cpu.ACCEL_EXCEPTIONS, which also says where
    the large ratios come from).
    """
    g = _outputs(out)
    B, Nmax = g["time"].shape
    ns = batch.get("num_samples_per_path")
    rep = dict(paths=0, accel_excused=0, accel_excused_max_ratio=0.0, accel_unexcused=0,
               accel_unexcused_max_ratio=0.0, stationary=0,
               sdd_zero=0, sd_cap=0, tiny_rows=0, vel_active=0, samples=0)
    for b in range(B) if paths is None else paths:
        if g["status"][b] != 0:
            continue
        n = Nmax if ns is None else int(ns[b])
        rep["paths"] += 1
        rep["samples"] += n
        t, s, sd, sdd = (g[k][b, :n] for k in ("time", "s", "sd", "sdd"))
        q, qd, qdd = (g[k][b, :n] for k in ("q", "qd", "qdd"))
        vmax = np.asarray(batch["vmax"][b], dtype=LD)
        amax = np.asarray(batch["amax"][b], dtype=LD)
        p0, dl = float(batch["path_start"][b]), float(batch["delta"][b])
        cps = np.asarray(batch["control_points"][b])
        where = "path %d" % b

        # sampling
        s_end = p0 + dl * (n - 1)
        ds = (s_end - p0) / (n - 1)
        assert s[-1] == s_end, where + ": s_end"
        s_ref = LD(p0) + np.arange(n, dtype=LD) * LD(dl)
        assert np.all(np.abs(s - s_ref) <= 1e-12 * max(abs(s_end), 1.0)), where + ": s"

        # q, qd, qdd against the exact spline
        rq, r1, r2 = sample_path(batch["knots"][b], cps, p0, dl, n)
        cscale = max(float(np.abs(cps).max()), 1e-300)
        assert np.all(np.abs(q - rq) <= 1e-12 * cscale), where + ": q"
        # rounding floors: a double evaluation of q' (q'') carries about eps * |cps| / h (/ h^2)
        # of absolute error, h the shortest knot interval, also where q' is exactly 0
        kn = np.asarray(batch["knots"][b], dtype=float)
        h = float(np.diff(kn)[np.diff(kn) > 0].min())
        e1 = LD(1e-13 * cscale / h)
        e2 = LD(1e-13 * cscale / (h * h))
        m1 = np.abs(r1).max(axis=0) + e1           # per joint: size of q' on this path
        m2 = np.abs(r2).max(axis=0) + e2
        sdL, sddL = sd.astype(LD)[:, None], sdd.astype(LD)[:, None]
        qd_ref = r1 * sdL
        tol = 1e-11 * np.abs(qd_ref) + 1e-14 * m1 * sdL + e1 * sdL
        assert np.all(np.abs(qd - qd_ref) <= tol), where + ": qd"
        acc = r1 * sddL + r2 * sdL * sdL
        qdd_ref = np.clip(acc, -amax, amax)
        tol = 1e-11 * np.abs(qdd_ref) + (1e-14 * m1 + e1) * np.abs(sddL) + \
            (1e-14 * m2 + e2) * sdL * sdL
        assert np.all(np.abs(qdd - qdd_ref) <= tol), where + ": qdd"

        # time
        assert t[0] == batch["time_start"][b], where + ": t0"
        both0 = (sd[:-1] == 0) & (sd[1:] == 0)
        den = sd[:-1].astype(LD) + sd[1:].astype(LD)
        step = np.where(both0, 0, 2 * LD(ds) / np.where(both0, 1, den))
        t_ref = LD(t[0]) + np.concatenate([[LD(0)], np.cumsum(step)])
        assert np.all(np.abs(t - t_ref) <= 1e-12 * max(float(np.abs(t).max()), 1e-300)), \
            where + ": time steps"
        assert np.all(np.diff(t)[both0] == 0), where + ": time moves where sd = 0"
        assert np.all(np.diff(t) >= 0), where + ": time decreases"

        # limits
        # (sample 0 carries the caller's sd_start, which need not respect the limit)
        lim = slice(1 if batch["sd_start"][b] > 0 else 0, n)
        assert np.all(np.abs(qd[lim]) <= LD(safety) * vmax * (1 + LD(1e-12))), where + ": |qd|"
        assert sd[-1] == 0, where + ": sd end"
        bound = LD(safety) * amax
        over = np.any(np.abs(acc) > bound * (1 + LD(1e-9)), axis=1)
        near = np.zeros(n, bool)
        z = sdd == 0.0
        near |= z
        near[1:] |= z[:-1]
        near[:-1] |= z[1:]
        still = np.all(np.abs(r1) < KTINY, axis=1)
        if stationary_ok:
            near |= still
            near[1:] |= still[:-1]
            near[:-1] |= still[1:]
        bad = over & ~near
        rep["accel_unexcused"] += int(bad.sum())
        if bad.any():
            rep["accel_unexcused_max_ratio"] = max(rep["accel_unexcused_max_ratio"], float(
                np.max(np.abs(acc[bad]) / bound)))
        assert accel_allowance is None or rep["accel_unexcused"] <= accel_allowance, \
            "%s: acceleration bound broken at samples %s (x %s)" % (
                where, np.flatnonzero(bad)[:8],
                np.max(np.abs(acc[bad]) / bound, axis=1)[:8].astype(float))
        if over.any():
            rep["accel_excused"] += int(over.sum())
            rep["accel_excused_max_ratio"] = max(rep["accel_excused_max_ratio"], float(
                np.max(np.abs(acc[over]) / bound)))
        rep["stationary"] += int(still.sum())
        rep["sdd_zero"] += int(z.sum())
        rep["sd_cap"] += int((sd[1:-1] == 1000.0).sum())
        rep["tiny_rows"] += int(((np.abs(r1) < KTINY) & (np.abs(r1) > 0)).sum())
        rep["vel_active"] += int(np.any(np.abs(qd) >= LD(safety) * vmax * (1 - LD(1e-9)),
                                        axis=1).sum())
    return rep


# ===================================================================== Cartesian paths
# Quaternions are [w, x, y, z]. The operations below are the textbook definitions:
#   product           (a0 b0 - a.b, a0 b + b0 a + a x b)
#   inverse           conj(q) / |q|^2
#   log q             (log |q|, v/|v| atan2(|v|, w)),  and (log |q|, 0) where |v| = 0
#   exp q             e^w (cos |v|, v/|v| sin |v|),    and (e^w, 0) where |v| = 0
#   q^p               exp(p log q), taken after q is flipped to w >= 0
# The reference (splines/bsplineq.cc QuatLog) returns (log |q|, v) instead of the atan2 form
# whenever |v| <= 1e-12. For w > 0 the two differ by |v| (1/w - 1) + O(|v|^3), below 1e-24 for a
# unit quaternion. For w < 0 and |v| ~ 0 (q ~ -1, whose rotation angle is 2 pi: the identity) the
# branch gives log q ~ 0, which is no logarithm of -1; but QuatPower flips q to w >= 0 before it
# takes the log (NormalizeIfNecessaryAndEnsurePositiveReal), so on a spline this case never
# reaches QuatLog: an antipodal neighbour (p1 = -p0, p0^-1 p1 = -1) becomes +1, and its power is
# the identity -- no rotation between two representations of one orientation. The flip here
# reproduces that. The same flip decides the direction of interpolation near a relative rotation
# of pi (w of p0^-1 p1 crossing 0): w < 0 turns the other way round, as in the reference.
# Where QuatPower renormalises only past |q|^2 - 1 > 1e-12, the definitions here carry |q| through
# log and exp and normalise the product once: identical directions, a different norm by at most
# that 1e-12 (and by about 1e-16 for unit control points).
MP_DPS = 40


def _qmul(a, b):
    """Hamilton product of [..., 4] arrays (any float dtype)."""
    a0, a1, a2, a3 = (a[..., k] for k in range(4))
    b0, b1, b2, b3 = (b[..., k] for k in range(4))
    return np.stack([a0 * b0 - a1 * b1 - a2 * b2 - a3 * b3,
                     a0 * b1 + a1 * b0 + a2 * b3 - a3 * b2,
                     a0 * b2 + a2 * b0 + a3 * b1 - a1 * b3,
                     a0 * b3 + a3 * b0 + a1 * b2 - a2 * b1], axis=-1)


def _qinv(q):
    n2 = np.sum(q * q, axis=-1, keepdims=True)
    return q * np.array([1, -1, -1, -1], dtype=q.dtype) / n2


def quat_log(q):
    """log of [..., 4] quaternions in longdouble (definition above)."""
    q = np.asarray(q, dtype=LD)
    n2 = np.sum(q * q, axis=-1)
    nv = np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1))
    ang = np.arctan2(nv, q[..., 0])
    f = np.where(nv > 0, ang / np.where(nv > 0, nv, 1), 0)
    return np.concatenate([(LD(0.5) * np.log(n2))[..., None], q[..., 1:] * f[..., None]], axis=-1)


def quat_exp(q):
    """exp of [..., 4] quaternions in longdouble (definition above)."""
    q = np.asarray(q, dtype=LD)
    nv = np.sqrt(np.sum(q[..., 1:] ** 2, axis=-1))
    f = np.where(nv > 0, np.sin(nv) / np.where(nv > 0, nv, 1), 0)
    e = np.exp(q[..., 0])
    return np.concatenate([(e * np.cos(nv))[..., None], q[..., 1:] * (e * f)[..., None]], axis=-1)


def quat_power(q, p):
    """q^p = exp(p log q) with q flipped to w >= 0 first; p broadcasts over q's leading axes."""
    q = np.asarray(q, dtype=LD)
    q = np.where((q[..., 0] < 0)[..., None], -q, q)
    return quat_exp(quat_log(q) * np.asarray(p, dtype=LD)[..., None])


def _mp_quat():
    """The same four operations on 4-tuples of mpmath numbers (the caller sets mp.dps)."""
    import mpmath as M

    def mul(a, b):
        return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])

    def inv(q):
        n2 = M.fsum(x * x for x in q)
        return (q[0] / n2, -q[1] / n2, -q[2] / n2, -q[3] / n2)

    def log(q):
        nv = M.sqrt(q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
        f = M.atan2(nv, q[0]) / nv if nv > 0 else M.mpf(0)
        return (M.log(M.fsum(x * x for x in q)) / 2, q[1] * f, q[2] * f, q[3] * f)

    def exp(q):
        nv = M.sqrt(q[1] ** 2 + q[2] ** 2 + q[3] ** 2)
        f = M.sin(nv) / nv if nv > 0 else M.mpf(0)
        e = M.exp(q[0])
        return (e * M.cos(nv), e * f * q[1], e * f * q[2], e * f * q[3])

    def power(q, p):
        if q[0] < 0:
            q = tuple(-x for x in q)
        return exp(tuple(p * x for x in log(q)))

    return M, mul, inv, log, exp, power


def quat_exp_mp(q, dps=MP_DPS):
    """exp of one quaternion with mpmath at `dps` digits -> 4 floats."""
    M, _, _, _, exp, _ = _mp_quat()
    with M.workdps(dps):
        return np.array([float(x) for x in exp(tuple(M.mpf(float(x)) for x in q))])


def quat_log_mp(q, dps=MP_DPS):
    M, _, _, log, _, _ = _mp_quat()
    with M.workdps(dps):
        return np.array([float(x) for x in log(tuple(M.mpf(float(x)) for x in q))])


def _positive_unit(q):
    q = q / np.sqrt(np.sum(q * q, axis=-1, keepdims=True))
    return np.where((q[..., 0] < 0)[..., None], -q, q)


def pose_parameters(knots, path_start, delta, N):
    """The sample parameters path_start + i delta in double (as the reference forms them) and the
    mask of samples at or past knots[-1] - delta, which repeat the last control pose
    (timeable_path_cartesian_spline.cc:488, :499-502)."""
    par = float(path_start) + np.arange(N) * float(delta)
    pad = ~(par < float(knots[-1]) - float(delta))
    return par, pad


def sample_poses(knots, translation_points, rotation_points, path_start, delta, N):
    """Poses [N][7] = (t | q) in longdouble of the degree-2 translation spline and the degree-2
    quaternion B-spline q(u) = p0 (p0^-1 p1)^cum0 (p1^-1 p2)^cum1 on the span of u, with the
    cumulative basis cum0 = b1 + b2, cum1 = b2 of the span's basis b0, b1, b2 (bsplineq.cc's
    UpdateCumulativeBasis), normalised to unit length and w >= 0. Samples from knots[-1] - delta
    on are the last control pose as given (not normalised)."""
    kn = np.asarray(knots, dtype=float)
    tr = np.asarray(translation_points, dtype=float)
    rot = np.asarray(rotation_points, dtype=float)
    P = tr.shape[0]
    par, pad = pose_parameters(kn, path_start, delta, N)
    out = np.zeros((N, 7), dtype=LD)
    out[pad, :3] = tr[-1]
    out[pad, 3:] = rot[-1]
    live = np.flatnonzero(~pad)
    if live.size == 0:
        return out
    u = par[live].astype(LD)
    span = _span(kn, 2, P, par[live])
    basis = _eval_degree(kn.astype(LD), 2, np.eye(P, dtype=LD), u)      # [M][P]
    m = np.arange(live.size)
    b1, b2 = basis[m, span - 1], basis[m, span]
    out[live, :3] = eval_spline(kn, 2, tr, u, 0)[0]
    r = rot.astype(LD)
    p0, p1, p2 = r[span - 2], r[span - 1], r[span]
    q = _qmul(p0, quat_power(_qmul(_qinv(p0), p1), b1 + b2))
    q = _qmul(q, quat_power(_qmul(_qinv(p1), p2), b2))
    out[live, 3:] = _positive_unit(q)
    return out


def sample_poses_mp(knots, translation_points, rotation_points, path_start, delta, N, index,
                    dps=MP_DPS):
    """sample_poses at the sample indices `index` with mpmath at `dps` digits, the basis from the
    recursive definition (eval_spline_mp) -> [len(index)][7] floats."""
    M, mul, inv, _, _, power = _mp_quat()
    kn = np.asarray(knots, dtype=float)
    tr = np.asarray(translation_points, dtype=float)
    rot = np.asarray(rotation_points, dtype=float)
    P = tr.shape[0]
    par, pad = pose_parameters(kn, path_start, delta, N)
    res = np.zeros((len(index), 7))
    with M.workdps(dps):
        for k, i in enumerate(index):
            if pad[i]:
                res[k, :3], res[k, 3:] = tr[-1], rot[-1]
                continue
            s = int(_span(kn, 2, P, np.array([par[i]]))[0])
            b = eval_spline_mp(kn, 2, np.eye(P)[:, s - 2:s + 1], par[i], nder=0, dps=dps)[0]
            b1, b2 = b[1], b[2]
            t = [M.fsum(b[r] * M.mpf(float(tr[s - 2 + r, c])) for r in range(3)) for c in range(3)]
            p = [tuple(M.mpf(float(x)) for x in rot[s - 2 + r]) for r in range(3)]
            q = mul(p[0], power(mul(inv(p[0]), p[1]), b1 + b2))
            q = mul(q, power(mul(inv(p[1]), p[2]), b2))
            n = M.sqrt(M.fsum(x * x for x in q))
            q = tuple((x / n) * (-1 if q[0] < 0 else 1) for x in q)
            res[k, :3] = [float(x) for x in t]
            res[k, 3:] = [float(x) for x in q]
    return res


# ------------------------------------------------------------- Cartesian profile check
def cartesian_derivatives(q, delta):
    """q', q'' [N][D] in longdouble of an IK table q [N][D] sampled every `delta`, by the
    reference's forward differences (timeable_path_cartesian_spline.cc:39-68):
    q'_i = (q_i+1 - q_i) / delta for i < N-1 and q'_N-1 = 0; q''_i = (q'_i+1 - q'_i) / delta for
    0 < i < N-1 (so q''_N-2 = -q'_N-2 / delta) and q''_0 = q''_N-1 = 0."""
    q = np.asarray(q, dtype=LD)
    dl = LD(float(delta))
    q1 = np.zeros_like(q)
    q2 = np.zeros_like(q)
    q1[:-1] = (q[1:] - q[:-1]) / dl
    q2[1:-1] = (q1[2:] - q1[1:-1]) / dl
    return q1, q2


def cartesian_velocities(J, q1):
    """|J_t q'|, |J_r q'| [N] (longdouble) and the size of the terms of each dot product
    (|J_t| |q'|, |J_r| |q'| [N]): the bound on the rounding of a double evaluation."""
    J = np.asarray(J, dtype=LD)
    v6 = np.einsum("nrd,nd->nr", J, q1)
    m6 = np.einsum("nrd,nd->nr", np.abs(J), np.abs(q1))
    n = lambda x: np.sqrt(np.sum(x * x, axis=1))
    return n(v6[:, :3]), n(v6[:, 3:]), n(m6[:, :3]), n(m6[:, 3:])


# The Cartesian rows' tolerance. The LP keeps b sd^2 <= v^2 for its own double b = |J q'|^2 as it
# keeps q'^2 sd^2 <= (safety vmax)^2 on a joint velocity row (both are rows with A = 0), which
# check_profile holds to 1e-12 relative. b itself differs from the exact |J q'|^2 by the rounding
# of the forward difference (a few ulp of each q'_d) and of a D-term dot product in double:
# at most (D + 3) eps sum_d |J_rd q'_d| per row, which the check adds as an absolute term.
CART_REL_TOL = 1e-12
EPS = 2.220446049250313e-16


def check_cartesian_profile(batch, out, safety=0.8, paths=None, accel_allowance=0,
                            stationary_ok=True):
    """Assert the properties of every solved path (status 0) of `out` for the Cartesian batch
    `batch` (tests/cartesian_paths.py format). Returns a report dict with counts.

    Per path of N samples:
      - the s grid and the time integration exactly as check_profile states them; time never
        decreases, sd_{N-1} = 0;
      - q is the IK table bit for bit;
      - qd = q' sd and qdd = clip(q' sdd + q'' sd^2, +-amax) with (q', q'') of
        cartesian_derivatives, to 1e-12 relative plus the rounding of q' (4 eps |q'|) and of q''
        (8 eps (|q'_i| + |q'_i+1|) / delta) in double;
      - |qd| <= safety vmax (1 + 1e-12) (sample 0 exempt when sd_start > 0);
      - |J_t q'| sd <= v_trans (1 + CART_REL_TOL) + (D + 3) eps |J_t| |q'| sd, and the same for
        the rotation row with v_rot. No safety factor: the reference applies it to the joint
        limits only (timeable_path_cartesian_spline.cc:583-592);
      - the acceleration rule of check_profile (|q' sdd + q'' sd^2| <= safety amax (1 + 1e-9)
        except within one sample of sdd == 0.0, and with stationary_ok next to a sample whose q'
        is below kTiny on every joint).
    The report counts, besides check_profile's fields, the samples where each Cartesian row is
    active (|J q'| sd >= v (1 - 1e-9)): trans_active, rot_active, and the largest ratio of each
    to its limit (trans_max_ratio, rot_max_ratio).
    """
    g = _outputs(out)
    B, N = g["time"].shape
    D = np.asarray(batch["vmax"]).shape[1]
    rep = dict(paths=0, samples=0, accel_excused=0, accel_unexcused=0,
               accel_unexcused_max_ratio=0.0, sdd_zero=0, stationary=0, vel_active=0,
               trans_active=0, rot_active=0, trans_max_ratio=0.0, rot_max_ratio=0.0)
    for b in range(B) if paths is None else paths:
        if g["status"][b] != 0:
            continue
        rep["paths"] += 1
        rep["samples"] += N
        where = "path %d" % b
        t, s, sd, sdd = (g[k][b] for k in ("time", "s", "sd", "sdd"))
        q, qd, qdd = (g[k][b] for k in ("q", "qd", "qdd"))
        p0, dl = float(batch["path_start"][b]), float(batch["delta"][b])
        vmax = np.asarray(batch["vmax"][b], dtype=LD)
        amax = np.asarray(batch["amax"][b], dtype=LD)
        ik = np.asarray(batch["ik_positions"][b])

        s_end = p0 + dl * (N - 1)
        ds = (s_end - p0) / (N - 1)
        assert s[-1] == s_end, where + ": s_end"
        s_ref = LD(p0) + np.arange(N, dtype=LD) * LD(dl)
        assert np.all(np.abs(s - s_ref) <= 1e-12 * max(abs(s_end), 1.0)), where + ": s"

        assert np.array_equal(q, ik), where + ": q is not the IK table"
        r1, r2 = cartesian_derivatives(ik, dl)
        lim = slice(1 if batch["sd_start"][b] > 0 else 0, N)
        assert np.all(np.abs(qd[lim]) <= LD(safety) * vmax * (1 + LD(1e-12))), where + ": |qd|"
        rep["vel_active"] += int(np.any(np.abs(qd) >= LD(safety) * vmax * (1 - LD(1e-9)),
                                        axis=1).sum())
        vt, vr, mt, mr = cartesian_velocities(batch["jacobians"][b], r1)
        sdl = sd.astype(LD)
        for name, v, m, vlim in (("trans", vt, mt, batch["vtrans"][b]),
                                 ("rot", vr, mr, batch["vrot"][b])):
            vlim = LD(float(vlim))
            got = (v * sdl)[lim]
            bound = vlim * (1 + LD(CART_REL_TOL)) + (D + 3) * LD(EPS) * (m * sdl)[lim]
            bad = got > bound
            assert not bad.any(), "%s: |J_%s q'| sd over its limit at samples %s (x %s)" % (
                where, name[0], np.flatnonzero(bad)[:8], (got[bad] / vlim)[:8].astype(float))
            rep[name + "_active"] += int((got >= vlim * (1 - LD(1e-9))).sum())
            if got.size:
                rep[name + "_max_ratio"] = max(rep[name + "_max_ratio"], float(got.max() / vlim))

        sdL, sddL = sd.astype(LD)[:, None], sdd.astype(LD)[:, None]
        a1 = np.abs(r1)
        e1 = 4 * LD(EPS) * a1
        e2 = np.zeros_like(a1)
        e2[:-1] = 8 * LD(EPS) * (a1[:-1] + a1[1:]) / LD(dl)
        qd_ref = r1 * sdL
        assert np.all(np.abs(qd - qd_ref) <= LD(1e-12) * np.abs(qd_ref) + e1 * sdL), where + ": qd"
        acc = r1 * sddL + r2 * sdL * sdL
        qdd_ref = np.clip(acc, -amax, amax)
        tol = LD(1e-12) * np.abs(qdd_ref) + e1 * np.abs(sddL) + e2 * sdL * sdL
        assert np.all(np.abs(qdd - qdd_ref) <= tol), where + ": qdd"

        assert t[0] == batch["time_start"][b], where + ": t0"
        both0 = (sd[:-1] == 0) & (sd[1:] == 0)
        den = sd[:-1].astype(LD) + sd[1:].astype(LD)
        step = np.where(both0, 0, 2 * LD(ds) / np.where(both0, 1, den))
        t_ref = LD(t[0]) + np.concatenate([[LD(0)], np.cumsum(step)])
        assert np.all(np.abs(t - t_ref) <= 1e-12 * max(float(np.abs(t).max()), 1e-300)), \
            where + ": time steps"
        assert np.all(np.diff(t)[both0] == 0), where + ": time moves where sd = 0"
        assert np.all(np.diff(t) >= 0), where + ": time decreases"
        assert sd[-1] == 0, where + ": sd end"

        bound = LD(safety) * amax
        over = np.any(np.abs(acc) > bound * (1 + LD(1e-9)), axis=1)
        z = sdd == 0.0
        near = z.copy()
        near[1:] |= z[:-1]
        near[:-1] |= z[1:]
        still = np.all(np.abs(r1) < KTINY, axis=1)
        if stationary_ok:
            near |= still
            near[1:] |= still[:-1]
            near[:-1] |= still[1:]
        bad = over & ~near
        rep["accel_unexcused"] += int(bad.sum())
        if bad.any():
            rep["accel_unexcused_max_ratio"] = max(rep["accel_unexcused_max_ratio"], float(
                np.max(np.abs(acc[bad]) / bound)))
        assert accel_allowance is None or rep["accel_unexcused"] <= accel_allowance, \
            "%s: acceleration bound broken at samples %s" % (where, np.flatnonzero(bad)[:8])
        rep["accel_excused"] += int(over.sum())
        rep["sdd_zero"] += int(z.sum())
        rep["stationary"] += int(still.sum())
    return rep


def cartesian_bang_bang_time(c, J, vmax, amax, vtrans, vrot, length, safety=0.8):
    """Rest-to-rest minimum time T of a move q(s) = q0 + c s over s in [0, length] with a constant
    Jacobian J [6][D], with the peak path speed v_peak of that profile and its path acceleration a:
      v = min(safety vmax_j / |c_j|, v_trans / |J_t c|, v_rot / |J_r c|),
      a = min_j safety amax_j / |c_j|;
    a triangle (v_peak = sqrt(a length)) when v^2 / a >= length, else a trapezoid (v_peak = v).
    Returns (T, v_peak, a).

    The discrete problem does not reach T. The forward-difference end rule (cartesian_derivatives)
    gives the last sample q' = 0 -- no row there -- and sample N-2 the row of q'' = -q'/delta. The
    solver brings the path to rest at sample N-2 already (sd_N-2 = 0, on every straight move
    measured), and the last step, with sd = 0 at both ends, takes no time. The timed motion
    covers length - delta: the profile is the bang-bang optimum for that length, T(length - delta),
    which is T - delta / v for a trapezoid (one cruise sample time early) and
    T - delta / v_peak (1 + delta / (4 length) + ...) for a triangle. On the grid it reaches that
    optimum up to the corners where the profile switches between acceleration and cruise: constant
    acceleration and constant speed are integrated exactly by the trapezoid time steps, and a step
    that contains a switch costs at most (delta / v)(v - sd_k) / (v + sd_k) <=
    (delta / v) 2 a delta / v^2 more than the continuous profile (sd_k^2 >= v^2 - 2 a delta).
    Hence, with two corners, t_N-2 - t_0 lies in [T(length - delta), T(length - delta) +
    (delta / v_peak) 4 a delta / v_peak^2] (straight_window)."""
    c = np.asarray(c, dtype=LD)
    J = np.asarray(J, dtype=LD)
    m = np.abs(c) > 0
    cands = list(LD(safety) * np.asarray(vmax, dtype=LD)[m] / np.abs(c[m]))
    jc = J @ c
    for part, lim in ((jc[:3], vtrans), (jc[3:], vrot)):
        n = np.sqrt(np.sum(part * part))
        if n > 0:
            cands.append(LD(float(lim)) / n)
    v = min(cands)
    a = np.min(LD(safety) * np.asarray(amax, dtype=LD)[m] / np.abs(c[m]))
    L = LD(float(length))
    if v * v / a >= L:
        return float(2 * np.sqrt(L / a)), float(np.sqrt(a * L)), float(a)
    return float(L / v + v / a), float(v), float(a)


def straight_window(b, i, safety=0.8):
    """(lo, hi) for t_N-2 - t_0 of path i of a straight Cartesian family (cartesian_paths.py: its
    "direction" c and "length"), as derived in cartesian_bang_bang_time."""
    dl = float(b["delta"][i])
    args = (b["direction"][i], b["jacobians"][i, 0], b["vmax"][i], b["amax"][i], b["vtrans"][i],
            b["vrot"][i])
    Ts, vp, a = cartesian_bang_bang_time(*args, float(b["length"][i]) - dl, safety)
    _, vp, a = cartesian_bang_bang_time(*args, float(b["length"][i]), safety)
    return Ts * (1 - 1e-9), Ts + (dl / vp) * 4 * a * dl / (vp * vp) + 1e-9 * Ts

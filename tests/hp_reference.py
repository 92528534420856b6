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

"""Inputs of the resample and s(t)-query edge tests, shared by tests/test_resample_reference_cpu.py
(which holds tests/resample_reference.py to the oracle on them, and asserts that they reach the
branches they claim) and tests/test_gpu_resample_query_edges.py (which holds the kernels to both).

A resample case is a dict: sol (time, s, sd, sdd [B][N]; q, qd, qdd [B][N][D]), amax [B][D],
start [B], dt, and optionally status [B]. The trajectories are random numbers on a time axis built
per case, as in tests/test_gpu_resample_skip_long.py: the resamplers read nothing but the time
stamps to decide and interpolate or copy the rest.

A query batch is a dict: time, s, sd, sd2 [B][N], tq [B][K]. s is the exact linspace the solver
writes (time_optimal_path_timing.cc:540-547), sd2 = sd * sd, and time is rebuilt by the trapezoid
rule (:450-466), so two neighbours at rest share a time stamp. Hand-set brackets (query_hand_set)
reach the branches a consistent profile cannot.

Plain numpy; no GPU, no product imports."""
import numpy as np

SOL = ("time", "s", "sd", "sdd", "q", "qd", "qdd")
ALL_DOFS = list(range(1, 17)) + [17, 63, 64, 65]
TICK = 2.0 ** -8


def trajectory(rng, time, D):
    """A solution dict around the time stamps time [B][N], and limits small enough that the
    acceleration clamp acts on some joints. numpy's uniform draws are multiples of 2^-52, a grid on
    which sums and differences below 2 never round (a + 1 (b - a) is then b, bit for bit, and a
    lower index one too low on a sample time would go unnoticed); the product of two draws has
    a full mantissa at every magnitude."""
    B, N = time.shape
    draw = lambda *shape: rng.uniform(-1.0, 1.0, shape) * rng.uniform(0.3, 1.0, shape)
    sol = dict(time=np.ascontiguousarray(time, dtype=np.float64))
    for k in ("s", "sd", "sdd"):
        sol[k] = draw(B, N)
    for k in ("q", "qd", "qdd"):
        sol[k] = draw(B, N, D)
    return sol, rng.uniform(0.1, 0.8, (B, D))


def _case(rng, time, D, start, dt, **kw):
    sol, amax = trajectory(rng, time, D)
    return dict(sol=sol, amax=amax, start=np.array(start, dtype=np.float64), dt=dt, **kw)


# ---------------------------------------------------------------------------- uniform
def uniform_dof_case(D):
    """N = 130, B = 4, 4 ms; random time axes with gaps of 1 .. 10 ms starting near 3.0; starts
    before the first sample, at 0.37 of the span, on sample 64 and nextafter above sample 64."""
    B, N = 4, 130
    rng = np.random.default_rng(5000 + D)
    time = 3.0 + np.cumsum(rng.uniform(0.001, 0.01, (B, N)), axis=1)
    span = time[:, -1] - time[:, 0]
    start = [time[0, 0] - 0.0131, time[1, 0] + 0.37 * span[1], time[2, 64], np.nextafter(time[3, 64], np.inf)]
    return _case(rng, time, D, start, 0.004)


def ticks_on_samples_case():
    """Time stamps k 2^-8 and a time step of 2^-8: from sample 0 and from sample 5 every tick is a
    sample time, where the strict comparison of the lower-index search decides; from half a step
    before sample 0 every tick is the middle of a bracket."""
    N = 40
    time = np.tile(np.arange(N) * TICK, (3, 1))
    return _case(np.random.default_rng(5101), time, 3, [time[0, 0], time[1, 5], time[2, 0] - 0.5 * TICK], TICK)


def past_the_end_case():
    """Starts at the last time stamp and 0.5, 1.5 and 10 time steps past it: counts 1, 1, 0 and a
    negative one."""
    N, dt = 50, 0.004
    rng = np.random.default_rng(5102)
    time = np.tile(2.0 + np.cumsum(rng.uniform(0.001, 0.01, N)), (4, 1))
    end = time[0, -1]
    return _case(rng, time, 3, [end, end + 0.5 * dt, end + 1.5 * dt, end + 10.0 * dt], dt)


def tiny_bracket_case():
    """The first two time stamps are 0 and 1e-17, two distinct samples closer than epsilon: the
    starts 0 and 5e-18 interpolate at 0.5 between them; the start 1e-17 is past that bracket."""
    N = 20
    rng = np.random.default_rng(5103)
    row = np.concatenate([[0.0, 1e-17], 1e-17 + np.cumsum(rng.uniform(0.001, 0.01, N - 2))])
    return _case(rng, np.tile(row, (3, 1)), 3, [0.0, 5e-18, 1e-17], 0.004)


def count_case(M, D=3):
    """Two paths whose count is M at a time step of 2^-8. Path 0: (end - start) / step is
    M - 1.5. Path 1: the time stamps are multiples of 2^-12 and the start is exactly M - 1 steps
    before the end, so the quotient is the integer M - 1 and nothing is rounded up."""
    N = 130
    rng = np.random.default_rng(5200 + M)
    gaps = rng.uniform(0.5, 1.5, (2, N))
    time = 1.0 + np.cumsum(gaps / gaps.sum(axis=1, keepdims=True), axis=1) * (0.9 * (M - 1) * TICK)
    time[1] = np.round(time[1] * 4096.0) / 4096.0
    assert (np.diff(time, axis=1) > 0).all()
    return _case(rng, time, D, [time[0, -1] - (M - 1.5) * TICK, time[1, -1] - (M - 1) * TICK], TICK)


def status_case():
    N = 50
    rng = np.random.default_rng(5104)
    time = np.cumsum(rng.uniform(0.001, 0.01, (3, N)), axis=1)
    return _case(rng, time, 3, time[:, 3].copy(), 0.004, status=np.array([0, 4, 0], dtype=np.int32))


def two_samples_case():
    """N = 2: starts before the first sample, inside the only bracket, on the last sample."""
    rng = np.random.default_rng(5105)
    time = np.tile(np.array([0.5, 0.5 + 0.0173]), (3, 1))
    return _case(rng, time, 3, [0.49, 0.5 + 0.006, time[2, 1]], 0.004)


def uniform_edge_cases():
    cases = dict(ticks_on_samples=ticks_on_samples_case(), past_the_end=past_the_end_case(),
                 tiny_bracket=tiny_bracket_case(), status=status_case(), two_samples=two_samples_case())
    for M in (255, 256, 257, 513):
        cases["count_%d" % M] = count_case(M)
    return cases


MAX_OUT_COUNT = 300


def max_outs(count):
    """count, count - 1, and cuts in the same 256-lane block as the count and in an earlier one."""
    return (count, count - 1, 256, 255, 1)


# ---------------------------------------------------------------------------- skip
def skip_dof_case(D):
    """N = 200 with gaps of 1.7 .. 2.7 ms at a 4 ms step: about every second sample is kept, some
    100 from before the first sample and some 80 from sample 40, so one full 64-entry register
    batch and a partial one are flushed."""
    N = 200
    rng = np.random.default_rng(6000 + D)
    time = 1.0 + np.cumsum(rng.uniform(0.0017, 0.0027, (2, N)), axis=1)
    return _case(rng, time, D, [time[0, 0] - 0.01, time[1, 40]], 0.004)


SKIP_MAX_OUTS = (None, 70)       # None: N + 1; 70: a cut inside the second batch


# ---------------------------------------------------------------------------- query
def query_row(N, seed, plateau_first=0, plateau_last=0, rest_ends=True):
    """One consistent profile row: s the solver's linspace, sd random (zero on the first
    1 + plateau_first and the last 1 + plateau_last samples if rest_ends), sd2 = sd * sd, time by
    the trapezoid rule. Returns time, s, sd, sd2 [N]."""
    rng = np.random.default_rng(seed)
    s_start = float(rng.uniform(-1.0, 1.0))
    s_end = s_start + float(rng.uniform(0.5, 2.0))
    ds = (s_end - s_start) / (N - 1)
    s = np.array([ds * i + s_start for i in range(N)])
    s[N - 1] = s_end
    sd = rng.uniform(0.2, 1.5, N)
    if rest_ends:
        sd[:1 + plateau_first] = 0.0
        sd[N - 1 - plateau_last:] = 0.0
    sd2 = sd * sd
    time = np.empty(N)
    time[0] = float(rng.uniform(0.0, 5.0))
    for i in range(1, N):
        if sd2[i - 1] > 0 or sd2[i] > 0:
            time[i] = time[i - 1] + 2.0 * ds / (sd[i - 1] + sd[i])
        else:
            time[i] = time[i - 1]
    return time, s, sd, sd2


HAND_SET = dict(clamp=10, invalid=20, saturate=30, zero_velocity=40)     # branch -> bracket k


def query_hand_set(N, seed):
    """A consistent row of N >= 65 samples with four brackets set by hand, the time stamps kept:
    clamp          sd[k] = 10: sd[k] dt exceeds ds_ over most of the bracket
    invalid        sd2[k] = 50 over sd[k] = 1e-3: the increment is negative, ok = 0
    saturate       clamp, and s[k + 1] half a step lower than the linspace: s[k] + ds_ > s[k + 1]
    zero_velocity  sd = sd2 = 0 at both ends of a bracket of positive length"""
    time, s, sd, sd2 = query_row(N, seed)
    k = HAND_SET["clamp"]
    sd[k] = 10.0; sd2[k] = 100.0
    k = HAND_SET["invalid"]
    sd[k] = 1e-3; sd2[k] = 50.0
    k = HAND_SET["saturate"]
    sd[k] = 10.0; sd2[k] = 100.0
    s[k + 1] = s[k] + 0.5 * (s[k + 1] - s[k])
    k = HAND_SET["zero_velocity"]
    sd[k] = sd[k + 1] = 0.0; sd2[k] = sd2[k + 1] = 0.0
    return time, s, sd, sd2


def query_times(time, first=()):
    """The first and the last time stamp and nextafter on both sides of each, and far outside;
    the middle and 0.9 of the brackets `first`; then every sample time and nextafter on both sides
    of it, and the middle and 0.9 of every bracket."""
    t = [time[0] - 10.0, time[-1] + 10.0]
    for x in (time[0], time[-1]):
        t += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    brackets = lambda ks: [time[k] + f * (time[k + 1] - time[k]) for k in ks for f in (0.5, 0.9)]
    t += brackets(first)
    for x in time:
        t += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    t += brackets(range(len(time) - 1))
    return np.array(t)


SOLVED_FAMILIES = ("stop_first", "stop_last", "stop_interior", "out_and_back")
SOLVED_D, SOLVED_N = 3, 65


def solved_batch():
    """One path of each of SOLVED_FAMILIES (tests/structured_paths.py), 3 joints and 65 samples:
    stop_first and stop_last for the time plateaus at the ends of a solved profile."""
    import structured_paths as sp
    return sp.concat([sp.make_family(name, 1, SOLVED_D, SOLVED_N) for name in SOLVED_FAMILIES])


def oracle_profile(tpo, b, i):
    """The oracle's solved TimeOptimalPathProfile of path i of a joint batch (for Profile.query)."""
    N, D = b["num_samples"], b["control_points"].shape[2]
    _, q1, q2 = tpo.joint_sample_path(b["knots"][i], b["control_points"][i], b["path_start"][i], b["delta"][i], N)
    rows = tpo.joint_constraint_setup(q1, q2, b["vmax"][i], b["amax"][i], b["safety"])
    p = tpo.Profile(N, 2 * D)
    p.set_max_loops(10 * N)
    s_start = b["path_start"][i]
    assert p.setup(*rows, s_start, s_start + b["delta"][i] * (N - 1), b["sd_start"][i], 0.0, b["time_start"][i]) == 0
    assert p.optimize() == 0
    return p


QUERY_SHAPES = [(255, 1), (256, 1), (257, 1), (511, 1), (513, 1), (1, 255), (1, 256), (1, 257),
                (2, 255), (2, 256), (2, 257),
                (4, 257)]          # (B, K): B K on each side of 256 and of 512; (4, 257): every row kind, many queries
QUERY_SAMPLES = (2, 3, 65)


def query_batch(N, B, K):
    """B rows of N samples with K query times each. Row b is, by b % 4: a profile at rest at both
    ends; one with a plateau of 3 samples at the start and 4 at the end; one moving at both ends;
    the hand-set row; the plateaus' and the hand-set brackets come first among the row's query times.
    Below 65 samples there is no room for plateaus or hand-set brackets: the
    rows are then at rest at both ends (N = 3) or moving (b odd, and N = 2, where two samples at
    rest would share one time stamp). The K times of row b are taken from query_times(row) in
    order from an offset that grows with b // 4, so a batch of many rows with one query each
    still reaches every branch."""
    rows, first = [], []
    for b in range(B):
        seed = 7000 + 10 * N + b % 8
        if N >= 65:
            kind = b % 4
            row = (query_row(N, seed), query_row(N, seed, 2, 3), query_row(N, seed, rest_ends=False),
                   query_hand_set(N, seed))[kind]
            first.append(((), (2, N - 5), (), tuple(HAND_SET.values()))[kind])
        else:
            first.append(())
            row = query_row(N, seed, rest_ends=(N > 2 and b % 2 == 0))
        rows.append(row)
    out = {k: np.ascontiguousarray(np.stack([r[i] for r in rows])) for i, k in enumerate(("time", "s", "sd", "sd2"))}
    tq = np.empty((B, K))
    for b in range(B):
        pool = query_times(out["time"][b], first[b])
        tq[b] = pool[(np.arange(K) + b // 4) % len(pool)]
    out["tq"] = tq
    return out

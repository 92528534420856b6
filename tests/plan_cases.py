"""Replan programs for planner sets, shared by test_plan_cases_cpu.py (the oracle alone) and
test_gpu_plan_all_dofs.py (a PlannerSet against the oracle). Deterministic, no GPU.

Program(tpo, kind, D, method, max_iterations) drives B oracle planners (tpo.Planner) through at most
MAX_STEPS Plan calls. Every call is one Step: the planners that were reset and given a new path
before it (what a PlannerSet has to be told), the start and horizon of every planner, and the
oracle's return codes; the oracle planners themselves stay readable until the next step. The next
step's arguments depend on the oracle's own end times (GetNextPlanStartTime clamps to them), so the
program is a generator and its consumer compares in lockstep.

A planner lives through a sequence of "lives". A life begins with a reset and a new path and ends
when a Plan fails (any failed Plan is followed by a reset and a new path: that the reset clears the
planner is part of what is compared) or when the planner has been planned at its end time. The
lives, per planner (LIVES below; generic "run" lives follow until the steps are used up):

  h0 / hneg    horizon 0 / negative on a new path           -> INVALID_ARGUMENT (:313-317)
  modified     kModifiedPath on a planner that never planned -> FAILED_PRECONDITION (:324)
  offtangent   an initial velocity that is refused            -> INVALID_ARGUMENT (:387-392):
               D >= 2: off the start tangent by 0.1 along a direction orthogonal to it (the largest
               component of a unit vector is >= 1/sqrt(D) = 0.25, so the error is >= 0.025, above
               max_initial_velocity_error = 0.01); D = 1: against the tangent (the projection clamps
               to zero, the error is the velocity itself)
  toofast      an initial velocity along the start tangent at three times what the joint velocity
               limits allow: the projection accepts it and so does the oracle's solver
  nospeed      a zero velocity limit on the middle joint: the solver's set-up fails -> INTERNAL
               (:394-417); a Plan at the end time often gives INTERNAL too, but not by construction
  whole        the whole path inside one window: target reached after the first Plan, then a Plan
               exactly at the end time (INTERNAL or OK, as the oracle says)
  run          a new path (2..5 waypoints / an IK table spanning 2..10 windows), first Plan on or off
               the time-step grid, then replans at min(end_time, start + increment) with horizons
               cycling short / medium / long until the planner has been planned at its end time.
               Options: tangent (an accepted initial velocity along the start tangent, taken from the
               oracle's own first-derivative sample: non-zero sd_start), same_start (a replan at the
               first Plan's start, which is the first history stamp: lower_bound gives index 0 and
               the offset clamps from -1 to 0), and one way to end early:
                 before   a start before the last Plan's start         -> INVALID_ARGUMENT (:527)
                 gap      end_time < start <= end_time + time step     -> INVALID_ARGUMENT (:523)
                 beyond   start > end_time + time step                 -> OUT_OF_RANGE (:508)
DEADLINE_EXCEEDED needs max_planning_iterations, which a set has once for all its planners: the
same program run with max_iterations = 1 fails every Plan that needs a second window, with
windows == 2 (the long horizons need three).

Two edges one could ask for cannot occur, in the reference or here, and are not in the program:
  * INVALID_ARGUMENT from a second (or later) window's non-positive duration. The loop goes on only
    while t[N-1] - start <= horizon, and the next window starts at TimeFromSec(t[decel_start]) with
    decel_start <= N - 2 (last_extremal_index stops at N - 2), so the next duration start + horizon -
    loop_start is at least t[N-1] - t[N-2]. That is positive unless the stamp repeats, which the
    solver does only where sd2 is zero at both ends of an interval (tp_oracle.c:967-968): the window
    ends at rest, so it would also have to stand still at sample N - 2, and then back to decel_start,
    which no path with a non-zero tangent and non-zero limits does (the nospeed life, which has a
    zero limit, fails in the solver's set-up before any window exists).
  * a window start after the last history stamp. Plan drops the trajectory behind the start first
    (GetTimeOffsetAfter) and refuses a start at or behind its last sample with INTERNAL, and the
    trajectory never reaches past the history it was resampled from; so lower_bound - 1 never
    exceeds the last index and the upper clamp of the window offset is never taken.
Of the starts at history stamps only the one equal to the first stamp is constructed (same_start).
A start before the first stamp is a start before the first Plan's start and therefore before the
last Plan's: the refusal of `before` (start < start_time), long before the history is searched. A
start equal to an interior stamp is not constructed: stamps are sums of doubles, and one that
equals a whole number of nanoseconds divided by 1e9 does not occur by choice.
"""
import collections
import importlib

import numpy as np

from conftest import PKG_NAME

MS = 1_000_000
TIME_STEP_NS = 4 * MS
B = 12
WINDOW_SIZES = (33, 64, 65)
MAX_STEPS = 80
DEADLINE_STEPS = 16              # steps of the run with max_planning_iterations = 1
MAX_INITIAL_VELOCITY_ERROR = 1e-2
SAFETY = 0.8
TIGHT_TRAJECTORY = 64           # trajectory capacity of the tight set; its history capacity is 2 N
KINDS = ("joint", "cartesian")
ALL_DOFS = tuple(range(1, 17))

# horizons (short: erase-only once something is planned; long: three or more windows) and start
# increments (on the grid, off it, and a longer one so that paths finish within the steps)
HORIZONS_MS = {"joint": (60, 400, 1500), "cartesian": (300, 2000, 8000)}
INCREMENTS_NS = {"joint": (52 * MS, 36 * MS + 777, 148 * MS), "cartesian": (200 * MS, 136 * MS + 777, 600 * MS)}

LIVES = (
    ("h0", "run:before", "toofast", "nospeed"),
    ("hneg", "run:same_start", "run:gap"),
    ("modified", "run:tangent:beyond", "run"),
    ("offtangent", "run", "run:before"),
    ("whole", "nospeed", "toofast", "run:same_start"),
    ("run:tangent", "h0", "run:gap"),
    ("run", "hneg", "run:beyond"),
    ("run:same_start", "modified", "toofast", "nospeed"),
    ("whole", "run:tangent", "offtangent"),
    ("run:gap", "run", "whole"),
    ("run:beyond", "run:tangent:same_start", "run"),
    ("run:before", "whole", "run"),
)
assert len(LIVES) == B

# the edges and the statuses the oracle may answer them with (a Plan at the end time: OK, or INTERNAL
# "nothing to resample", or INVALID_ARGUMENT where the clamped end time lies 1 ns before the last start)
EDGE_STATUS = {"h0": (3,), "hneg": (3,), "modified": (1,), "offtangent": (3,), "toofast": (0,), "nospeed": (4,), "tangent": (0,), "whole": (0,),
               "at_end": (0, 3, 4), "same_start": (0,), "before": (3,), "gap": (3,), "beyond": (2,)}


def window_samples(D, method):
    """N in turn from WINDOW_SIZES across (D, method): 64 and 65 both occur among the joint counts
    with their own kernels (3..8, 14) and among the generic ones."""
    return WINDOW_SIZES[(2 * (D - 1) + method) % 3]


class Step:
    """One Plan call of the program: `new_paths` {planner: path dict} (reset, then this path, before
    the call), start / horizon [B] int64, rc [B] the oracle's return codes, lives [B] the name of
    the life each planner is in, edges [B] the edge this call is for that planner (a key of
    EDGE_STATUS, or ""), oracle [B] the planners after the call."""

    def __init__(self, index, new_paths, start, horizon, rc, lives, edges, oracle):
        self.index, self.new_paths, self.start, self.horizon = index, new_paths, start, horizon
        self.rc, self.lives, self.edges, self.oracle = rc, lives, edges, oracle


class _Life:
    def __init__(self, name, path, first_start):
        parts = name.split(":")
        self.name, self.kind, self.options = name, parts[0], set(parts[1:])
        self.path = path
        self.first_start = first_start
        self.plans = 0                # Plans of this life so far
        self.last_start = None
        self.at_end = False           # the last Plan's start was the end time


class Program:
    def __init__(self, tpo, kind, D, method, max_iterations=200, max_steps=MAX_STEPS):
        assert kind in KINDS
        self.tpo, self.kind, self.D, self.method = tpo, kind, int(D), int(method)
        self.N = window_samples(D, method)
        self.max_iterations, self.max_steps = int(max_iterations), int(max_steps)
        self.syn = importlib.import_module(PKG_NAME + ".synthetic")
        self.serial = 0
        self.requested = set()        # planners a consumer wants reset (force_reset)
        self.horizons = [h * MS for h in HORIZONS_MS[kind]]
        self.increments = INCREMENTS_NS[kind]

    # ------------------------------------------------------------------ paths
    def _rng(self):
        self.serial += 1
        return np.random.default_rng([KINDS.index(self.kind), self.D, self.method, self.serial])

    def _path(self, b, whole):
        """A new path for planner b; `whole`: it fits one window."""
        D, N, tpo = self.D, self.N, self.tpo
        rng = self._rng()
        spans = 1.0 if whole else 2.0 + 1.5 * ((b + self.serial) % 6)      # windows the path spans
        vmax, amax = rng.uniform(1.0, 2.0, D), rng.uniform(2.0, 4.0, D)
        path = dict(kind=self.kind, vmax=vmax, amax=amax, initial_velocity=np.zeros(D), state=1)
        if self.kind == "joint":
            W = 2 + (b + self.serial) % 4
            cps, knots = tpo.joint_fit_spline(rng.uniform(-0.8, 0.8, (W, D)), 0.2)
            # just short of the end: close to it (kSmall 1e-4), and no sample past the last knot
            length = knots[-1] - 5e-5 if whole else knots[-1]
            path.update(knots=knots, control_points=cps, delta=float(length / (N - 1) / spans))
            path["tangent"] = tpo.joint_sample_path(knots, cps, 0.0, path["delta"], N)[1][0]
        else:
            rows = N + int(round((N - 1) * spans))
            batch = self.syn.make_cartesian_batch(1, D, rows, 2 + (b + self.serial) % 3,
                                                  first_path_index=1000 * self.D + 100 * self.method + self.serial)
            delta = float(batch["delta"][0])
            path.update(ik_positions=batch["ik_positions"][0], jacobians=batch["jacobians"][0], delta=delta,
                        path_end=delta * (rows - N), vtrans=float(batch["vtrans"][0]), vrot=float(batch["vrot"][0]),
                        vmax=batch["vmax"][0], amax=batch["amax"][0])
            path["tangent"] = tpo.cartesian_path_derivatives(path["ik_positions"][:N], delta)[0][0]
        return path

    def _velocity(self, path, accepted, scale=0.1):
        """An initial velocity along the start tangent (`scale` times what the joint limits allow),
        or one the projection must refuse."""
        t, D = path["tangent"], self.D
        along = scale * np.min(path["vmax"] / np.maximum(np.abs(t), 1e-12)) * t
        if accepted:
            return along
        if D == 1:
            return -0.1 * np.sign(t)
        e = np.zeros(D)
        e[int(np.argmin(np.abs(t)))] = 1.0
        n = e - t * (e @ t) / (t @ t)
        return along + 0.1 * n / np.linalg.norm(n)

    def make_oracle(self, path):
        o = self.tpo.Planner(self.D, self.N, delta=path["delta"], safety=SAFETY, time_step_ns=TIME_STEP_NS,
                             skip=bool(self.method), max_planning_iterations=self.max_iterations,
                             max_initial_velocity_error=MAX_INITIAL_VELOCITY_ERROR)
        o.set_limits(path["vmax"], path["amax"])
        if path["kind"] == "joint":
            o.set_spline(path["knots"], path["control_points"], path["state"])
        else:
            o.set_ik_table(path["ik_positions"], path["jacobians"], path["path_end"], path["vtrans"], path["vrot"],
                           path["state"])
        o.set_initial_velocity(path["initial_velocity"])
        return o

    # ------------------------------------------------------------------ lives
    def _new_life(self, b, count, clock):
        names = LIVES[b]
        name = names[count] if count < len(names) else "run"
        kind = name.split(":")[0]
        path = self._path(b, whole=(kind == "whole"))
        if kind == "modified":
            path["state"] = 2
        if kind == "offtangent":
            path["initial_velocity"] = self._velocity(path, accepted=False)
        if kind == "nospeed":
            path["vmax"] = np.array(path["vmax"])
            path["vmax"][self.D // 2] = 0.0
        if kind == "toofast":
            path["initial_velocity"] = self._velocity(path, accepted=True, scale=3.0)
        if "tangent" in name.split(":")[1:]:
            path["initial_velocity"] = self._velocity(path, accepted=True)
        # first Plans alternate between the time-step grid and 1.000333 ms off it
        first = clock + 100 * MS + (1_000_333 if (b + count) % 2 else 0)
        return _Life(name, path, first)

    def _arguments(self, life, o, k):
        """(start, horizon, edge) of the life's next Plan."""
        hz = self.horizons
        if life.plans == 0:
            horizon = {"h0": 0, "hneg": -5 * MS, "whole": hz[2]}.get(life.kind, hz[(k + 1) % 3])
            if "same_start" in life.options:
                horizon = hz[0]       # one window: the replan at the same start has windows left to plan
            edge = life.kind if life.kind != "run" else ("tangent" if "tangent" in life.options else "")
            return life.first_start, horizon, edge
        end, last = o.end_time, life.last_start
        if life.kind == "whole":
            return end, hz[1], "at_end"
        if "same_start" in life.options and life.plans == 1:
            # at the first history stamp; a horizon past everything planned so far, so that windows run
            return life.first_start, max(o.final_decel_start - last, 0) + hz[2], "same_start"
        start = min(end, last + self.increments[k % 3])
        # the way this life ends early, if it has one: at its ninth / twelfth replan, or when the
        # planner would otherwise be planned at its end time
        if (life.plans >= 9 or start == end) and "before" in life.options:
            return last - MS, hz[1], "before"
        if (life.plans >= 12 or start == end) and "gap" in life.options:
            return end + 1, hz[1], "gap"
        if (life.plans >= 12 or start == end) and "beyond" in life.options:
            return end + TIME_STEP_NS + 1, hz[1], "beyond"
        return start, hz[k % 3], ("at_end" if start == end else "")

    def force_reset(self, b):
        """The consumer lost planner b (a set's planner ran out of room): its current life ends, the
        next step resets it and gives it a new path, in the oracle as well."""
        self.requested.add(int(b))

    def steps(self):
        lives, counts, oracle = [None] * B, [0] * B, [None] * B
        clock = [900 * MS + 12 * MS * b for b in range(B)]
        for k in range(self.max_steps):
            new_paths, edges = {}, []
            start, horizon = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64)
            for b in range(B):
                if lives[b] is None or b in self.requested:
                    lives[b] = self._new_life(b, counts[b], clock[b])
                    counts[b] += 1
                    oracle[b] = self.make_oracle(lives[b].path)
                    new_paths[b] = lives[b].path
                start[b], horizon[b], edge = self._arguments(lives[b], oracle[b], k + b)
                edges.append(edge)
            self.requested.clear()
            rc = np.array([oracle[b].plan(int(start[b]), int(horizon[b])) for b in range(B)], dtype=np.int32)
            names = [lives[b].name for b in range(B)]
            for b in range(B):
                life = lives[b]
                life.at_end = edges[b] == "at_end"
                life.plans += 1
                life.last_start = int(start[b])
                clock[b] = max(clock[b], int(start[b]))
            yield Step(k, new_paths, start, horizon, rc, names, edges, list(oracle))
            for b in range(B):
                if rc[b] != 0 or lives[b].at_end:
                    lives[b] = None


# ---------------------------------------------------------------- invariants of one trajectory
def check_invariants(time, s, qdd, amax, path_end, kind, method, where):
    """What holds for every trajectory of a successful Plan, whoever computed it."""
    assert (np.diff(time) > 0).all(), (where, "time stamps strictly increasing")
    assert (np.abs(qdd) <= amax[None, :]).all(), (where, "|qdd| <= amax")
    # end_time and final_decel_start as exact time-step multiples: not kept by the oracle (TimeFromSec
    # truncates multiple * time_step_sec: 4219999999 ns occurs), so left out
    assert (np.diff(s) >= 0).all() and (s <= path_end).all(), (where, "s non-decreasing, at most the last window's end")
    # s >= 0: not kept by the oracle for joint paths with skip sampling (EraseTrajectoryBefore starts
    # InterpolateAtTime's search at a trajectory index and can extrapolate the first sample below 0)
    if not (kind == "joint" and method == 1):
        assert (s >= 0).all(), (where, "s >= 0")


def path_end_of(path, N):
    """The largest path parameter a trajectory of this path can hold. Not the end of the path: the
    oracle, as the reference, lets the last window run its full N - 1 steps, past the last knot (or
    knots.back() of a Cartesian path, whose table holds those rows), so that is the bound: a window
    starts before the end of the path."""
    end = float(path["knots"][-1]) if path["kind"] == "joint" else float(path["path_end"])
    return end + path["delta"] * (N - 1)


class Stats:
    """What one run of a program contained, counted from the oracle's side of every step."""

    def __init__(self, N):
        self.N = N
        self.ok = self.multi_window = self.max_history = self.max_samples = 0
        self.windows, self.status, self.edges = (collections.Counter() for _ in range(3))
        self.reached = set()

    def add(self, step, planners=range(B)):
        for b in planners:
            o, rc = step.oracle[b], int(step.rc[b])
            self.status[rc] += 1
            if step.edges[b]:
                self.edges[(step.edges[b], rc)] += 1
            self.max_history = max(self.max_history, o.history_count)      # a failed Plan leaves its windows too
            if rc != 0:
                continue
            self.ok += 1
            self.windows[min(o.windows, 3)] += 1
            self.multi_window += o.windows >= 2
            self.max_samples = max(self.max_samples, o.num_samples)
            if o.target_reached:
                self.reached.add(b)

    def line(self):
        return "ok %d multi-window %d windows %s status %s reached %d max history %d (%.1f N) max samples %d" % (
            self.ok, self.multi_window, dict(sorted(self.windows.items())), dict(sorted(self.status.items())),
            len(self.reached), self.max_history, self.max_history / self.N, self.max_samples)

"""The numpy / oracle statement of the refined batch calls (include/tpamd.h
tpamd_time_joint_paths_refined_*): solve every path with the CPU oracle, check it with
check_reference.check_rows, give the paths that need refinement slots in ascending path order, and
solve a slot's path again with n -> 2 n - 1 samples and delta -> delta / 2 until it is clean, the
rounds are used up or the next grid does not fit. Nothing here reads the engine.

refine_joint_batch returns a dict:
  round0        per path, the solve at the caller's grid: dict(n, delta, status, record, sd2, sdd, rows)
  slot          [B] int32: slot, -1 nothing to refine, -2 no slot left, -3 too long
  slot_path     [M] int32: path of a slot, -1 unused
  num_refined   int
  rounds, num_samples [M] int32 and delta [M]: solves made in a slot and the grid of its last one
                (0 for an unused slot)
  history       per slot, the list of the solves made in it (dicts as in round0), [] for an unused one
  final         per slot, history[-1], or None
  refined_check per slot, the record of its last solve (NOT_CHECKED for an unused slot)
"""
import numpy as np

import check_reference as cr

NOTHING, NO_SLOT, TOO_LONG = -1, -2, -3


def needs_refinement(record, tolerance):
    """violations > 0 and worst_excess > tolerance; false for a record that was not checked."""
    return bool(record[0] > 0 and record[1] > tolerance)


def solve_path(tpo, batch, b, n, delta, stride=None):
    """The oracle's solve and check of path b at n samples of spacing delta. A count outside
    [2, stride] fails the path as the engine's set-up does (6) and it is not checked."""
    n, delta = int(n), float(delta)
    if batch["knots"][b] is None:                  # a waypoint batch's path without waypoints
        return dict(n=n, delta=delta, status=11, record=cr.NOT_CHECKED, sd2=None, sdd=None, rows=None)
    if n < 2 or (stride is not None and n > stride):
        return dict(n=n, delta=delta, status=6, record=cr.NOT_CHECKED, sd2=None, sdd=None, rows=None)
    rows = cr.joint_rows(tpo, batch, b, n, delta=delta)
    s0 = float(batch["path_start"][b])
    rc, p = cr.oracle_profile(tpo, rows, s0, s0 + delta * (n - 1), batch["sd_start"][b], batch["time_start"][b])
    rec = cr.check_rows(*rows, p.sd2, p.sdd) if rc == 0 else cr.NOT_CHECKED
    return dict(n=n, delta=delta, status=int(rc), record=rec, sd2=p.sd2, sdd=p.sdd, rows=rows)


def slot_map(records, counts, max_samples, max_refined, tolerance):
    """slot [B], slot_path [M] and the number of used slots from round 0's records."""
    B = len(records)
    slot = np.full(B, NOTHING, dtype=np.int32)
    slot_path = np.full(max_refined, -1, dtype=np.int32)
    rank = 0
    for b in range(B):
        if not needs_refinement(records[b], tolerance):
            continue
        if 2 * int(counts[b]) - 1 > max_samples:
            slot[b] = TOO_LONG
            continue
        if rank < max_refined:
            slot[b] = rank
            slot_path[rank] = b
        else:
            slot[b] = NO_SLOT
        rank += 1
    return slot, slot_path, min(rank, max_refined)


def refine_joint_batch(tpo, batch, max_rounds, max_samples, max_refined, tolerance=0.0, counts=None, stride=None,
                       round0=None):
    """`batch`: a dict as synthetic.make_joint_batch returns (knots, control_points, vmax, amax,
    path_start, delta, sd_start, time_start, safety). counts: per-path sample counts (None: stride each;
    stride None: batch["num_samples"]). round0: the result of an earlier call on the same batch and
    grid, to share its solves."""
    B = len(batch["control_points"])
    N = int(batch["num_samples"] if stride is None else stride)
    counts = np.full(B, N, dtype=np.int64) if counts is None else np.asarray(counts, dtype=np.int64)
    if round0 is None:
        round0 = [solve_path(tpo, batch, b, counts[b], batch["delta"][b], N) for b in range(B)]
    slot, slot_path, used = slot_map([r["record"] for r in round0], counts, max_samples, max_refined, tolerance)
    M = max_refined
    rounds = np.zeros(M, dtype=np.int32)
    num_samples = np.zeros(M, dtype=np.int32)
    delta = np.zeros(M)
    history = [[] for _ in range(M)]
    for k in range(used):
        b = int(slot_path[k])
        n, dl = int(counts[b]), float(batch["delta"][b])
        r = 0
        while True:
            r += 1
            n, dl = 2 * n - 1, dl / 2.0
            made = solve_path(tpo, batch, b, n, dl)
            history[k].append(made)
            if not (needs_refinement(made["record"], tolerance) and r < max_rounds and 2 * n - 1 <= max_samples):
                break
        rounds[k], num_samples[k], delta[k] = r, n, dl
    final = [h[-1] if h else None for h in history]
    return dict(round0=round0, slot=slot, slot_path=slot_path, num_refined=used, rounds=rounds,
                num_samples=num_samples, delta=delta, history=history, final=final,
                refined_check=[f["record"] if f else cr.NOT_CHECKED for f in final])

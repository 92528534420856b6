"""The buffer-set row kernels (k_bset_insert with its compaction, k_bset_discard, k_bset_add_offset,
k_bset_clear, k_bset_info, k_bset_regrow) and the bulk readout kernels (k_pset_sample_at_ticks,
k_pset_scan_offsets, k_pset_pack_trajectories, k_stop_scan_offsets) at every joint count D = 1..16
and every structural edge, against tests/buffer_reference.py: a restatement of TrajectoryBuffer
written from the reference's sources and held to the mirror and the kernels' host-compilable cores
on the CPU (tests/test_buffer_reference_cpu.py), and exact rational checkers on the GPU's own
values. Every comparison is bit for bit; every output array is pre-filled with a sentinel and what
a call must not write keeps it; the _device entries (CUDA tensors) and the host-pointer entries
(ctypes) are both driven.

  layout        one buffer per (kept rows K, first row) with K D just below, at and just above
                256 and 512 doubles (the copy chunk) and shifts of one row, under a chunk, a chunk
                and more, and beyond K rows: the insert / append that fits only through compaction,
                the one a row longer (TPAMD_PLAN_MORE, nothing changes), and through the host
                entries the growth of a set whose buffers start behind row 0
  programs      48 buffers, 33 rounds of insert / append / discard / add_offset / clear with ids a
                shuffled subset or NULL, in a set exactly as large as the reference's largest count;
                differences exactly equal to the tolerance and one ulp beside it; repeated stamps
  ticks         37 x 7 and 32 x 8 ticks on the buffers the programs leave: on and 1 ns beside the
                end stamps, far outside, empty buffers, repeated and bad ids, int64 overflow
  packs, scans  id lists of 0, 1, 1023, 1024, 1025, 2049 and 2500 entries (the scans have 1024
                threads), capacity equal to the total, one more and one less; the same on a planner
                set's trajectories, ticks and stopping trajectories; insert_from with permuted planners

Every name of buffer_reference.OUTCOMES must occur for every D on the GPU's own results."""
import collections
import ctypes as C
import importlib
import time

import numpy as np
import pytest

from conftest import PKG_NAME
import buffer_reference as br
import stop_reference as sr

pytestmark = pytest.mark.gpu

ALL_DOFS = list(range(1, 17))
SCAN_DOFS = [1, 7, 16]
MS = 1_000_000
_T0 = time.time()
_OUTCOMES = collections.defaultdict(collections.Counter)
_LEFT, _STATS = {}, {}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    yield dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), lib=eng.load_library())
    for _, backend in _LEFT.values():
        backend.close()
    _LEFT.clear()


class GpuBackend:
    """A buffer set behind the interface of buffer_reference.run_program / compare_ticks /
    compare_pack: through the _device entries with CUDA tensors, or (`host`) through the
    host-pointer entries with numpy arrays. Every output starts as a sentinel."""

    def __init__(self, env, program, host):
        self.env, self.host, self.lib = env, host, env["lib"]
        self.B, self.D = program["B"], program["D"]
        self.bs = env["eng"].BufferSet(env["E"], self.B, self.D, capacity=program["capacity"],
                                       timestep_tolerance=program["tolerance"])
        assert self.capacity() == program["capacity"]

    def close(self):
        self.bs.close()

    def capacity(self):
        return self.bs.capacity

    # numpy in, the entry's kind of array out, and back
    def _arr(self, a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        return a if self.host else self.env["torch"].from_numpy(a).to(self.env["dev"])

    def _p(self, a):
        if a is None or (a.size if self.host else a.numel()) == 0:
            return None
        return a.ctypes.data if self.host else a.data_ptr()

    def _back(self, a):
        return a if self.host or a is None else a.cpu().numpy()

    def _ids(self, ids):
        return None if ids is None else self._arr(np.asarray(ids, dtype=np.int32))

    def _call(self, name, *args):
        f = getattr(self.lib, "tpamd_buffer_set_" + name + ("" if self.host else "_device"))
        rc = f(self.bs._handle(), *args) if self.host else f(self.bs._handle(), *args, None)
        if not self.host:
            self.env["torch"].cuda.synchronize()
        return rc

    def apply(self, rnd):
        n, kind = len(rnd["entries"]), rnd["kind"]
        a = {k: self._arr(v) for k, v in br.pack_entries(rnd, self.D).items()}
        ids = self._ids(rnd["ids"])
        status = self._arr(np.full(n, -77, dtype=np.int32))
        p = self._p
        if kind == "insert":
            rows = (a["time"].shape[0],) if not self.host else ()
            rc = self._call("insert", n, p(ids), p(a["offsets"]), *rows, p(a["time"]), p(a["q"]), p(a["qd"]), p(a["qdd"]),
                            p(status))
        elif kind == "append":
            rc = self._call("append_sample", n, p(ids), p(a["time"]), p(a["q"]), p(a["qd"]), p(a["qdd"]), p(status))
        elif kind == "clear":
            rc = self._call("clear", n, p(ids), *(() if self.host else (p(status),)))
        else:
            rc = self._call("discard_before" if kind == "discard" else "add_offset", n, p(ids), p(a.get("ns")), p(a.get("sec")),
                            *(() if self.host else (p(status),)))
        assert rc == 0, (kind, rc)
        if self.host and kind not in ("insert", "append"):
            return [br.OK] * n                               # these host entries report through rc alone
        return [int(x) for x in self._back(status)]

    def download(self, ids=None, capacity=None):
        count = self.B if ids is None else len(ids)
        rows = self.B * self.capacity() if capacity is None else capacity
        off = self._arr(np.full(count + 1, -77, dtype=np.int64))
        out = {k: self._arr(np.full(rows * w, br.SENTINEL)) for k, w in (("t", 1), ("q", self.D), ("qd", self.D), ("qdd", self.D))}
        idt = self._ids(ids)
        p = self._p
        rc = self._call("download", count, p(idt), p(off), rows, p(out["t"]), p(out["q"]), p(out["qd"]), p(out["qdd"]))
        off = [int(x) for x in self._back(off)]
        # the host entry reports a total beyond the capacity through rc, the device entry cannot
        assert (rc != 0) == (self.host and off[-1] > rows), (rc, off[-1], rows)
        out = {k: self._back(v) for k, v in out.items()}
        out["offsets"] = off
        if capacity is None:
            total = off[-1]
            for k, w in (("t", 1), ("q", self.D), ("qd", self.D), ("qdd", self.D)):
                assert br._all_sentinel(out[k][total * w:]), ("nothing behind the packed rows is written", k)
                out[k] = out[k][:total * w]
        return out

    def info(self, ids, time_ns):
        n = len(time_ns)
        out = {k: self._arr(np.full(n, -77, dtype=dt)) for k, dt in
               (("count", np.int32), ("seq", np.int32), ("start_ns", np.int64), ("end_ns", np.int64), ("up_to", np.int32))}
        times, idt = self._arr(np.asarray(time_ns, dtype=np.int64)), self._ids(ids)
        p = self._p
        rc = self._call("info", n, p(idt), p(times), *[p(out[k]) for k in ("count", "seq", "start_ns", "end_ns", "up_to")])
        assert rc == 0
        return {k: [int(x) for x in self._back(v)] for k, v in out.items()}

    def ticks(self, ids, start_ns, step_ns, T, want=(True, True, True)):
        n = len(start_ns)
        out = {k: self._arr(np.full(n * T * self.D, br.SENTINEL)) if w else None for k, w in zip(br.ARRAYS, want)}
        status = self._arr(np.full(n * T, -77, dtype=np.int32))
        starts, idt = self._arr(np.asarray(start_ns, dtype=np.int64)), self._ids(ids)
        p = self._p
        rc = self._call("sample_at_ticks", n, p(idt), p(starts), step_ns, T, p(out["q"]), p(out["qd"]), p(out["qdd"]), p(status))
        assert rc == 0
        res = {k: self._back(v) for k, v in out.items()}
        res["status"] = [int(x) for x in self._back(status)]
        return res


def _left(env, D, host):
    """The buffers the operation program of D joints leaves (reference set and backend), run by
    test_operation_programs or here."""
    if (D, host) not in _LEFT:
        program = br.operation_program(D)
        backend = GpuBackend(env, program, host)
        seen, stats = collections.Counter(), collections.Counter()
        ref = br.run_program(backend, program, seen, stats)
        _LEFT[(D, host)] = (ref, backend)
        _STATS[(D, host)] = (seen, stats)
    return _LEFT[(D, host)]


def _missing(seen, names):
    return [k for k in names if not seen[k]]


# ------------------------------------------------------------------ 3a: layout and compaction
@pytest.mark.parametrize("D", ALL_DOFS)
def test_layout_and_compaction(env, D):
    cases = br.layout_cases(D)
    program = br.layout_program(D)
    seen, stats = collections.Counter(), collections.Counter()
    backend = GpuBackend(env, program, host=False)
    try:
        br.run_program(backend, program, seen, stats)        # asserts every planned case a compaction
    finally:
        backend.close()
    assert stats["compactions"] == 2 * len(cases), (D, stats)
    assert stats["more"] == len(cases) + sum(1 for K, f in cases if f == 1), (D, stats)
    assert _missing(seen, br.LAYOUT_OUTCOMES) == [], D
    # the host entries: the exact fit compacts, the insert one row longer grows a set whose
    # buffers start behind row 0 (bset_make_room, k_bset_regrow)
    program = br.layout_program(D, host=True)
    hstats = collections.Counter()
    backend = GpuBackend(env, program, host=True)
    try:
        br.run_program(backend, program, seen, hstats)
        assert backend.capacity() == 2 * program["capacity"], (D, backend.capacity())
    finally:
        backend.close()
    assert hstats["compactions"] == len(cases) and hstats["more"] == 0, (D, hstats)
    _OUTCOMES[D].update(seen)


# ------------------------------------------------------------------ 3b: operation programs
@pytest.mark.parametrize("D", ALL_DOFS)
def test_operation_programs(env, D):
    for host in (False, True):
        ref, backend = _left(env, D, host)
        seen, stats = _STATS[(D, host)]
        # The device set is exactly as large as the reference's largest count: tight fits and
        # compactions occur, MORE never. The host entries make room for count + segment rows before
        # they know the kept count, so that set may have grown; its results are the same.
        assert stats["more"] == 0, (D, host, stats)
        if not host:
            assert stats["compactions"] > 0 and stats["tight_fits"] > 0, (D, stats)
            assert backend.capacity() == br.operation_program(D)["capacity"]
        assert _missing(seen, br.PROGRAM_OUTCOMES) == [], (D, host)
        if not host:
            _OUTCOMES[D].update(seen)


@pytest.mark.parametrize("D", ALL_DOFS)
def test_exact_tolerance_and_repeated_stamps(env, D):
    seen = collections.Counter()
    for host in (False, True):
        program = br.tolerance_program(D)
        backend = GpuBackend(env, program, host)
        try:
            br.run_program(backend, program, seen)
        finally:
            backend.close()
    assert _missing(seen, ("insert_kept_one_less", "insert_kept_0_no_replace", "discard_close_before", "discard_on_sample",
                           "discard_interpolated")) == [], D
    program = br.operation_program(D, True)
    stats = collections.Counter()
    backend = GpuBackend(env, program, host=False)
    try:
        ref = br.run_program(backend, program, seen, stats)
        assert stats["more"] == 0 and stats["compactions"] > 0, (D, stats)
        ids, starts = br.repeated_stamp_ticks(ref.buffers)
        assert len(ids) > 0, D
        br.compare_ticks(ref, backend, ids, starts, 1, 3, seen=seen, where=(D, "repeated stamps"))
    finally:
        backend.close()


# ------------------------------------------------------------------ 3c: setpoint ticks
@pytest.mark.parametrize("D", ALL_DOFS)
def test_setpoint_ticks(env, D):
    seen = collections.Counter()
    for host in (False, True):
        ref, backend = _left(env, D, host)
        # the host entries check every id before the first copy: bad ids go through the device entries
        br.run_ticks(ref, backend, np.random.default_rng(D), seen if not host else None, bad_ids=not host,
                     null_arrays=True, where=(D, "host" if host else "device"))
    assert _missing(seen, br.TICK_OUTCOMES) == [], D
    _OUTCOMES[D].update(seen)


# ------------------------------------------------------------------ 3d: packed download and the scans
@pytest.mark.parametrize("D", SCAN_DOFS)
def test_packed_download_long_lists(env, D):
    for host in (False, True):
        ref, backend = _left(env, D, host)
        br.run_packs(ref, backend, np.random.default_rng(D), bad_ids=not host, where=(D, "host" if host else "device"))


def _planned_set(env, D, B=24, N=64):
    """24 planners of D joints planned once from waypoints; returns the set (open) and per planner
    its trajectory downloaded alone (tpamd_planner_set_download_trajectory): dict of numpy rows."""
    torch, eng, E, dev, lib = env["torch"], env["eng"], env["E"], env["dev"], env["lib"]
    rng = np.random.default_rng(20261020 + D)
    W = rng.integers(3, 7, size=B)
    offsets = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    wps = rng.uniform(-2.0, 2.0, size=(int(offsets[-1]), D))
    vmax, amax = rng.uniform(1.0, 2.0, size=(B, D)), rng.uniform(2.0, 4.0, size=(B, D))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ps = eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=4 * MS)
    status, _ = ps.set_waypoints(up(wps), offsets, up(vmax), up(amax), up(rng.uniform(0.01, 0.03, size=B)))
    assert (status.cpu().numpy() == 0).all()
    summary = ps.plan(1000 * MS, 400 * MS)
    counts = summary["num_samples"].numpy()
    assert (summary["status"].numpy() == 0).all() and (counts > 2).all()
    rows = []
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for b in range(B):
        n = int(counts[b])
        r = dict(time=np.zeros(n), s=np.zeros(n), sd=np.zeros(n), sdd=np.zeros(n), q=np.zeros((n, D)), qd=np.zeros((n, D)),
                 qdd=np.zeros((n, D)))
        assert lib.tpamd_planner_set_download_trajectory(ps._handle(), b, 0, n, *[p(r[k]) for k in
                                                         ("time", "s", "sd", "sdd", "q", "qd", "qdd")]) == 0
        rows.append(r)
    return ps, rows, amax


def _as_buffers(rows, D):
    """The planners' trajectories as reference buffers (for ticks and for insert_from)."""
    ref = br.ReferenceSet(len(rows), D)
    for buf, r in zip(ref.buffers, rows):
        buf.insert_segment(r["time"].tolist(), r["q"].tolist(), r["qd"].tolist(), r["qdd"].tolist())
    return ref


@pytest.mark.parametrize("D", SCAN_DOFS)
def test_planner_set_readouts_long_lists(env, D):
    """tpamd_planner_set_download_trajectories* (s, sd, sdd included) and
    tpamd_planner_set_sample_at_ticks* over long id lists against the single-planner downloads."""
    torch, dev, lib = env["torch"], env["dev"], env["lib"]
    ps, rows, _ = _planned_set(env, D)
    B = len(rows)
    keys = ("time", "s", "sd", "sdd", "q", "qd", "qdd")
    width = lambda k: D if k in br.ARRAYS else 1
    rng = np.random.default_rng(D)
    ref = _as_buffers(rows, D)
    try:
        for host in (False, True):
            for n in br.PACK_LENGTHS:
                ids = np.asarray(br.id_list(rng, n, B, bad=not host), dtype=np.int32)
                counts = [len(rows[b]["time"]) if 0 <= b < B else 0 for b in ids]
                want_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
                total = int(want_off[-1])
                want = {k: b"".join(rows[b][k].tobytes() for b in ids if 0 <= b < B) for k in keys}
                for cap in sorted({total, total + 1, max(total - 1, 0)}):
                    off = np.full(n + 1, -77, dtype=np.int64)
                    out = {k: np.full(cap * width(k), br.SENTINEL) for k in keys}
                    if host:
                        hp = lambda a: a.ctypes.data_as(C.c_void_p) if a.size else None
                        rc = lib.tpamd_planner_set_download_trajectories(ps._handle(), n, hp(ids), hp(off), cap,
                                                                         *[hp(out[k]) for k in keys])
                        assert (rc != 0) == (total > cap), (D, n, cap, rc)
                    else:
                        t = {k: torch.from_numpy(v).to(dev) for k, v in out.items()}
                        to, ti = torch.from_numpy(off).to(dev), torch.from_numpy(ids).to(dev)
                        dp = lambda a: a.data_ptr() if a.numel() else None
                        assert lib.tpamd_planner_set_download_trajectories_device(
                            ps._handle(), n, dp(ti), dp(to), cap, *[dp(t[k]) for k in keys], None) == 0
                        torch.cuda.synchronize()
                        off, out = to.cpu().numpy(), {k: v.cpu().numpy() for k, v in t.items()}
                    where = (D, "host" if host else "device", n, cap - total)
                    assert (off == want_off).all(), where + ("offsets",)
                    for k in keys:
                        if cap < total:
                            assert br._all_sentinel(out[k]), where + (k, "one row short: nothing is written")
                        else:
                            assert out[k][:total * width(k)].tobytes() == want[k], where + (k,)
                            assert br._all_sentinel(out[k][total * width(k):]), where + (k, "behind the rows")
            # ticks over a long list: 1025 x 1 (the last block of 256 holds one tick) and 37 x 7

            class Ticks:
                def ticks(self, ids, start_ns, step_ns, T, want=(True, True, True)):
                    m = len(start_ns)
                    out = {k: np.full((m, T, D), br.SENTINEL) for k in br.ARRAYS}
                    st = np.full((m, T), -77, dtype=np.int32)
                    if host:
                        g = dict(out, status=st)
                        hp = lambda a: a.ctypes.data_as(C.c_void_p)
                        assert lib.tpamd_planner_set_sample_at_ticks(
                            ps._handle(), m, hp(np.asarray(ids, dtype=np.int32)), hp(np.asarray(start_ns, dtype=np.int64)),
                            step_ns, T, hp(out["q"]), hp(out["qd"]), hp(out["qdd"]), hp(st)) == 0
                    else:
                        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
                        g = ps.sample_at_ticks(up(np.asarray(start_ns, dtype=np.int64)), step_ns, T,
                                               ids=up(np.asarray(ids, dtype=np.int32)), q=up(out["q"]), qd=up(out["qd"]),
                                               qdd=up(out["qdd"]), status=up(st))
                        torch.cuda.synchronize()
                        g = {k: v.cpu().numpy() for k, v in g.items()}
                    return dict(status=[int(x) for x in g["status"].reshape(-1)], **{k: g[k].reshape(-1) for k in br.ARRAYS})

            for count, T in ((1025, 1), (37, 7)):
                ids = br.id_list(rng, count, B, bad=not host)
                starts = []
                for e, b in enumerate(ids):
                    t = ref.buffers[b].t if 0 <= b < B else [1.0]
                    lo, hi = int(t[0] * 1e9), int(t[-1] * 1e9)
                    starts.append((lo + 1, (lo + hi) // 2, hi - 2 * MS, lo - 1, hi + 1)[e % 5])
                br.compare_ticks(ref, Ticks(), ids, starts, MS // 2, T, where=(D, host, count, T))
    finally:
        ps.close()


@pytest.mark.parametrize("D", SCAN_DOFS)
def test_planner_set_stop_trajectories_long_lists(env, D):
    """tpamd_planner_set_stop_trajectories with 1025 and 2049 repeated ids: k_stop_scan_offsets
    with more than one entry per thread. Per entry the reference is stop_reference's StopBeforeTime."""
    lib = env["lib"]
    ps, rows, amax = _planned_set(env, D)
    B = len(rows)
    rng = np.random.default_rng(D)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    lists = {b: {k: rows[b][k].tolist() for k in ("time", "q", "qd", "qdd")} for b in range(B)}
    memo = {}
    try:
        for Q in (1025, 2049):
            ids = rng.integers(0, B, size=Q).astype(np.int32)
            t_ns = np.zeros(Q, dtype=np.int64)
            for k, b in enumerate(ids):
                t = rows[b]["time"]
                lo, hi = int(round(t[0] * 1e9)), int(round(t[-1] * 1e9))
                t_ns[k] = (lo - MS, (lo + hi) // 2, hi, lo + (hi - lo) // 4, hi + MS, lo + 3 * (hi - lo) // 4)[(k + b) % 6]
            am = np.ascontiguousarray(amax[ids])
            refs = []
            for k, b in enumerate(ids):
                key = (int(b), int(t_ns[k]))
                if key not in memo:
                    memo[key] = sr.stop_before_time(lists[b]["time"], lists[b]["qd"], lists[b]["qdd"], amax[b].tolist(), 4e-3,
                                                    float(t_ns[k]) / 1e9)
                refs.append(memo[key])
            want_off = np.concatenate([[0], np.cumsum([len(r["time"]) for r in refs])]).astype(np.int64)
            total = int(want_off[-1])
            for cap in (total, total - 1):
                h = dict(status=np.full(Q, -77, np.int32), keep=np.full(Q, -77, np.int32), offsets=np.full(Q + 1, -77, np.int64),
                         time=np.full(cap, br.SENTINEL), q=np.full((cap, D), br.SENTINEL), qd=np.full((cap, D), br.SENTINEL),
                         qdd=np.full((cap, D), br.SENTINEL))
                rc = lib.tpamd_planner_set_stop_trajectories(ps._handle(), Q, p(ids), p(t_ns), p(am), 4e-3, p(h["status"]),
                                                             p(h["keep"]), p(h["offsets"]), cap, p(h["time"]), p(h["q"]),
                                                             p(h["qd"]), p(h["qdd"]))
                assert (rc != 0) == (cap < total), (D, Q, cap, rc)
                assert (h["offsets"] == want_off).all(), (D, Q, cap, "offsets")
                assert h["status"].tolist() == [r["status"] for r in refs] and h["keep"].tolist() == [r["keep"] for r in refs]
                if cap < total:
                    assert all(br._all_sentinel(h[k]) for k in ("time", "q", "qd", "qdd")), (D, Q, "one row short")
                    continue
                assert h["time"].tobytes() == br.bits([x for r in refs for x in r["time"]]), (D, Q, "time")
                for k in ("qd", "qdd"):
                    assert h[k].tobytes() == br.bits([x for r in refs for row in r[k] for x in row]), (D, Q, k)
                want_q = b"".join(rows[b]["q"][r["first"]:r["last"] + 1].tobytes() for b, r in zip(ids, refs))
                assert h["q"].tobytes() == want_q, (D, Q, "q")
            assert sum(1 for r in refs if r["status"] == sr.OK and len(r["time"]) > 1) > Q // 4
    finally:
        ps.close()


@pytest.mark.parametrize("D", [1, 9, 16])
def test_insert_from_permuted_planners(env, D):
    """tpamd_buffer_set_insert_from_planner_set* with permuted planner_ids and buffer ids against
    the reference fed with the downloaded trajectories; then again after a discard, so that the
    second insert keeps samples."""
    torch, eng, E, dev, lib = env["torch"], env["eng"], env["E"], env["dev"], env["lib"]
    ps, rows, _ = _planned_set(env, D)
    B = len(rows)
    rng = np.random.default_rng(D)
    try:
        for host in (False, True):
            room = 2 * max(len(r["time"]) for r in rows) + 8      # no MORE, and the host entries never grow the set
            program = dict(B=B, D=D, tolerance=br.TIMESTEP_TOLERANCE, capacity=room)
            backend = GpuBackend(env, program, host)
            ref = br.ReferenceSet(B, D, capacity=room)
            try:
                for turn in range(2):
                    ids = rng.permutation(B)[:B - 3].astype(np.int32)
                    pids = rng.permutation(B)[:B - 3].astype(np.int32)
                    if turn:          # drop the front half of every buffer and move the rest back to start 1 ms
                        # before its old start: the new segments' fronts (the same plan start) fall inside
                        times = [dict(sec=buf.t[len(buf.t) // 2] if buf.t else 1.0) for buf in ref.buffers]
                        back = [dict(sec=-(buf.t[len(buf.t) // 2] - buf.t[0] + 1e-3) if buf.t else 0.0) for buf in ref.buffers]
                        for rnd in (dict(kind="discard", ids=None, unit="sec", entries=times),
                                    dict(kind="add_offset", ids=None, unit="sec", entries=back)):
                            assert backend.apply(rnd) == ref.apply(rnd)
                    entries = [dict(t=rows[pl]["time"].tolist(), q=rows[pl]["q"].tolist(), qd=rows[pl]["qd"].tolist(),
                                    qdd=rows[pl]["qdd"].tolist()) for pl in pids]
                    want = ref.apply(dict(kind="insert", ids=[int(x) for x in ids], unit="sec", entries=entries))
                    st = backend._arr(np.full(len(ids), -77, dtype=np.int32))
                    a, b = backend._arr(ids), backend._arr(pids)
                    f = lib.tpamd_buffer_set_insert_from_planner_set if host else lib.tpamd_buffer_set_insert_from_planner_set_device
                    rc = f(backend.bs._handle(), ps._handle(), len(ids), backend._p(a), backend._p(b), backend._p(st),
                           *(() if host else (None,)))
                    torch.cuda.synchronize()
                    assert rc == 0 and [int(x) for x in backend._back(st)] == want == [br.OK] * len(ids), (D, host, turn)
                    br.compare_download(ref.download(), backend.download(), (D, host, turn))
                    info = backend.info(None, [0] * B)
                    assert info["seq"] == [buf.seq for buf in ref.buffers] and info["count"] == [len(buf.t) for buf in ref.buffers]
                assert any(buf.seq > 0 for buf in ref.buffers), (D, "the second insert keeps samples")
            finally:
                backend.close()
    finally:
        ps.close()


def test_print_outcome_table_and_wall_time():
    """Prints only: the outcome table of the GPU results gathered by the tests above that ran in
    this process (each of them asserts its own columns) and the module's wall time so far."""
    print(br.outcome_table("buffer-set operations and ticks, GPU results (device entries)", br.OUTCOMES, _OUTCOMES))
    print("wall time of tests/test_gpu_buffer_readout_all_dofs.py: %.1f s" % (time.time() - _T0))

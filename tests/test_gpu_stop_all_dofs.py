"""The three stop kernels (k_fastest_stop<D>, k_stop_trajectories<D>, k_bset_stop<D>) at every
joint count D = 1..16, i.e. every lane-group width L = 2, 4, 8, 16, 32, full groups (2 D = L) and a
mostly idle one (D = 9), with 67 rows so that the last wave has only some of its groups live. The
inputs are the case families of tests/stop_reference.py (random, solver-shaped and the edge
branches: joints under the velocity cut, every candidate invalid, tied candidates, candidates on
the validity slack, a first step that ends the stop, a rest row on the last sample, non-increasing
times far into the row, counts 0, 1 and 2), not solver outputs. Every result must equal the
restatements bit for bit (fastest_stop_at_time of tests/test_fastest_stop_cpu.py, and
stop_reference's StopBeforeTime / StopAtIndex, written from the reference's sources) and pass the
long-double property checkers, which do not share the kernels' order of operations. What a call
must not write keeps a sentinel. Every outcome must occur for every D on the GPU's own results.

The batch fastest-stop entry has no `ids` argument; the ids permutation with repeats is driven
through the planner-set entries, which launch the same kernels (D in {1, 2, 4, 8, 9, 16})."""
import collections
import ctypes as C
import importlib
import time

import numpy as np
import pytest

from conftest import PKG_NAME
import stop_reference as sr
from test_fastest_stop_cpu import fastest_stop_at_time
from test_stop_reference_cpu import TIME_STEP, batch_results

pytestmark = pytest.mark.gpu

ALL_DOFS = list(range(1, 17))
SENTINEL = -9.25
MS = 1_000_000
_T0 = time.time()
_OUTCOMES = {"forward": {}, "backward": {}}


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    eng.build_library()
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev=torch.device("cuda", 0), lib=eng.load_library())


def _bits(a):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
    return np.ascontiguousarray(a).tobytes()


def _f64(x):
    return np.asarray(x, dtype=np.float64)


def _packed(D):
    results = batch_results(D)
    return results, sr.pack_batch([r["row"] for r in results], D)


# ------------------------------------------------------------------ fastest stop
def _fastest_stop(env, pk, D, host):
    """tpamd_fastest_stop_device / _host with every output pre-filled with the sentinel."""
    torch, eng, E, lib = env["torch"], env["eng"], env["E"], env["lib"]
    B, M = pk["time"].shape
    keys = ("time", "s", "qd", "qdd", "count", "amax", "fs_query")
    out = dict(stop_parameter=np.full(B, SENTINEL), stop_index=np.full(B, -77, np.int32), duration=np.full(B, SENTINEL),
               status=np.full(B, -77, np.int32), profile_time=np.full((B, M), SENTINEL),
               profile_rate2=np.full((B, M), SENTINEL), profile_drate2=np.full((B, M), SENTINEL))
    names = ("stop_parameter", "stop_index", "duration", "status", "profile_time", "profile_rate2", "profile_drate2")
    if host:
        inp = {k: np.ascontiguousarray(pk[k]) for k in keys}
        p = lambda a: a.ctypes.data
    else:
        inp = {k: torch.from_numpy(np.ascontiguousarray(pk[k])).to(env["dev"]) for k in keys}
        out = {k: torch.from_numpy(v).to(env["dev"]) for k, v in out.items()}
        p = lambda a: a.data_ptr()
    args = eng._FastestStopArgs(B, M, D, 0, *[p(inp[k]) for k in keys], *[p(out[k]) for k in names])
    if host:
        rc = lib.tpamd_fastest_stop_host(E._h, C.byref(args))
    else:
        rc = lib.tpamd_fastest_stop_device(E._h, C.byref(args), None)
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in out.items()}
    assert rc == 0
    return out


@pytest.mark.parametrize("D", ALL_DOFS)
def test_fastest_stop(env, D):
    results, pk = _packed(D)
    seen = collections.Counter()
    for host in (False, True):
        g = _fastest_stop(env, pk, D, host)
        for b, r in enumerate(results):
            row, ref, where = r["row"], r["forward"], (D, b, r["row"]["label"], "host" if host else "device")
            m = len(ref["rate2"])
            got = dict(status=int(g["status"][b]), stop_parameter=float(g["stop_parameter"][b]),
                       stop_index=int(g["stop_index"][b]), duration=float(g["duration"][b]),
                       time=g["profile_time"][b, :m].tolist(), rate2=g["profile_rate2"][b, :m].tolist(),
                       drate2=g["profile_drate2"][b, :m].tolist())
            assert (got["status"], got["stop_index"]) == (ref["status"], ref["stop_index"]), where
            for k in ("stop_parameter", "duration", "time", "rate2", "drate2"):
                assert _bits(_f64(got[k])) == _bits(_f64(ref[k])), where + (k,)
            for k in ("profile_time", "profile_rate2", "profile_drate2"):     # nothing behind the written prefix
                assert (g[k][b, m:] == SENTINEL).all(), where + (k, "sentinel")
            sr.check_fastest_stop(row["time"], row["s"], row["qd"], row["qdd"], row["amax"], row["fs_query"], got)
            if not host:
                seen.update(sr.forward_outcomes(row, got))
    _OUTCOMES["forward"][D] = seen
    missing = [k for k in sr.FORWARD_OUTCOMES if not seen[k] and k not in sr.UNREACHABLE.get(D, set())]
    assert missing == [], (D, missing)


# ------------------------------------------------------------------ stopping trajectories
def _got_stop(g, b, D):
    f, l = int(g["first"][b]), int(g["last"][b])
    return dict(status=int(g["status"][b]), keep=int(g["keep"][b]), first=f, last=l,
                time=g["out_time"][b, f:l + 1].tolist(), qd=g["out_qd"][b, f:l + 1].reshape(-1, D).tolist(),
                qdd=g["out_qdd"][b, f:l + 1].reshape(-1, D).tolist())


@pytest.mark.parametrize("D", ALL_DOFS)
def test_stop_trajectories(env, D):
    torch, E = env["torch"], env["E"]
    results, pk = _packed(D)
    B, M = pk["time"].shape
    seen = collections.Counter()
    for by_index in (False, True):
        for host in (False, True):
            conv = (lambda a: np.ascontiguousarray(a)) if host else \
                (lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"]))
            out = dict(out_time=conv(np.full((B, M), SENTINEL)), out_qd=conv(np.full((B, M, D), SENTINEL)),
                       out_qdd=conv(np.full((B, M, D), SENTINEL)))
            g = E.stop_trajectories(conv(pk["time"]), conv(pk["qd"]), conv(pk["qdd"]), conv(pk["amax"]), TIME_STEP,
                                    stop_time=None if by_index else conv(pk["query"]),
                                    stop_index=conv(pk["index"]) if by_index else None, count=conv(pk["count"]),
                                    out=out, host=host)
            if not host:
                torch.cuda.synchronize()
                g = {k: v.cpu().numpy() for k, v in g.items()}
            for b, r in enumerate(results):
                row, ref = r["row"], r["by_index" if by_index else "by_time"]
                where = (D, b, row["label"], "index" if by_index else "time", "host" if host else "device")
                got = _got_stop(g, b, D)
                assert tuple(got[k] for k in ("status", "keep", "first", "last")) == \
                    tuple(ref[k] for k in ("status", "keep", "first", "last")), where
                for k in ("time", "qd", "qdd"):
                    assert _bits(_f64(got[k])) == _bits(_f64(ref[k])), where + (k,)
                outside = np.ones(M, dtype=bool)
                outside[got["first"]:got["last"] + 1] = False       # a failed stop: first = n, last = n - 1
                for k in ("out_time", "out_qd", "out_qdd"):
                    assert (g[k][b][outside] == SENTINEL).all(), where + (k, "sentinel")
                sr.check_stop_segment(row["time"], row["qd"], row["qdd"], row["amax"], TIME_STEP, got,
                                      index=row["index"] if by_index else None, stop_time=row["query"])
                if not host:
                    seen.update(sr.backward_outcomes(row, got, by_index))
    _OUTCOMES["backward"][D] = seen
    missing = [k for k in sr.BACKWARD_OUTCOMES if not seen[k] and k not in sr.UNREACHABLE.get(D, set())]
    assert missing == [], (D, missing)


# ------------------------------------------------------------------ buffer sets
@pytest.mark.parametrize("D", ALL_DOFS)
def test_buffer_set_stop_in_place(env, D):
    """insert, then stop_before_time on the same rows: the download equals input[0, keep) ++
    segment, count and sequence number follow InsertSegment, a failed stop leaves the bytes."""
    torch, eng, E, dev = env["torch"], env["eng"], env["E"], env["dev"]
    results, pk = _packed(D)
    B = len(results)
    rows = [r["row"] for r in results]
    offsets = np.concatenate([[0], np.cumsum(pk["count"])]).astype(np.int64)
    flat = {k: np.concatenate([_f64(r[k]).reshape(len(r["time"]), D) for r in rows]) for k in ("q", "qd", "qdd")}
    flat["time"] = np.concatenate([_f64(r["time"]) for r in rows])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with eng.BufferSet(E, B, D, capacity=sr.STRIDE + 8) as bs:
        st = bs.insert(up(flat["time"]), up(flat["q"]), up(flat["qd"]), up(flat["qdd"]), up(offsets))
        assert (st["status"].cpu().numpy() == 0).all()
        before = bs.download()
        info0 = bs.info()
        stop = bs.stop_before_time(up(pk["amax"]), TIME_STEP, time_sec=up(pk["query"]))
        after = bs.download()
        info1 = bs.info()
        torch.cuda.synchronize()
        status = stop["status"].cpu().numpy()
        off0, off1 = before["offsets"].cpu().numpy(), after["offsets"].cpu().numpy()
        b0 = {k: before[k].cpu().numpy() for k in ("time", "q", "qd", "qdd")}
        b1 = {k: after[k].cpu().numpy() for k in ("time", "q", "qd", "qdd")}
        seq0, seq1 = info0["sequence"].cpu().numpy(), info1["sequence"].cpu().numpy()
        cnt1 = info1["num_samples"].cpu().numpy()
        moved = collections.Counter()
        for b, r in enumerate(results):
            row, ref, where = r["row"], r["by_time"], (D, b, r["row"]["label"])
            assert status[b] == ref["status"], where
            bt, bq, bv, ba = sr.stopped_buffer(row["time"], row["q"], row["qd"], row["qdd"], ref)
            sl = slice(int(off1[b]), int(off1[b + 1]))
            assert cnt1[b] == len(bt) == sl.stop - sl.start, where
            for k, want in (("time", bt), ("q", bq), ("qd", bv), ("qdd", ba)):
                assert _bits(b1[k][sl]) == _bits(_f64(want)), where + (k,)
            want_seq = 0 if ref["replaced"] else seq0[b] + 1 if ref["inserted"] else seq0[b]
            assert seq1[b] == want_seq, where + (int(seq1[b]), int(want_seq))
            if ref["status"] != sr.OK:
                s0 = slice(int(off0[b]), int(off0[b + 1]))
                for k in b0:
                    assert _bits(b0[k][s0]) == _bits(b1[k][sl]), where + (k, "a failed stop changes nothing")
                moved["failed"] += 1
            elif len(row["time"]):
                moved["keep_below_first" if ref["keep"] < ref["first"] else
                      "keep_above_first" if ref["keep"] > ref["first"] else "in_place"] += 1
        assert all(moved[k] for k in ("failed", "keep_below_first", "keep_above_first", "in_place")), (D, moved)


# ------------------------------------------------------------------ planner sets
@pytest.mark.parametrize("D", [1, 2, 4, 8, 9, 16])
def test_planner_set_stops(env, D):
    """70 planners (every seventh without a path) planned from waypoints on the device; the
    stop parameters (ids permuted, with repeats) and the stopping trajectories (host entry, and
    the device entry on a non-blocking stream) against the restatements on the download."""
    torch, eng, E, dev, lib = env["torch"], env["eng"], env["E"], env["dev"], env["lib"]
    B, N, step_ns = 70, 200, MS
    rng = np.random.default_rng(20261017 + D)
    W = rng.integers(3, 7, size=B)
    W[::7] = 0                                            # no waypoints: the planner keeps "no path"
    offsets = np.concatenate([[0], np.cumsum(W)]).astype(np.int32)
    wps = rng.uniform(-2.0, 2.0, size=(int(offsets[-1]), D))
    vmax, amax = rng.uniform(1.0, 2.0, size=(B, D)), rng.uniform(2.0, 4.0, size=(B, D))
    delta = rng.uniform(0.01, 0.03, size=B)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    with eng.PlannerSet(E, B, D, N, num_points=4, time_step_ns=step_ns) as ps:
        status, _ = ps.set_waypoints(up(wps), offsets, up(vmax), up(amax), up(delta))
        assert (status.cpu().numpy() == np.where(W == 0, sr.INVALID_ARGUMENT, 0)).all()
        summary = ps.plan(1000 * MS, 500 * MS)
        planned = (summary["status"].numpy() == 0) & (summary["num_samples"].numpy() > 2)
        assert not planned[::7].any() and planned.sum() >= B // 2, planned.sum()
        traj = ps.download_trajectories()
        torch.cuda.synchronize()
        off = traj["offsets"].cpu().numpy()
        tj = {k: traj[k].cpu().numpy() for k in ("time", "s", "q", "qd", "qdd")}
        rows = []
        for b in range(B):
            sl = slice(int(off[b]), int(off[b + 1]))
            rows.append({k: tj[k][sl].tolist() for k in tj})
        # one query per listed planner: ids a permutation with repeats
        # (tpamd_planner_set_stop_parameters takes at most B entries)
        ids = rng.permutation(np.concatenate([rng.permutation(B)[:B - 20], rng.integers(0, B, size=20)])).astype(np.int32)
        assert len(set(ids.tolist())) < len(ids) == B
        Q = len(ids)
        t_ns = np.zeros(Q, dtype=np.int64)
        for k, b in enumerate(ids):
            t = rows[b]["time"]
            if not t:
                t_ns[k] = 1000 * MS
                continue
            lo, hi = int(round(t[0] * 1e9)), int(round(t[-1] * 1e9))
            t_ns[k] = (lo - MS, lo, int(rng.integers(lo, hi + 1)), hi, hi + MS, (lo + hi) // 2)[k % 6]
        t_sec = t_ns.astype(np.float64) / 1e9                 # TimeToSec
        am = amax[ids]

        got = ps.stop_parameters(t_ns, ids=ids)
        mids = 0
        for k, b in enumerate(ids):
            r = rows[b]
            if not planned[b] and not r["time"]:
                want = (sr.OK, 0.0, 0.0)                      # no plan yet (path_timing_trajectory.cc:239-242)
            else:
                st, sp, idx, dur = fastest_stop_at_time(r["time"], r["s"], r["qd"], r["qdd"], amax[b].tolist(),
                                                        float(t_sec[k]))[:4]
                want = (st, sp, dur)
                mids += st == sr.OK and 0 < dur and idx < len(r["time"]) - 1
            assert int(got["status"][k]) == want[0], (D, k, b)
            assert _bits(got["stop_parameter"][k]) == _bits(np.float64(want[1])), (D, k, b)
            assert _bits(got["duration"][k]) == _bits(np.float64(want[2])), (D, k, b)
        assert mids > 0

        # the stopping trajectories: host entry, then the device entry on a non-blocking stream
        cap = int(sum(len(rows[b]["time"]) for b in ids)) + 64
        h = dict(status=np.full(Q, -77, np.int32), keep=np.full(Q, -77, np.int32), offsets=np.zeros(Q + 1, np.int64),
                 time=np.full(cap, SENTINEL), q=np.full((cap, D), SENTINEL), qd=np.full((cap, D), SENTINEL),
                 qdd=np.full((cap, D), SENTINEL))
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        rc = lib.tpamd_planner_set_stop_trajectories(ps._handle(), Q, p(ids), p(t_ns), p(np.ascontiguousarray(am)),
                                                     TIME_STEP, p(h["status"]), p(h["keep"]), p(h["offsets"]), cap,
                                                     p(h["time"]), p(h["q"]), p(h["qd"]), p(h["qdd"]))
        assert rc == 0
        stream = torch.cuda.Stream(device=dev)
        args = (up(t_ns), up(am), up(ids))
        with torch.cuda.stream(stream):                   # the wrapper reads offsets on the current stream
            d = ps.stop_trajectories(args[0], args[1], TIME_STEP, ids=args[2], capacity=cap, stream=stream)
        stream.synchronize()
        d = {k: v.cpu().numpy() for k, v in d.items()}
        seen = collections.Counter()
        for name, g in (("host", h), ("device", d)):
            assert g["offsets"][0] == 0
            for k, b in enumerate(ids):
                r, where = rows[b], (D, name, k, int(b))
                ref = sr.stop_before_time(r["time"], r["qd"], r["qdd"], am[k].tolist(), TIME_STEP, float(t_sec[k]))
                sl = slice(int(g["offsets"][k]), int(g["offsets"][k + 1]))
                assert int(g["status"][k]) == ref["status"] and int(g["keep"][k]) == ref["keep"], where
                assert sl.stop - sl.start == len(ref["time"]), where
                assert _bits(g["time"][sl]) == _bits(_f64(ref["time"])), where
                assert _bits(g["qd"][sl]) == _bits(_f64(ref["qd"]).reshape(-1, D)), where
                assert _bits(g["qdd"][sl]) == _bits(_f64(ref["qdd"]).reshape(-1, D)), where
                assert _bits(g["q"][sl]) == _bits(_f64(r["q"][ref["first"]:ref["last"] + 1]).reshape(-1, D)), where
                got_k = dict(ref, time=g["time"][sl].tolist(), qd=g["qd"][sl].tolist(), qdd=g["qdd"][sl].tolist())
                sr.check_stop_segment(r["time"], r["qd"], r["qdd"], am[k].tolist(), TIME_STEP, got_k,
                                      stop_time=float(t_sec[k]))
                seen[sr.STATUS_NAMES.get(ref["status"], "other")] += 1
            assert (g["time"][int(g["offsets"][Q]):] == SENTINEL).all(), (D, name, "rows behind the segments")
        assert seen["ok"] and seen["out_of_range"], seen


def test_print_outcome_table_and_wall_time():
    """Prints only: the outcome tables of the GPU results gathered by the tests above that ran in
    this process (each of them asserts its own row) and the module's wall time so far."""
    for kind, names in (("forward", sr.FORWARD_OUTCOMES), ("backward", sr.BACKWARD_OUTCOMES)):
        print(sr.outcome_table("%s stops, GPU results" % kind, names, _OUTCOMES[kind]))
    print("wall time of tests/test_gpu_stop_all_dofs.py: %.1f s" % (time.time() - _T0))

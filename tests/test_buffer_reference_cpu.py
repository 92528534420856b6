"""The buffer-set row operations and the bulk readouts against an independent statement
(tests/buffer_reference.py), on the CPU. For every D = 1..16 and exactly the programs the GPU test
(tests/test_gpu_buffer_readout_all_dofs.py) uses, the restatement of TrajectoryBuffer equals, bit
for bit and after every operation, the mirror (host/trajectory_buffer.cc) and the host-compilable
cores the kernels run (csrc/tpamd_buffer.h, csrc/tpamd_readout.h) through
tests/cpp/test_buffer_reference.cc; the cores' plan.move shows that every layout case is a
compaction there; the exact checkers pass on the restatement's own outputs; and every mutation
below, each standing for one kernel mistake, is noticed by the comparison the GPU test runs, on the
GPU test's own inputs. No GPU needed."""
import collections
import json
import math
import os
import subprocess
import zlib

import numpy as np
import pytest

from conftest import ROOT
from native_driver import build_driver
import buffer_reference as br

ALL_DOFS = list(range(1, 17))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver("test_buffer_reference.cc", tmp_path_factory.mktemp("buffer_reference"), opt="-O2",
                        extra_sources=("host/rescale_to_stop.cc", "host/trajectory_buffer.cc"), timeout=600)


def _hex(values):
    return " ".join(float(x).hex() for x in values)


def _op_line(rnd, b, e):
    kind = rnd["kind"]
    if kind == "insert":
        return "I %d %d %s" % (b, len(e["t"]), _hex(e["t"] + br._flat(e["q"]) + br._flat(e["qd"]) + br._flat(e["qdd"])))
    if kind == "append":
        return "A %d %s" % (b, _hex([e["t"]] + e["q"] + e["qd"] + e["qdd"]))
    if kind in ("discard", "add_offset"):
        return "%s %d %s" % ("D" if kind == "discard" else "O", b,
                             "1 %d" % e["ns"] if rnd["unit"] == "ns" else "0 " + float(e["sec"]).hex())
    return "X %d" % b


def _digest(buf):
    data = br.bits(buf.t + br._flat(buf.q) + br._flat(buf.qd) + br._flat(buf.qdd))
    return [zlib.crc32(data), zlib.adler32(data)]


def run_against_driver(exe, path, program, rng):
    """Runs the program through the driver and compares the mirror's and the cores' state after
    every operation, the info of every buffer after every round and the ticks at the end with the
    restatement. Returns the cores' plan.move per round and entry."""
    B, D = program["B"], program["D"]
    ref = br.ReferenceSet(B, D, program["tolerance"], program["capacity"])
    lines, checks = [], []
    for r, rnd in enumerate(program["rounds"]):
        before = [len(b.t) for b in ref.buffers]
        want = ref.apply(rnd)
        ids = rnd["ids"] if rnd["ids"] is not None else range(len(rnd["entries"]))
        for e, b in enumerate(ids):
            lines.append(_op_line(rnd, b, rnd["entries"][e]))
            buf = ref.buffers[b]
            checks.append(("op", (r, e, b, rnd["kind"]), [want[e], len(buf.t), buf.seq] + _digest(buf), before[b]))
        times = br.info_times(ref.buffers, r)
        info = ref.info(None, times)
        for b in range(B):
            lines.append("Q %d %d" % (b, times[b]))
            checks.append(("info", (r, b), [info[k][b] for k in ("count", "seq", "start_ns", "end_ns", "up_to")], None))
    for count, T, step in ((37, 7, br.TICK_STEP_NS), (32, 8, br.TICK_STEP_NS), (5, 4, 2 ** 62)):
        ids, starts = br.tick_requests(ref.buffers, count, rng, bad_ids=False)
        for b, s0 in zip(ids, starts):
            lines.append("T %d %d %d %d" % (b, s0, step, T))
            status, rows = br.sample_at_ticks(ref.buffers[b], s0, step, T)
            data = br.bits([x for row in rows if row is not None for arr in row for x in arr])
            checks.append(("ticks", (b, s0, step, T), status + [zlib.crc32(data), zlib.adler32(data)], None))
    with open(path, "w") as f:
        f.write("%d %d %d %s %d\n" % (B, D, program["capacity"], float(program["tolerance"]).hex(), len(lines)))
        f.write("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().split("\n")
    assert len(got) == 2 * len(checks)
    moves = collections.defaultdict(dict)
    for k, (what, where, want, count_before) in enumerate(checks):
        m, c = got[2 * k].split(), got[2 * k + 1].split()
        assert m[0] == "M" and c[0] == "C"
        m, c = [int(x) for x in m[1:]], [int(x) for x in c[1:]]
        if what == "op":
            assert m == want, (D, "mirror") + where + (m, want)
            assert c[:3] + c[5:] == want, (D, "cores") + where + (c, want)
            moves[where[0]][where[1]] = c[3]
        else:
            assert m == want, (D, "mirror", what) + where + (m, want)
            assert c == want, (D, "cores", what) + where + (c, want)
    return moves


@pytest.mark.parametrize("D", ALL_DOFS)
def test_restatement_equals_mirror_and_cores_bit_for_bit(driver, tmp_path, D):
    rng = np.random.default_rng(D)
    layout = br.layout_program(D)
    moves = run_against_driver(driver, tmp_path / "layout.txt", layout, rng)
    reached = 0
    for r, expect in enumerate(layout["expect"]):          # every layout case is a compaction on the cores
        if expect is None:
            continue
        ids = layout["rounds"][r]["ids"]
        for e, b in enumerate(ids):
            K, first = layout["cases"][b % len(layout["cases"])]
            rows = K if layout["rounds"][r]["kind"] == "insert" else layout["capacity"] - first
            assert moves[r][e] == rows, (D, r, e, K, first, moves[r][e])
            reached += 1
    assert reached == 2 * len(layout["cases"])
    run_against_driver(driver, tmp_path / "tolerance.txt", br.tolerance_program(D), rng)
    for repeat in (True, False):
        moves = run_against_driver(driver, tmp_path / "program.txt", br.operation_program(D, repeat), rng)
        assert any(v > 0 for rnd in moves.values() for v in rnd.values()), (D, repeat, "no compaction on the cores")


@pytest.mark.parametrize("D", ALL_DOFS)
def test_checkers_pass_on_the_restatement_and_every_outcome_is_reached(D):
    """run_program, run_ticks and run_packs (what the GPU test runs) on the restatement itself."""
    seen, stats = collections.Counter(), collections.Counter()
    rng = np.random.default_rng(D)
    for host in (False, True):
        program = br.layout_program(D, host=host)
        br.run_program(br.ReferenceBackend(program), program, seen, stats)
    assert stats["more"] > 0 and stats["compactions"] >= 3 * len(br.layout_cases(D))
    program = br.tolerance_program(D)
    br.run_program(br.ReferenceBackend(program), program, seen)
    for repeat in (True, False):
        program = br.operation_program(D, repeat)
        backend = br.ReferenceBackend(program)
        ref = br.run_program(backend, program, seen, stats)
        br.run_ticks(ref, backend, rng, seen, null_arrays=True)
        if repeat:      # ticks on and beside the repeated stamps: the reference's results are finite
            ids, starts = br.repeated_stamp_ticks(ref.buffers)
            assert len(ids) > 0, D
            br.compare_ticks(ref, backend, ids, starts, 1, 3, seen=seen)
            got = ref.ticks(ids, starts, 1, 3)
            assert br.OK in got["status"] and all(math.isfinite(x) for k in br.ARRAYS for x in got[k])
            assert all(math.isfinite(x) for buf in ref.buffers for x in buf.t + br._flat(buf.q) + br._flat(buf.qd))
    br.run_packs(ref, backend, rng, lengths=(0, 1, 1025))
    assert [k for k in br.OUTCOMES if not seen[k]] == [], D


def test_exact_tolerance_family_is_exact():
    """The boundary arguments of tolerance_program differ from the tolerance by nothing or by one
    ulp, in exact rationals, and each pair of buffers ends differently."""
    from fractions import Fraction as F
    program = br.tolerance_program(3)
    tol = F(program["tolerance"])
    first, ins, dis, tight, tdis = program["rounds"]
    t = lambda b, i: F(first["entries"][b]["t"][i])
    assert F(ins["entries"][0]["t"][0]) - t(0, 5) == tol and tol - (F(ins["entries"][1]["t"][0]) - t(1, 5)) == F(2) ** -52
    assert F(ins["entries"][2]["t"][0]) - t(2, 0) == tol and tol - (F(ins["entries"][3]["t"][0]) - t(3, 0)) == F(2) ** -52
    x = [F(e["sec"]) for e in dis["entries"]]
    assert x[0] - t(4, 3) == tol and x[1] - t(5, 3) == tol + F(2) ** -52
    assert t(8, 6) - x[4] == tol and t(9, 6) - x[5] == tol + F(2) ** -52
    y = [F(e["sec"]) for e in tdis["entries"]]
    assert y[0] - 3 == tol and y[1] - 3 == tol + F(2) ** -51
    ref = br.run_program(br.ReferenceBackend(program), program)
    counts = [len(b.t) for b in ref.buffers]
    assert counts[8] != counts[9] or ref.buffers[8].t[0] != ref.buffers[9].t[0]
    assert ref.buffers[0].t[0] == 3.0 and ref.buffers[1].t[0] != 3.0       # close (kept) / not close


def test_reference_test_numbers_hold():
    """The expected numbers the reference's own test states for InsertSegment (with and without
    the tolerance) and AppendSample, restated as data in tests/golden/trajectory_buffer_cases.json."""
    with open(os.path.join(ROOT, "tests", "golden", "trajectory_buffer_cases.json")) as f:
        cases = json.load(f)
    dt, D = cases["sample_time"], cases["num_joints"]
    for sc in cases["scenarios"]:
        buf, tol = br.Buffer(sc["tolerance"]), sc["tolerance"]
        for step in sc["steps"]:
            if step["op"] == "insert_empty":
                assert buf.insert_segment([], [], [], []) == br.OK
            elif step["op"] == "clear":
                buf.clear()
            else:
                offset = step["offset_base"] + step["offset_samples"] * dt
                t = [i * dt + offset for i in range(step["count"])]
                t[0] += step["front_shift_tolerances"] * tol
                rows = lambda f: [[float(f * i)] * D for i in range(step["count"])]
                assert buf.insert_segment(t, rows(1), rows(10), rows(100)) == br.OK
                want = [step["offset_base"] + k * dt for k in step["time_samples"]]
                if step["shifted"] >= 0:
                    want[step["shifted"]] += step["front_shift_tolerances"] * tol
                assert buf.t == want, (sc["name"], buf.t, want)
                for f, arr in ((1, buf.q), (10, buf.qd), (100, buf.qdd)):
                    assert arr == [[float(f * v)] * D for v in step["values"]], sc["name"]
            assert (buf.sequence_number(), buf.num_samples()) == (step["sequence"], step["num_samples"]), (sc["name"], step)
            if "start_ns" in step:
                assert (buf.start_time_ns(), buf.end_time_ns()) == (step["start_ns"], step["end_ns"])
    buf = br.Buffer()
    for a in cases["append"]:
        assert buf.append_sample(a["time"], *[[float(v)] * D for v in a["values"]]) == a["status"], a
    want = cases["append_result"]
    assert buf.num_samples() == want["num_samples"]
    for key, arr in (("positions", buf.q), ("velocities", buf.qd), ("accelerations", buf.qdd)):
        assert arr == [[float(v)] * D for v in want[key]]


# ------------------------------------------------------------------ mutations
class KeptCountOffByOne(br.Buffer):
    """k_bset_insert keeps one row too many (plan.keep + 1): caught by the packed download after
    the insert (run_program: 'download'; check_buffer_invariants: the kept count)."""
    def insert_segment(self, t, q, qd, qdd):
        old = self.snapshot()
        st = super().insert_segment(t, q, qd, qdd)
        cut = len(self.t) - len(t)
        if self.last == "kept" and cut < len(old["t"]):
            self.t.insert(cut, old["t"][cut])
            for k in br.ARRAYS:
                getattr(self, k).insert(cut, old[k][cut])
        return st


class InsertToleranceNotStrict(br.Buffer):
    """rs_kept_count compares `front - prev <= tolerance` (not <): caught by the exact-tolerance
    family, where the difference equals the tolerance (run_program: 'download')."""
    def insert_segment(self, t, q, qd, qdd):
        if q and self.t and self.t[0] < t[0]:
            it = sum(1 for x in self.t if x < t[0])
            if t[0] - self.t[it - 1] == self.tol:
                self.seq += 1
                for k, new in (("t", list(t)), ("q", q), ("qd", qd), ("qdd", qdd)):
                    setattr(self, k, getattr(self, k)[:it - 1] + [x if k == "t" else list(x) for x in new])
                self.last = "kept"
                return br.OK
        return super().insert_segment(t, q, qd, qdd)


class DiscardFlipped(br.Buffer):
    """bs_discard with one comparison's strictness flipped: `close` as < (flip = "close") or
    `interpolate` as >= (flip = "interpolate"): caught by the exact-tolerance family
    (run_program: 'download' and check_buffer_invariants)."""
    flip = "close"

    def discard_segment_before(self, time_sec):
        if not self.t or time_sec <= self.t[0] or time_sec > self.t[-1]:
            return super().discard_segment_before(time_sec)
        offset = sum(1 for x in self.t if x < time_sec)
        close = time_sec - self.t[offset - 1] <= self.tol
        interpolate = abs(self.t[offset] - time_sec) > self.tol
        if self.flip == "close":
            close = time_sec - self.t[offset - 1] < self.tol
        else:
            interpolate = abs(self.t[offset] - time_sec) >= self.tol
        if close or interpolate:
            offset -= 1
        if interpolate:
            rows = [self._value_at_time(a, time_sec)[1] for a in (self.q, self.qd, self.qdd)]
            self.t[offset] = time_sec
            self.q[offset], self.qd[offset], self.qdd[offset] = rows
        del self.t[:offset], self.q[:offset], self.qd[:offset], self.qdd[:offset]


class DiscardInterpolateFlipped(DiscardFlipped):
    flip = "interpolate"


class InterpolatedRowOneLate(br.Buffer):
    """bs_discard writes the interpolated row at first + offset + 1: the new first row keeps its
    old values and the second is overwritten (run_program: 'download')."""
    def discard_segment_before(self, time_sec):
        old = self.snapshot()
        n = len(self.t)
        super().discard_segment_before(time_sec)
        if self.last == "interpolated" and len(self.t) >= 2:
            drop = n - len(self.t)
            new = (self.t[0], self.q[0], self.qd[0], self.qdd[0])
            self.t[0], self.q[0], self.qd[0], self.qdd[0] = old["t"][drop], old["q"][drop], old["qd"][drop], old["qdd"][drop]
            self.t[1], self.q[1], self.qd[1], self.qdd[1] = new


class LastStampInterpolated(br.Buffer):
    """tb_bracket without the `lo == n` case: a tick on the last stamp is interpolated between the
    last two samples (fraction 1) instead of copied (compare_ticks: 'tick values', check_setpoint)."""
    def _value_at_time(self, values, time_sec):
        st, l, u = self.offset_bracket(time_sec)
        if st == br.OK and l == u and l > 0:
            f = (time_sec - self.t[l - 1]) / (self.t[l] - self.t[l - 1])
            return br.OK, [a + f * (b - a) for a, b in zip(values[l - 1], values[l])]
        return super()._value_at_time(values, time_sec)


class FractionFromUpperEnd(br.Buffer):
    """tb_fraction as (t_u - x) / (t_u - t_l): the lerp runs from the wrong bracket end
    (compare_ticks: 'tick values', check_setpoint; run_program through the discard's new row)."""
    def _value_at_time(self, values, time_sec):
        st, l, u = self.offset_bracket(time_sec)
        if st == br.OK and l != u:
            f = (self.t[u] - time_sec) / (self.t[u] - self.t[l])
            return br.OK, [a + f * (b - a) for a, b in zip(values[l], values[u])]
        return super()._value_at_time(values, time_sec)


def _mutant(buffer_class):
    return lambda program: br.ReferenceBackend(program, buffer_class)


def faulty_move(values, shift, chunks_reversed):
    """bs_move_down_wg gone wrong on `values` (the kept doubles, which stand `shift` doubles above
    their destination): 256-double chunks copied forward, either with chunk c + 1 written before
    chunk c is read (`chunks_reversed`: the chunks in the wrong order), or without the barrier
    between a chunk's reads and its writes while its four waves run last first."""
    n = len(values)
    mem = [None] * shift + list(values)
    if chunks_reversed:
        for base in reversed(range(0, n, 256)):
            x = [mem[shift + i] for i in range(base, min(base + 256, n))]
            mem[base:base + len(x)] = x
    else:
        for base in range(0, n, 256):
            for wave in (3, 2, 1, 0):
                for i in range(base + 64 * wave, min(base + 64 * wave + 64, n)):
                    mem[i] = mem[shift + i]
    return mem[:n]


class FaultyCompaction(br.ReferenceBackend):
    """k_bset_insert whose compaction is faulty_move: the kept rows of a compacting insert or
    append arrive damaged (run_program: 'download' / kept rows are bit-copies). The first row of
    each buffer is tracked as the header of csrc/tpamd_buffer.h states it."""
    chunks_reversed = False

    def __init__(self, program):
        super().__init__(program)
        self.first = [0] * program["B"]

    def apply(self, rnd):
        before = [len(b.t) for b in self.set.buffers]
        status = super().apply(rnd)
        ids = rnd["ids"] if rnd["ids"] is not None else range(len(rnd["entries"]))
        D = self.set.D
        for e, b in enumerate(ids):
            buf = self.set.buffers[b]
            n1 = len(buf.t)
            added = 0 if status[e] != br.OK else 1 if rnd["kind"] == "append" else \
                len(rnd["entries"][e]["t"]) if rnd["kind"] == "insert" else 0
            if added:
                keep = n1 - added
                if keep == 0:
                    self.first[b] = 0
                elif self.first[b] + n1 > self.room:
                    shift = self.first[b]
                    buf.t[:keep] = faulty_move(buf.t[:keep], shift, self.chunks_reversed)
                    for a in (buf.q, buf.qd, buf.qdd):
                        flat = faulty_move(br._flat(a[:keep]), shift * D, self.chunks_reversed)
                        a[:keep] = [flat[i * D:(i + 1) * D] for i in range(keep)]
                    self.first[b] = 0
            elif rnd["kind"] in ("discard", "clear"):
                self.first[b] = 0 if n1 == 0 else self.first[b] + before[b] - n1
        return status


class FaultyCompactionChunksReversed(FaultyCompaction):
    chunks_reversed = True


class ScanDropsCarry(br.ReferenceBackend):
    """k_pset_scan_offsets with per >= 2 entries per thread, where thread t's exclusive prefix
    misses the sum of thread t - 1's run (compare_pack: 'offsets'). With at most 1024 entries
    every thread has one entry and the mistake does not exist: the long lists are needed."""
    def download(self, ids=None, capacity=None):
        out = super().download(ids, capacity)
        if ids is not None and len(ids) > 1024:
            per = (len(ids) + 1023) // 1024
            counts = [len(self.set.buffers[b].t) if 0 <= b < self.set.B else 0 for b in ids]
            off = list(out["offsets"])
            for k in range(per, len(ids)):
                lo = (k // per) * per                      # the first entry of this entry's thread
                off[k] -= sum(counts[lo - per:lo])
            out["offsets"] = off
        return out


class PackIgnoresCapacity(br.ReferenceBackend):
    """k_pset_pack_trajectories with `offsets[count] > capacity + 1` as its guard: rows are written
    when the total exceeds the capacity by one (compare_pack: 'one row short: nothing is written')."""
    def download(self, ids=None, capacity=None):
        out = super().download(ids, capacity)
        if capacity is not None and out["offsets"][-1] == capacity + 1:
            for k, w in (("t", 1), ("q", self.set.D), ("qd", self.set.D), ("qdd", self.set.D)):
                rows = np.frombuffer(br.pack_bytes(self.set.buffers, ids, k), dtype=np.float64)
                out[k][:] = rows[:capacity * w]
        return out


def _gpu_comparison(make_backend, D, parts):
    """What tests/test_gpu_buffer_readout_all_dofs.py runs for D joints, on another backend."""
    rng = np.random.default_rng(D)
    if "layout" in parts:
        program = br.layout_program(D)
        br.run_program(make_backend(program), program)
    if "tolerance" in parts:
        program = br.tolerance_program(D)
        br.run_program(make_backend(program), program)
    if "program" in parts or "ticks" in parts or "packs" in parts:
        program = br.operation_program(D)
        backend = make_backend(program)
        ref = br.run_program(backend, program)
        if "ticks" in parts:
            br.run_ticks(ref, backend, rng)
        if "packs" in parts:
            br.run_packs(ref, backend, rng)


MUTATIONS = [
    ("kept count off by one", _mutant(KeptCountOffByOne), ("program",)),
    ("insert tolerance <= instead of <", _mutant(InsertToleranceNotStrict), ("tolerance",)),
    ("discard close < instead of <=", _mutant(DiscardFlipped), ("tolerance",)),
    ("discard interpolate >= instead of >", _mutant(DiscardInterpolateFlipped), ("tolerance",)),
    ("interpolated row one row late", _mutant(InterpolatedRowOneLate), ("program",)),
    ("compaction without the barrier inside a chunk", FaultyCompaction, ("layout",)),
    ("compaction with a chunk written before the one below is read", FaultyCompactionChunksReversed, ("layout",)),
    ("offset scan drops a carry between two threads' runs", ScanDropsCarry, ("packs",)),
    ("pack writes with the total one above the capacity", PackIgnoresCapacity, ("packs",)),
    ("tick on the last stamp interpolated", _mutant(LastStampInterpolated), ("ticks",)),
    ("lerp fraction from the wrong bracket end", _mutant(FractionFromUpperEnd), ("ticks",)),
]


@pytest.mark.parametrize("D", [1, 7, 16])
@pytest.mark.parametrize("name,make_backend,parts", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_noticed(name, make_backend, parts, D):
    with pytest.raises(AssertionError):
        _gpu_comparison(make_backend, D, parts)


def test_unmutated_comparison_passes_and_short_lists_miss_the_scan_mistake():
    """The comparison of the mutation test passes on the restatement itself, so a mutation that is
    noticed is noticed for what it changes; and the dropped carry of the scan passes every list of
    at most 1024 entries, which is why the GPU test lists 1025 and more."""
    _gpu_comparison(br.ReferenceBackend, 3, ("layout", "tolerance", "program", "ticks"))
    program = br.operation_program(3)
    backend = ScanDropsCarry(program)
    ref = br.run_program(backend, program)
    br.run_packs(ref, backend, np.random.default_rng(3), lengths=(0, 1, 1023, 1024))
    with pytest.raises(AssertionError):
        br.run_packs(ref, backend, np.random.default_rng(3), lengths=(1025,))

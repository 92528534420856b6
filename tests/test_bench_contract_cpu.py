"""What can be checked of bench.py without a GPU: the metric string is BASELINE.json's, the
algorithmic-bytes figure is SURVEY.md 8(d)'s, and the script refuses to run without a GPU."""
import importlib.util
import json
import os
import subprocess
import sys

from conftest import ROOT


def _bench():
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_metric_and_algorithmic_bytes():
    bench = _bench()
    with open(os.path.join(ROOT, "BASELINE.json")) as f:
        assert bench.baseline_metric() == json.load(f)["metric"]
    # inputs 8*(P*D + P+3 + 2D + 4) + outputs t, s, sd, q: 8*N*(3+D); D = 7, N = 2000, P = 28
    assert bench.algorithmic_bytes_per_path(7, 2000, 28) == 8 * (28 * 7 + 31 + 14 + 4) + 8 * 2000 * 10
    assert bench.algorithmic_bytes_per_path(7, 2000, 28) == 161960
    assert bench.HBM_PEAK_GBS == 8000.0


def test_bench_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        return
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=300)
    assert res.returncode != 0
    assert "needs a GPU" in (res.stderr + res.stdout)


def test_gather_payload_bytes_and_counter_file_binding(tmp_path, monkeypatch):
    bench = _bench()
    assert bench.gather_bytes_per_path("none", 7, 2000) == 0
    assert bench.gather_bytes_per_path("minimal", 7, 2000) == 16016       # sd, ds, time_start (default)
    assert bench.gather_bytes_per_path("compact", 7, 2000) == 32016       # sd, sdd, ds, time_start
    assert bench.gather_bytes_per_path("profile", 7, 2000) == 48000       # t, sd, sdd
    assert bench.gather_bytes_per_path("full", 7, 2000) == 160000         # + q
    assert bench.WORKLOADS == {"configs1": 1024, "configs2": 8192}
    # roofline.traffic is only reported from counters measured on these very kernel sources
    h = bench.kernel_source_hash()
    assert len(h) == 64 and h == bench.kernel_source_hash()
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    monkeypatch.setattr(bench, "kernel_source_hash", lambda: h)
    good = {"tag": "t", "source_sha256": h, "workload": "B1024:D7:N2000",
            "kernels": {"k_sweep": {"hbm_bytes": 5, "avg_us": 400.0, "valu_insts": 10,
                                    "valu_busy_pct": 40.0}}}
    (prof / "counters.json").write_text(json.dumps(good))
    assert bench.recorded_counters(1024, 7, 2000)["kernels"]["k_sweep"]["hbm_bytes"] == 5
    assert bench.recorded_counters(2048, 7, 2000) is None                  # other batch shape
    (prof / "counters.json").write_text(json.dumps(dict(good, source_sha256="0" * 64)))
    assert bench.recorded_counters(1024, 7, 2000) is None                  # stale kernels
    r = bench.roofline_block({"k_sweep": (0.4, 20), "k_sample_lp": (0.2, 5)}, 0.4, 1024, 7, 2000,
                             28, 0.7)
    assert r["traffic"] is None and r["valu"] is None and r["bound"] == "hbm"
    assert abs(r["achieved"] - 161960 * 1024 / 0.4e-3 / 1e9) < 1e-2
    (prof / "counters.json").write_text(json.dumps(good))
    r = bench.roofline_block({"k_sweep": (0.4, 20)}, 0.4, 1024, 7, 2000, 28, 0.7)
    assert r["traffic"] == 5 and r["step_traffic"] == 5 and r["valu"]["busy_pct"] == 40.0
    assert "instruction issue" in r["limiter"]


def test_dump_outputs_sample_budget_and_files(tmp_path):
    """--dump-outputs: a fixed subset of paths within 64 MB on disk at the benchmarked shapes, every
    array a float64 .npy holding the rows of the chosen paths."""
    import numpy as np
    import torch
    bench = _bench()
    for B, D, N in ((1024, 7, 2000), (8192, 7, 2000), (1024, 14, 2000)):
        s = bench.dump_path_subset(B, D, N)
        assert len(s) < B and (np.diff(s) > 0).all() and s[0] >= 0 and s[-1] < B
        assert (s == bench.dump_path_subset(B, D, N)).all()                  # same paths on every run
        assert 8 * 3 * B + len(s) * (8 * N * (4 + 3 * D) + 8) + 11 * 128 <= 64 * 10**6
    assert (bench.dump_path_subset(5, 7, 300) == np.arange(5)).all()         # small batches: every path
    B, D, N = 6, 3, 10
    g = torch.Generator().manual_seed(1)
    out = {k: torch.rand(B, N, dtype=torch.float64, generator=g) for k in ("time", "s", "sd", "sdd")}
    out.update({k: torch.rand(B, N, D, dtype=torch.float64, generator=g) for k in ("q", "qd", "qdd")})
    out["status"] = torch.arange(B, dtype=torch.int32)
    out["last_extremal_index"] = torch.arange(B, dtype=torch.int32) * 3
    out["max_time_increment"] = torch.rand(B, dtype=torch.float64, generator=g)
    sample = np.array([1, 4])
    nbytes = bench.dump_outputs(out, sample, 100, str(tmp_path / "d"))
    files = {p.stem: np.load(p) for p in (tmp_path / "d").iterdir()}
    assert set(files) == set(out) | {"path_index"}
    assert all(a.dtype == np.float64 for a in files.values())
    assert sum(p.stat().st_size for p in (tmp_path / "d").iterdir()) == nbytes
    assert nbytes == sum(a.nbytes for a in files.values()) + 11 * 128     # .npy headers
    assert (files["path_index"] == [101, 104]).all()
    assert (files["status"] == np.arange(B)).all() and files["max_time_increment"].shape == (B,)
    assert (files["q"] == out["q"].numpy()[sample]).all() and files["time"].shape == (2, N)

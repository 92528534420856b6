"""Refined waypoint batches on the GPU (include/tpamd.h tpamd_time_waypoint_paths_refined_*): a
small batch whose waypoint counts differ (one path has none), 33 samples that cover each path
exactly (delta NULL). The primary outputs are those of time_waypoint_paths, every used slot is the
joint-form plain solve of the engine's own fitted spline at the slot's final grid, and slot map,
counters, status, sd2, sdd and records are the oracle's (tests/refine_cases.py waypoint_case, whose
conditions tests/test_refine_cpu.py asserts on the CPU). Bit equality, NaN by position."""
import importlib

import numpy as np
import pytest

import check_reference as cr
import refine_cases as cases
import refine_reference as rr
from conftest import PKG_NAME
from test_gpu_refine_joint import (PER_PATH, PER_SAMPLE, PER_SAMPLE_D, PRE, PRE_INT, refine_arrays, same,
                                   solution_arrays, to_numpy)

pytestmark = pytest.mark.gpu

N = cases.SAMPLES
NO_WAYPOINTS = 11


@pytest.fixture(scope="module")
def env():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: -m gpu tests must run on an MI355X")
    eng = importlib.import_module(PKG_NAME + ".engine")
    return dict(torch=torch, eng=eng, E=eng.Engine(0), dev="cuda:0")


def waypoint_outputs(Bw, D, S, host, env):
    out = solution_arrays(Bw, N, D, host, env)
    extra = {"num_points": np.full(Bw, PRE_INT, dtype=np.int32), "path_end": np.full(Bw, PRE),
             "delta_used": np.full(Bw, PRE), "knots": np.full((Bw, S + 3), PRE),
             "control_points": np.full((Bw, S, D), PRE)}
    for k, a in extra.items():
        out[k] = a if host else env["torch"].from_numpy(a).to(env["dev"])
    return out


def run(env, D, refined, host=False):
    call, joint, ref = cases.waypoint_case(D)
    Bw = len(cases.WAYPOINT_COUNTS)
    S = max(4, max(len(c) for c in joint["control_points"] if c is not None))
    conv = (lambda a: np.ascontiguousarray(a)) if host else (
        lambda a: env["torch"].from_numpy(np.ascontiguousarray(a)).to(env["dev"]))
    out = waypoint_outputs(Bw, D, S, host, env)
    args = (conv(call["waypoints"]), call["offsets"], conv(call["vmax"]), conv(call["amax"]), N)
    if refined:
        arrays = refine_arrays(Bw, Bw, cases.MAX_SAMPLES, D, host, env)
        got, refine = env["E"].time_waypoint_paths_refined(*args, cases.MAX_ROUNDS, cases.MAX_SAMPLES, Bw,
                                                           outputs=out, refined=arrays, host=host)
    else:
        got, refine = env["E"].time_waypoint_paths(*args, outputs=out, host=host), None
    if not host:
        env["torch"].cuda.synchronize()
    return to_numpy(got), to_numpy(refine) if refine else None, S


@pytest.mark.parametrize("D", [7, 16])
def test_refined_waypoint_batch(env, D):
    eng, E, torch = env["eng"], env["E"], env["torch"]
    call, joint, ref = cases.waypoint_case(D)
    Bw = len(cases.WAYPOINT_COUNTS)
    empty = cases.WAYPOINT_COUNTS.index(0)
    plain, _, S = run(env, D, refined=False)
    out, got, _ = run(env, D, refined=True)
    for name in list(PER_SAMPLE + PER_SAMPLE_D + PER_PATH) + ["num_points", "path_end", "delta_used", "knots",
                                                              "control_points"]:
        assert same(out[name], plain[name]), name
    assert out["status"][empty] == NO_WAYPOINTS and got["slot"][empty] == rr.NOTHING
    assert got["check"]["violations"][empty] == -1
    # the engine's fit is the oracle's, so the reference's delta is the engine's
    for b in range(Bw):
        if joint["knots"][b] is not None:
            P = len(joint["control_points"][b])
            assert out["num_points"][b] == P and same(out["knots"][b, :P + 3], joint["knots"][b])
            assert same(out["control_points"][b, :P], joint["control_points"][b])
            assert same(out["delta_used"][b], np.float64(joint["delta"][b]))
        assert cr.same_record(cr.record_of(got["check"], b), ref["round0"][b]["record"]), b
    assert same(got["slot"], ref["slot"]) and same(got["slot_path"], ref["slot_path"])
    assert got["num_refined"][0] == ref["num_refined"] >= 2
    assert same(got["rounds"], ref["rounds"]) and same(got["num_samples"], ref["num_samples"])
    assert same(got["delta"], ref["delta"])
    sol = got["refined"]
    for k in range(Bw):
        b, n = int(ref["slot_path"][k]), int(ref["num_samples"][k])
        assert cr.same_record(cr.record_of(got["refined_check"], k), ref["refined_check"][k]), (k, b)
        for name in PER_SAMPLE + PER_SAMPLE_D:
            assert (sol[name][k, n:] == PRE).all(), (name, k)
        if b < 0:
            for name in PER_PATH:
                assert sol[name][k] == (PRE if name == "max_time_increment" else PRE_INT), (name, k)
            continue
        # the joint-form plain solve of the engine's fitted spline, alone, at the slot's final grid
        P = int(out["num_points"][b])
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env["dev"])
        inp = {"knots": t(out["knots"][b:b + 1, :P + 3]), "control_points": t(out["control_points"][b:b + 1, :P]),
               "max_velocity": t(call["vmax"][b:b + 1]), "max_acceleration": t(call["amax"][b:b + 1]),
               "path_start": t(np.zeros(1)), "delta": t(ref["delta"][k:k + 1]), "sd_start": t(np.zeros(1)),
               "time_start": t(np.zeros(1))}
        alone = solution_arrays(1, n, D, False, env)
        E.time_joint_paths(inp, alone, n)
        torch.cuda.synchronize()
        alone = to_numpy(alone)
        for name in PER_SAMPLE + PER_SAMPLE_D:
            assert same(sol[name][k, :n], alone[name][0]), (name, k, b)
        for name in PER_PATH:
            assert same(sol[name][k], alone[name][0]), (name, k, b)
        f = ref["final"][k]
        assert sol["status"][k] == f["status"], (k, b)
        if f["status"] == 0:
            assert same(sol["sd2"][k, :n], f["sd2"]) and same(sol["sdd"][k, :n], f["sdd"]), (k, b)


def test_host_entry_equals_the_device_entry(env):
    D = 7
    out_d, got_d, _ = run(env, D, refined=True)
    out_h, got_h, _ = run(env, D, refined=True, host=True)
    for name in PER_SAMPLE + PER_SAMPLE_D + PER_PATH:
        assert same(out_h[name], out_d[name]), name
        assert same(got_h["refined"][name], got_d["refined"][name]), name
    for name in ("slot", "slot_path", "num_refined", "rounds", "num_samples", "delta"):
        assert same(got_h[name], got_d[name]), name
    for name in cr.KEYS:
        assert same(got_h["check"][name], got_d["check"][name]), name
        assert same(got_h["refined_check"][name], got_d["refined_check"][name]), name

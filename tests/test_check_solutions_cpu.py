"""The reference side of the solution check, without a GPU: tests/check_reference.py against the
oracle's SolutionSatisfiesConstraints (tpo.Profile.constraint_violations, time_optimal_path_timing.cc:
492-518) on the oracle's own solutions of the synthetic batches the GPU tests use, that those batches
hold both outcomes, and the layouts of the two new C structs."""
import ctypes
import importlib

import numpy as np
import pytest

import check_reference as cr
from conftest import PKG_NAME


@pytest.fixture(scope="module")
def env():
    from oracle import tpo
    tpo.build()
    return dict(tpo=tpo, syn=importlib.import_module(PKG_NAME + ".synthetic"))


@pytest.fixture(scope="module")
def joint_counts(env):
    return {s: cr.oracle_counts(env["tpo"], env["syn"].make_joint_batch(16, s[0], s[1], s[2])) for s in cr.JOINT_SHAPES}


@pytest.fixture(scope="module")
def cartesian_counts(env):
    return {s: cr.oracle_counts(env["tpo"], env["syn"].make_cartesian_batch(cr.cartesian_paths(s), s[0], s[1], s[2]),
                                cartesian=True) for s in cr.CARTESIAN_SHAPES}


def _nonzero(counts):
    return [b for b, (rc, viol, _, _) in enumerate(counts) if rc == 0 and viol != 0]


@pytest.mark.parametrize("shape", cr.JOINT_SHAPES)
def test_helper_counts_what_the_oracle_counts_joint(joint_counts, shape):
    for b, (rc, viol, rec, _) in enumerate(joint_counts[shape]):
        assert rc == 0, (shape, b, rc)
        assert rec[0] == viol, (shape, b)
        assert (rec[4] == -1) == (viol == 0)
        assert 0 <= rec[2] < shape[1] and 0 <= rec[3] < 2 * shape[0]
        assert (rec[1] > cr.KT) == (viol != 0)      # a violated row exceeds its bound by more than kTiny


@pytest.mark.parametrize("shape", cr.CARTESIAN_SHAPES)
def test_helper_counts_what_the_oracle_counts_cartesian(cartesian_counts, shape):
    for b, (rc, viol, rec, _) in enumerate(cartesian_counts[shape]):
        assert rc == 0, (shape, b, rc)
        assert rec[0] == viol, (shape, b)
        assert (rec[4] == -1) == (viol == 0)
        assert 0 <= rec[2] < shape[1] and 0 <= rec[3] < 2 * shape[0] + 2


def test_inputs_hold_both_outcomes_joint(joint_counts):
    nz = {s: _nonzero(c) for s, c in joint_counts.items()}
    assert nz[(7, 65, 4)] == [5, 10, 12]
    assert nz[(6, 257, 5)] == [2]
    assert nz[(8, 200, 10)] == [1, 5, 11]
    assert nz[(16, 33, 3)] == [b for b in range(16) if b != 14]
    for s in ((1, 3, 2), (3, 64, 3), (14, 129, 6)):
        assert nz[s] == []
    for s in ((7, 65, 4), (6, 257, 5), (8, 200, 10), (16, 33, 3)):
        assert 0 < len(nz[s]) < 16, s


def test_inputs_hold_both_outcomes_cartesian(cartesian_counts):
    nz = {s: len(_nonzero(c)) for s, c in cartesian_counts.items()}
    assert nz == {(1, 3, 2): 0, (3, 64, 3): 0, (6, 65, 4): 1, (7, 257, 5): 5, (14, 129, 6): 14, (16, 33, 3): 13}
    for s in ((6, 65, 4), (7, 257, 5), (14, 129, 6), (16, 33, 3)):
        assert 0 < nz[s] < 16, s


def test_helper_edges():
    """The kTiny edge, NaN rows, the tie rule and the empty record on hand-made rows."""
    A = np.array([[1.0, 0.0], [1.0, 0.0], [1.0, 0.0]])
    B = np.array([[0.0, 1.0], [0.0, 1.0], [0.0, 1.0]])
    sdd, sd2 = np.array([0.5, 0.5, np.nan]), np.array([2.0, 2.0, 2.0])
    lo = np.full((3, 2), -10.0)
    hi = np.array([[0.5 - cr.KT, 10.0], [np.nextafter(0.5 - cr.KT, -np.inf), 10.0], [10.0, 10.0]])
    rec = cr.check_rows(A, B, lo, hi, sd2, sdd)
    assert rec[0] == 1 and rec[4] == 1 and (rec[2], rec[3]) == (1, 0)
    # equal excesses: the first flattened index wins
    rec = cr.check_rows(A[:2], B[:2], lo[:2], np.full((2, 2), 10.0), sd2[:2], sdd[:2])
    assert rec == (0, -8.0, 0, 1, -1)
    # nothing but NaN
    assert cr.same_record(cr.check_rows(A, B, lo, hi, sd2, np.full(3, np.nan)), (0, np.nan, -1, -1, -1))
    assert not cr.same_record((0, 0.0, 0, 0, -1), (0, -0.0, 0, 0, -1))
    rec = cr.check_rows(A * np.nan, B, lo, hi, sd2, sdd)
    assert rec[0] == 0 and np.isnan(rec[1]) and rec[2:] == (-1, -1, -1)


def test_struct_layouts_match_header():
    eng = importlib.import_module(PKG_NAME + ".engine")
    assert ctypes.sizeof(eng._Solution) == 4 * 8            # tpamd_solution: four pointers
    assert ctypes.sizeof(eng._CheckOutputs) == 5 * 8        # tpamd_check_outputs: five pointers
    assert [n for n, _ in eng._Solution._fields_] == ["sd2", "sd", "sdd", "status"]
    assert [n for n, _ in eng._CheckOutputs._fields_] == list(cr.KEYS)
    for name in ("tpamd_check_rows", "tpamd_check_joint_paths", "tpamd_check_cartesian_paths"):
        assert name + "_device" in eng.ABI_SYMBOLS and name + "_host" in eng.ABI_SYMBOLS

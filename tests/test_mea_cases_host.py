"""The constructed pair lists of tests/mea_cases.py through the host stage (npr_mea_cigar) against the oracle's O(k^2) all-pairs restatement of
the rule: ops and score exactly.  No GPU: this checks the generator and the host stage before a device is involved."""
import numpy as np
import pytest

import mea_cases as mc
from helpers import orc

CASES = mc.cases()  # asserts, while it generates, that every case hits the corner it is named for
_NAMED = [c for c in CASES if not c[0].startswith("i_fuzz")]
_FUZZ = [c for c in CASES if c[0].startswith("i_fuzz")]


@pytest.fixture(scope="module")
def brute():
    """name -> (ops, score) of the brute force, computed once"""
    return {c[0]: brute_force(c) for c in CASES}


def brute_force(case):
    _, lX, lY, x, y, p, gg, mg = case
    ops, score = orc.mea_cigar(lX, lY, x, y, p.astype(np.float64), gg, mg, brute_force=True)
    return [tuple(o) for o in ops], score


def _check(case, want):
    from nanopore_amd import realign as R
    name, lX, lY, x, y, p, gg, mg = case
    order = np.lexsort((y, x))
    got, gs = R.mea_cigar(lX, lY, x[order], y[order], p[order], gg, mg)
    assert [tuple(o) for o in got] == want[0], name
    assert gs == want[1], name
    fen, fs = orc.mea_cigar(lX, lY, x, y, p.astype(np.float64), gg, mg)
    assert [tuple(o) for o in fen] == want[0] and fs == want[1], name
    rep = mc.replay(case)  # the walk in the kernels' visit order is a statement of the rule as well
    assert rep["ops"] == want[0] and rep["score"] == want[1], name
    assert sum(n for o, n in want[0] if o != mc.OP_I) == lX and sum(n for o, n in want[0] if o != mc.OP_D) == lY, name


@pytest.mark.parametrize("case", _NAMED, ids=[c[0] for c in _NAMED])
def test_named_case_host_stage_equals_brute_force(case, brute):
    _check(case, brute[case[0]])


def test_fuzz_cases_host_stage_equals_brute_force(brute):
    assert len(_FUZZ) >= 290 and len({(c[6], c[7]) for c in _FUZZ}) == 9
    for case in _FUZZ:
        _check(case, brute[case[0]])


def test_rules_every_case_keeps():
    for name, lX, lY, x, y, p, gg, mg in CASES:
        assert p.dtype == np.float32 and x.dtype == np.int32 and y.dtype == np.int32
        assert len(set(zip(x.tolist(), y.tolist()))) == len(x), name
        if len(x):
            assert np.bincount(y).max() <= 64, name
            assert np.bincount(x).max() <= 64 or name == "e_group65", name

"""npr_bam_sort_order (csrc/npr_bam.hip: k_sort_hist, the scan, k_sort_scatter) against Python's stable sort of the same keys
(tests/bam_reference.py), exactly: sizes around the wavefront, the round (256), the tile (2048) and several tiles; ties, which must keep
their input order; keys whose tid digits straddle a pass."""
import numpy as np
import pytest

import bam_reference as ref

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 100003)


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


def _check(ctx, tid, pos, flag):
    from nanopore_amd import bam
    got = bam.sort_order(ctx, tid, pos, flag)
    want = ref.stable_order(tid, pos, flag)
    assert got.tolist() == want
    return got


@pytest.mark.parametrize("n", SIZES)
def test_random_keys_with_many_ties(ctx, n):
    rng = np.random.default_rng(n)
    tid = rng.integers(-1, 3, n).astype(np.int32)          # two references and more, tid -1 mixed in
    pos = rng.integers(-1, 50, n).astype(np.int64)         # few positions: many equal keys
    flag = (rng.integers(0, 2, n) * 16 + rng.integers(0, 2, n) * 4).astype(np.int32)
    _check(ctx, tid, pos, flag)


@pytest.mark.parametrize("n", (1, 257, 4097))
def test_all_keys_equal_is_the_identity(ctx, n):
    got = _check(ctx, np.zeros(n, np.int32), np.full(n, 7, np.int64), np.zeros(n, np.int32))
    assert got.tolist() == list(range(n))


@pytest.mark.parametrize("n", (2049, 100003))
def test_sorted_and_reversed_input(ctx, n):
    pos = np.arange(n, dtype=np.int64)
    tid, flag = np.zeros(n, np.int32), np.zeros(n, np.int32)
    assert _check(ctx, tid, pos, flag).tolist() == list(range(n))
    assert _check(ctx, tid, pos[::-1].copy(), flag).tolist() == list(range(n - 1, -1, -1))


def test_extreme_positions_and_strands(ctx):
    pos = np.array([1 << 28, (1 << 29) - 1, 0, -1, 5, 5, 5, 5, (1 << 29) - 1, -1], dtype=np.int64)
    flag = np.array([0, 16, 0, 0, 16, 0, 16, 0, 0, 16], dtype=np.int32)
    tid = np.array([0, 0, 0, 0, 1, 1, 1, 1, -1, -1], dtype=np.int32)
    got = _check(ctx, tid, pos, flag)
    assert got.tolist() == [3, 2, 0, 1, 5, 7, 4, 6, 9, 8]   # POS 0 first; forward before reverse at one position, file order among equals; tid -1 last


def test_forty_references(ctx):
    rng = np.random.default_rng(40)
    n = 5000
    tid = rng.integers(-1, 40, n).astype(np.int32)
    pos = rng.integers(-1, 1 << 29, n).astype(np.int64)
    flag = (rng.integers(0, 2, n) * 16).astype(np.int32)
    pos[::7] = pos[0]
    _check(ctx, tid, pos, flag)


def test_repeat_call_is_identical(ctx):
    from nanopore_amd import bam
    rng = np.random.default_rng(5)
    n = 4097
    tid, pos, flag = rng.integers(-1, 2, n).astype(np.int32), rng.integers(0, 9, n).astype(np.int64), np.zeros(n, np.int32)
    assert bam.sort_order(ctx, tid, pos, flag).tolist() == bam.sort_order(ctx, tid, pos, flag).tolist()


def test_out_of_range_is_refused(ctx):
    from nanopore_amd import _lib, bam
    with pytest.raises(_lib.NprError):
        bam.sort_order(ctx, [-2], [0], [0])
    with pytest.raises(_lib.NprError):
        bam.sort_order(ctx, [0], [-2], [0])

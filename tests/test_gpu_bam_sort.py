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


# ---------------------------------------------------------------- wide tids, every pass count, the contract's ends
def _bits_of(v):
    return int(v).bit_length()


def _passes(tid, pos):
    """the passes npr_bam_sort_order takes, by the rule of csrc/npr_bam_api.cpp: the key tid' << 33 | (pos + 1) << 1 | reverse has
    33 + bits_of(no_tid) bits with no_tid = the largest tid + 1 (the tid' of tid -1), or, when that is 0, the bits of the largest
    (pos + 1) << 1 | 1; 8 bits a pass, one pass at least"""
    no_tid = max([int(t) for t in tid] + [-1]) + 1
    max_pos = max([int(p) + 1 for p in pos] + [0])
    bits = 33 + _bits_of(no_tid) if no_tid else _bits_of(max_pos << 1 | 1)
    return max(1, (bits + 7) // 8)


@pytest.mark.parametrize("n", (257, 2049))
def test_wide_tids(ctx, n):
    rng = np.random.default_rng(n)
    tids, poss = [-1, 0, 127, 128, 255, 256, 32767, 32768, (1 << 30) - 1], [-1, 0, (1 << 29) - 1, 1 << 29, (1 << 31) - 2]
    keys = [(t, p, f) for t in tids for p in poss for f in (0, 16)]
    pick = np.concatenate([np.arange(len(keys)), rng.integers(0, len(keys), n - len(keys))])    # every key once at least, the rest drawn: ties
    rng.shuffle(pick)
    tid = np.array([keys[k][0] for k in pick], dtype=np.int32)
    pos = np.array([keys[k][1] for k in pick], dtype=np.int64)
    flag = (np.array([keys[k][2] for k in pick]) + rng.integers(0, 2, n) * 4).astype(np.int32)
    assert _passes(tid, pos) == 8 and len(tid) == n
    _check(ctx, tid, pos, flag)


# passes -> (the largest tid, the largest pos) with which the key just fills them; -1: every record without a reference
PASS_CASES = {1: (-1, 126), 2: (-1, 32766), 3: (-1, (1 << 23) - 2), 4: (-1, (1 << 31) - 2), 5: (126, (1 << 31) - 2), 6: (32766, (1 << 29) - 1),
              7: ((1 << 23) - 2, (1 << 31) - 2), 8: ((1 << 30) - 1, (1 << 31) - 2)}


@pytest.mark.parametrize("passes", sorted(PASS_CASES))
def test_every_pass_count(ctx, passes):
    """n = 2049: two tiles.  The values drawn lie at both ends of the top digit of the last pass, around the digit edges below it, and
    repeat: ties in every pass."""
    max_tid, max_pos = PASS_CASES[passes]
    n, rng = 2049, np.random.default_rng(passes)

    def around(top):
        vals = {0, 1, top, top - 1, top // 2, top // 255} | {(1 << b) - d for b in range(7, 31, 8) for d in (0, 1)}
        return np.array(sorted(v for v in vals if 0 <= v <= top))
    tid = np.full(n, -1, dtype=np.int32) if max_tid < 0 else rng.choice(np.append(around(max_tid), -1), n).astype(np.int32)
    pos = rng.choice(np.append(around(max_pos), -1), n).astype(np.int64)
    flag = (rng.integers(0, 2, n) * 16).astype(np.int32)
    tid[5], pos[7] = max_tid, max_pos
    assert _passes(tid, pos) == passes
    largest = max((max_tid + 1) << 33, (max_pos + 1) << 1 | 1)      # (tid -1 is drawn in every case, so max_tid + 1 is a key's tid')
    assert 0 < largest >> (8 * (passes - 1)) < 256, "the last pass has a digit that is not 0, and there is no digit above it"
    _check(ctx, tid, pos, flag)


def test_the_contracts_upper_ends_are_refused(ctx):
    from nanopore_amd import _lib, bam
    for tid, pos in (([1 << 30], [0]), ([0], [(1 << 31) - 1]), ([0, 1 << 30], [5, 5]), ([0, 0], [5, (1 << 31) - 1])):
        with pytest.raises(_lib.NprError) as e:
            bam.sort_order(ctx, tid, pos, [0] * len(tid))
        assert e.value.code == _lib.ERR_INVALID
    assert bam.sort_order(ctx, [(1 << 30) - 1, 0], [(1 << 31) - 2, (1 << 31) - 2], [0, 0]).tolist() == [1, 0]

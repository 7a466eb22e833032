"""The one device prefix sum (csrc/npr_scan.h) at the sizes where it can go wrong, through the entry points that use it: the cigar text's
offsets and the pileup's word 5 (the tiled form), the seed map's and the seed chains' offsets and the SNP variants' tile offsets (the
one-workgroup form).  Tile boundaries, trip boundaries, and the tile counts at which the tiled form's middle pass needs its carry.
Every expectation is host arithmetic that shares nothing with the device scan; everything is compared as exact integers or bytes.

npr_seed_chains refuses a row of length 0, so every chain has an M and no chain has zero operations: the shortest guide there is, a
single M that covers its read and its reference, stands among the longer ones instead."""
import numpy as np
import pytest

from nanopore_amd import _lib
from nanopore_amd._lib import ptr
from seed_chain_reference import as_chains, chains_by_rule, pack
from test_gpu_pileup import _expect
from test_gpu_seed_map import _check as check_map
from test_gpu_snp_variants import HMM_ERROR_MATRIX, NULL_MATRIX, T, assert_same_variants, guarded_reference, mixed_table

pytestmark = pytest.mark.gpu

S = 2048   # SCAN_TILE of csrc/npr_scan.h: the entries one workgroup of the tiled scan takes
G = 256    # SCAN_THREADS of csrc/npr_scan.h: the entries of one trip of the one-workgroup scan (and of the tiled scan's middle pass)


# ---- cigar text: launch_scan_tiled<int64_t, int64_t> in place over the lengths ----

def _sparse_lists(n, seed):
    """n lists, all empty but a seeded few of one to three operations whose lengths have 1 and 10 digits; the first list, the last one and
    the ones around the first tile boundary are among the few."""
    rng = np.random.default_rng(seed)
    some = np.unique(np.concatenate([rng.integers(0, n, size=40), [0, S - 2, S - 1, n - 1]]))
    some = some[some < n]
    nops = np.zeros(n, dtype=np.int64)
    nops[some] = rng.integers(1, 4, size=len(some))
    woff = np.zeros(n, dtype=np.int64)
    woff[1:] = np.cumsum(nops)[:-1]
    k = int(nops.sum())
    length = np.where(rng.random(k) < 0.5, rng.integers(1, 10, size=k), rng.integers(1000000000, 1 << 30, size=k)).astype(np.uint32)
    words = (length << 2) | rng.integers(0, 3, size=k).astype(np.uint32)
    return woff, nops, words


@pytest.mark.parametrize("n", [S - 2, S - 1, S, S + 1, G * S - 1, G * S, G * S + 1])
def test_cigar_text_offsets_across_tiles(gpu_ctx, n):
    from nanopore_amd import realign as R
    woff, nops, words = _sparse_lists(n, 100 + n % 97)
    digits = np.array([len(str(int(w) >> 2)) for w in words], dtype=np.int64)
    assert set(digits) == {1, 10}
    lengths = np.ones(n, dtype=np.int64)                                # "*"
    lengths[nops > 0] = np.add.reduceat(digits + 1, woff[nops > 0])
    want, want_off = R.format_cigars_packed(woff, nops, words)
    assert np.array_equal(np.diff(want_off), lengths)                   # the host formatter's string lengths are the restated ones
    got, got_off = R.cigar_text_packed(gpu_ctx, woff, nops, words)
    assert got_off.dtype == np.int64 and np.array_equal(got_off, np.concatenate([[0], np.cumsum(lengths)]))
    assert bytes(got) == bytes(want)


# ---- pileup: k_scan_tile_sums, k_scan_group, then the unit's own last pass over the same tiles ----

def _boundary_records(ref_lengths):
    """D runs where the scan's tiles meet: one that ends with its sequence (its -1 lands in the spare slot), one across every tile boundary
    a sequence's slots contain (the first two and the last), one from the second position of the longest sequence to its last but one
    (every tile that sequence has), and a few M columns."""
    reads, cigars, ref_index, start = [], [], [], []

    def one(k, x, cigar, read=""):
        reads.append(read), cigars.append(cigar), ref_index.append(k), start.append((x, 0))

    first_slot = 0
    for k, length in enumerate(ref_lengths):
        if length >= 8:
            one(k, length - 4, [(2, 4)])
            one(k, 0, [(0, 2), (2, 3), (0, 2)], "ACGT")
            inside = [t * S - first_slot for t in range(1, (first_slot + length) // S + 1) if 3 <= t * S - first_slot <= length - 3]
            for row in inside[:2] + inside[-1:]:
                one(k, row - 3, [(0, 1), (2, 6), (0, 1)], "GT")
        first_slot += length + 1
    k = int(np.argmax(ref_lengths))
    one(k, 1, [(2, ref_lengths[k] - 2)])
    return reads, cigars, ref_index, start


@pytest.mark.parametrize("ref_lengths", [[1000, S - 3 - 1000], [S - 1], [S - 1, 0], [G * S - 1, 0], [S - 1, S, G * S - 2 * S - 1]],
                         ids=["S-1", "S", "S+1", "GS+1", "GS+1_three"])
def test_pileup_word_5_across_tiles(gpu_ctx, ref_lengths):
    """n_slots = rows + sequences.  [S - 1]: the spare slot is the last slot of a tile; [S - 1, 0] and [G S - 1, 0]: the second sequence's
    only slot, its spare one, is the first slot of the next tile; [S - 1, S, ...]: spare slots at S - 1 (the last of a tile), 2 S and G S
    (the first of one).  G S + 1 slots are G + 1 tiles: the one workgroup over the tile sums makes a second trip."""
    n_slots = sum(ref_lengths) + len(ref_lengths)
    assert n_slots in (S - 1, S, S + 1, G * S + 1)
    reads, cigars, ref_index, start = _boundary_records(ref_lengths)
    assert max(n for c in cigars for op, n in c if op == 2) == max(ref_lengths) - 2   # (in [G S - 1, 0]: a D run over G tiles)
    want = _expect(ref_lengths, reads, cigars, ref_index, start)
    assert want[:, 5].sum() > 0 and want[:, :4].sum() > 0
    pl = gpu_ctx.pileup(ref_lengths)
    try:
        pl.add(reads, cigars, ref_index, start=start)
        got = pl.counts()
        assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        depth, covered = pl.depth()
        assert np.array_equal(depth, want[:, :5].sum(axis=1)) and np.array_equal(covered, want[:, :6].sum(axis=1) != 0)
        assert np.array_equal(pl.counts(), want)                        # read again: the difference array stays what it is
        pl.add(reads, cigars, ref_index, start=start)                   # ... and accumulates
        assert np.array_equal(pl.counts(), 2 * want)
        assert np.array_equal(pl.depth()[0], 2 * want[:, :5].sum(axis=1))
    finally:
        pl.close()


# ---- seed map: launch_scan_group<uint32_t, int64_t> (hit_off), <int64_t, int64_t> in place (chain_off), and the chains' n_ops ----

@pytest.mark.parametrize("n_reads", [G - 1, G, G + 1, 4 * G + 1])
def test_seed_map_offsets_across_trips(gpu_ctx, n_reads):
    """Reads of 60 bases cut from a 3 kb reference (every third with a substitution in the middle: two rows, one chain) and random 40-mers
    that match nothing: the first two reads, the ones around the middle, the last one and every seventh."""
    import random
    rng = random.Random(n_reads)
    ref = "".join(rng.choice("ACGT") for _ in range(3000))
    nothing = {0, 1, n_reads // 2, n_reads // 2 + 1, n_reads - 1} | set(range(5, n_reads, 7))
    reads = []
    for i in range(n_reads):
        if i in nothing:
            reads.append("".join(rng.choice("ACGT") for _ in range(40)))
            continue
        at = rng.randrange(0, len(ref) - 60)
        piece = list(ref[at:at + 60])
        if i % 3 == 0:
            piece[30] = "ACGT"[("ACGT".index(piece[30]) + 1) % 4]
        reads.append("".join(piece))
    hit_off, hits, chain_off, chains, ops_off, ops = check_map(gpu_ctx, [ref], reads, 12, 16)   # the six arrays whole, against matches + seed_chains
    rows = np.diff(hit_off)
    assert all(rows[i] == 0 for i in nothing) and (rows[[i for i in range(n_reads) if i not in nothing]] >= 1).all()
    assert rows.max() >= 2 and np.array_equal(np.diff(chain_off), (rows > 0).astype(np.int64))
    assert len(hit_off) == len(chain_off) == n_reads + 1 and len(ops_off) == chain_off[-1] + 1 and ops_off[-1] == len(ops)


# ---- seed chains: launch_scan_group<int64_t, int64_t> in place over the chains' op pairs ----

@pytest.mark.parametrize("n_chains", [G, G + 1])
def test_seed_chain_offsets_across_trips(gpu_ctx, n_chains):
    """One chain per read: one to three rows on one of two references and either strand, and every fifth read the shortest guide there is."""
    import random
    rng = random.Random(n_chains)
    ref_len = [400, 300, 7]
    reads = []
    for i in range(n_chains):
        if i % 5 == 4:
            reads.append((7, [(2, 0, 0, 0, 7)]))                        # one M, nothing before or after it
            continue
        r, strand = i % 2, (i // 2) % 2
        rows = [(r, 10 + 40 * j + rng.randrange(0, 5), 12 + 40 * j + rng.randrange(0, 9), strand, rng.randrange(4, 20)) for j in range(1 + i % 3)]
        reads.append((200 + i % 11, rows))
    read_len, hit_off, hits = pack(reads)
    want = chains_by_rule(read_len, ref_len, hit_off, hits, 200)
    assert sum(len(m) for m in want) == n_chains and {len(g) for m in want for *_, g in m} >= {1, 5}
    chain_off, chains, ops_off, ops = gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, 200)
    assert np.array_equal(chain_off, np.arange(n_chains + 1))
    assert np.array_equal(ops_off, np.concatenate([[0], np.cumsum([len(g) for m in want for *_, g in m])])) and ops_off[-1] == len(ops)
    assert as_chains(chain_off, chains, ops_off, ops) == want


# ---- SNP variants: launch_scan_group<uint32_t, int64_t> over the tiles' call counts ----

@pytest.mark.parametrize("where", ["first_tile", "last_tile", "every_tile"])
@pytest.mark.parametrize("rows", [T * (G - 1) + 1, T * G, T * G + 1])
def test_snp_variant_offsets_across_trips(gpu_ctx, rows, where):
    """G - 1 + 1, G and G + 1 tiles of T rows.  Calls in one tile alone leave every other tile's offset equal to its neighbour's."""
    tiles = (rows + T - 1) // T
    variant_rows = {"first_tile": np.arange(3, T, 5), "last_tile": np.arange((tiles - 1) * T, rows), "every_tile": np.append(np.arange(3, rows, 16), rows - 1)}[where]
    weights, seen, ref = mixed_table(rows, rows, variant_rows=variant_rows)
    if where != "first_tile":   # (the last tile of T (G - 1) + 1 and T G + 1 rows is one row: an ordinary one)
        weights[rows - 1], seen[rows - 1], ref[rows - 1] = (1.0, 40.0, 2.0, 0.5), True, 0
    want = guarded_reference(weights, seen, ref, HMM_ERROR_MATRIX, 0.5)
    called = np.unique(want["call_row"] // T)
    assert {"first_tile": [0], "last_tile": [tiles - 1], "every_tile": list(range(tiles))}[where] == called.tolist()
    assert_same_variants(gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5), want)


# ---- nothing to sum ----

def test_empty_inputs(gpu_ctx):
    """Zero lists, zero reads, zero chains: offsets of length 1 holding 0."""
    off = np.full(1, -7, dtype=np.int64)
    z64, z32 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint32)
    assert _lib.load().npr_cigar_text_packed(gpu_ctx._h, 0, ptr(z64), ptr(z64), ptr(z32), ptr(off), None, 0) == 0 and off[0] == 0
    ref = "ACGTTGCAAGGCTTAACCGGATCGATTACAGGCATCGGA" * 5
    out = check_map(gpu_ctx, [ref], [], 12, 16)                        # no reads
    assert [a.tolist() for a in (out[0], out[2], out[4])] == [[0], [0], [0]] and [len(out[i]) for i in (1, 3, 5)] == [0, 0, 0]
    out = check_map(gpu_ctx, [ref], ["T" * 10 + "G" * 10 + "C" * 10 + "A" * 10, ""], 12, 16)         # reads without a row: no chain
    assert out[0].tolist() == [0, 0, 0] and out[2].tolist() == [0, 0, 0] and out[4].tolist() == [0]
    read_len, hit_off, hits = pack([])
    chain_off, chains, ops_off, ops = gpu_ctx.seed_chains(read_len, [10], hit_off, hits, 200)
    assert chain_off.tolist() == [0] and ops_off.tolist() == [0] and len(chains) == 0 and len(ops) == 0

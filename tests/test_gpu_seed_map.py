"""The device-resident seed map (include/nprealign.h: npr_seed_map_*; csrc/npr_seedmap.hip): SeedIndex.map against the two calls it
stands for, SeedIndex.matches followed by Context.seed_chains, array for array -- and the fused SeedMapper against the unfused one, file
for file."""
import ctypes
import os
import random

import numpy as np
import pytest

from helpers import ROOT
from seed_mapper import revcomp
from seed_reference import DictionaryOracle

pytestmark = pytest.mark.gpu

C1 = os.path.join(ROOT, "tests", "golden", "c1")
NAMES = ("hit_off", "hits", "chain_off", "chains", "ops_off", "ops")


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _spans(reads):
    """reads -> (uint8 text with a few bytes of other text between the reads, begin, end)"""
    text, begin, end = b"", [], []
    for r in reads:
        text += b"\n@x\n"
        begin.append(len(text))
        text += r.encode()
        end.append(len(text))
    return np.frombuffer(text + b"\n", dtype=np.uint8), np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def _two_calls(ctx, index, refs, text, begin, end, min_len, strands, max_gap):
    hit_off, hits = index.matches(text, begin, end, min_len, strands)
    return (hit_off, hits) + tuple(ctx.seed_chains(end - begin, [len(r) for r in refs], hit_off, hits, max_gap))


def _same(got, want):
    assert len(got) == len(want) == 6
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def _check(ctx, refs, reads, k, min_len, strands=3, max_gap=200, **kw):
    """SeedIndex.map == matches + seed_chains on the same input; -> the arrays"""
    text, begin, end = _spans(reads)
    index = ctx.seed_index(refs, k)
    try:
        want = _two_calls(ctx, index, refs, text, begin, end, min_len, strands, max_gap)
        got = index.map(text, begin, end, min_len, strands, max_gap, rows=True, **kw)
        _same(got, want)
        short = index.map(text, begin, end, min_len, strands, max_gap, **kw)      # rows=False: the last four
        assert len(short) == 4 and all(np.array_equal(s, w) for s, w in zip(short, want[2:]))
    finally:
        index.close()
    return want


@pytest.fixture(scope="module")
def edge():
    """Two references and, in this order: an empty read, one shorter than k, one without a match, one with exactly one row, one with hits
    on the forward strand only, one with hits on the reverse strand only, one with hits on both references, one with both strands."""
    rng = random.Random(5)
    refs = [_rand(rng, 900), _rand(rng, 500)]

    def noisy(piece, step):  # a substitution every `step` bases: several rows on one diagonal
        piece = list(piece)
        for q in range(step // 2, len(piece), step):
            piece[q] = "ACGT"[("ACGT".index(piece[q]) + 1) % 4]
        return "".join(piece)

    reads = ["", refs[0][10:21], _rand(rng, 300), _rand(rng, 40) + refs[0][100:130] + _rand(rng, 40), noisy(refs[0][200:600], 45),
             revcomp(noisy(refs[1][50:450], 50)), noisy(refs[0][600:850], 40) + _rand(rng, 30) + noisy(refs[1][300:480], 35),
             noisy(refs[0][300:500], 60) + revcomp(refs[0][640:800])]
    return refs, reads


@pytest.mark.parametrize("strands", [3, 1, 2])
def test_hand_made_and_edge_reads(gpu_ctx, edge, strands):
    refs, reads = edge
    hit_off, hits, chain_off, chains, ops_off, ops = _check(gpu_ctx, refs, reads, 12, 16, strands)
    rows, n_chains = np.diff(hit_off), np.diff(chain_off)
    assert rows[:3].tolist() == [0, 0, 0] and n_chains[:3].tolist() == [0, 0, 0]
    if strands & 1:
        assert rows[3] == 1 and n_chains[3] == 1 and rows[4] >= 5 and n_chains[6] == 2 and rows[6] >= 6
    else:
        assert rows[3] == 0 and rows[4] == 0
    if strands & 2:
        assert rows[5] >= 5 and n_chains[5] == 1 and chains[chain_off[5], 1] == 1
    else:
        assert rows[5] == 0
    if strands == 3:   # read 4 forward only, read 5 reverse only, read 7 rows on both strands of one reference: one chain
        strand = lambda i: set((hits[hit_off[i]:hit_off[i + 1], 2].astype(np.int64) & 0xffffffff) >> 31)  # noqa: E731
        assert strand(4) == {0} and strand(5) == {1} and strand(7) == {0, 1} and n_chains[7] == 1
        assert set(hits[hit_off[6]:hit_off[6 + 1], 0]) == {0, 1}


def test_nothing_at_all(gpu_ctx, edge):
    """No reads; and reads none of which has a row: empty, well-formed arrays."""
    refs, reads = edge
    for none in ([], reads[:3]):
        out = _check(gpu_ctx, refs, none, 12, 16)
        assert not out[0].any() and not out[2].any() and out[4].tolist() == [0] and [len(out[i]) for i in (1, 3, 5)] == [0, 0, 0]
    _check(gpu_ctx, [], reads, 12, 16)   # ... and an index without a reference


# ---- both tiers of the sort, and their boundary ----

def test_both_sort_tiers_and_the_boundary(gpu_ctx):
    """c copies of a 24-mer in a reference of its own against d copies in a read: c * d rows, every one the 24-mer (the bases between the
    copies are A / C in the reference and G / T in the read: no match extends).  One read a row below what the LDS tier holds, one at it,
    one a row above, one of 80 x 80 rows; unrelated reads among them."""
    from nanopore_amd import _lib
    limit = _lib.SEED_MAP_LDS_ROWS
    shapes = [(63, 65), (64, 64), (17, 241), (80, 80)]
    assert [c * d for c, d in shapes] == [limit - 1, limit, limit + 1, 6400]
    rng = random.Random(77)
    refs, big = [], []
    for c, d in shapes:
        unit = _rand(rng, 24)
        refs.append("".join(unit + "AC"[i % 2] for i in range(c)))
        big.append("".join(unit + "GT"[j % 2] for j in range(d)))
    # the row counts are what this test assumes, by the dictionary oracle on the CPU: c * d forward, none on the other strand or reference
    for i, (c, d) in enumerate(shapes):
        for r, ref in enumerate(refs):
            oracle = DictionaryOracle(ref, 16)
            assert len(oracle.matches(big[i], 20)) == (c * d if r == i else 0) and not oracle.matches(revcomp(big[i]), 20)
    other = _rand(rng, 2000)
    refs.append(other)
    reads = [other[100:400], big[0], revcomp(other[900:1300]), big[1], big[2], "", big[3], other[1500:1900]]
    hit_off, hits = _check(gpu_ctx, refs, reads, 16, 20)[:2]
    assert np.diff(hit_off).tolist() == [1, limit - 1, 1, limit, limit + 1, 0, 6400, 1]
    assert (hits[hit_off[6]:hit_off[7], 3] == 24).all()


def test_a_homopolymer_run_of_a_thousand_rows(gpu_ctx):
    refs, reads = ["C" + "A" * 1000 + "G"], ["A" * 40, "ACGTACGTAGCTAGCTAGGATCGATCGAT"]
    hit_off = _check(gpu_ctx, refs, reads, 12, 20)[0]
    assert 900 <= hit_off[1] <= 1100 and hit_off[2] == hit_off[1]


def test_200_reads_against_a_megabase(gpu_ctx):
    """Reads of about 2 kb through an error channel, either strand, against a random megabase (as test_gpu_seed_chain makes them)."""
    rng = random.Random(23)
    ref = "".join(rng.choice("ACGT") for _ in range(1000000))
    reads = []
    for i in range(200):
        s = rng.randrange(0, len(ref) - 2100)
        out = []
        for c in ref[s:s + rng.randrange(1800, 2200)]:
            r = rng.random()
            if r < 0.05:
                out.append(rng.choice("ACGT"))
            elif r < 0.08:
                continue
            elif r < 0.11:
                out.append(c)
                out.append(rng.choice("ACGT"))
            else:
                out.append(c)
        reads.append(revcomp("".join(out)) if i % 2 else "".join(out))
    hit_off, hits, chain_off, chains, ops_off, ops = _check(gpu_ctx, [ref], reads, 16, 20)
    assert len(hits) >= 1000 and len(chains) >= 190 and sum(int(chains[chain_off[i], 1]) == i % 2 for i in range(200) if chain_off[i + 1] > chain_off[i]) >= 190


def test_chunks_give_the_same_arrays(gpu_ctx, edge):
    from nanopore_amd.realign import SeedIndex
    refs, reads = edge
    reads = reads + reads[3:]
    text, begin, end = _spans(reads)
    chunk_bases = int((end - begin).sum()) // 3 + 150
    assert len(SeedIndex._chunks("test", text, begin, end, chunk_bases)[3]) == 3
    whole = _check(gpu_ctx, refs, reads, 12, 16)
    assert len(whole[3]) >= 8
    _same(_check(gpu_ctx, refs, reads, 12, 16, chunk_bases=chunk_bases), whole)


# ---- the C ABI as it stands ----

def _create(index, min_len, strands, max_gap, text, begin, end):
    from nanopore_amd import _lib
    h = ctypes.c_void_p(0x5a5a)
    rc = _lib.load().npr_seed_map_create(index._h, min_len, strands, max_gap, len(begin), _lib.ptr(text), _lib.ptr(begin), _lib.ptr(end), ctypes.byref(h))
    return rc, h


def test_refused_arguments_make_no_map(gpu_ctx):
    from nanopore_amd import _lib
    ref = "ACGTTGCAAGGCTAGGATCCATGCAATCGGA"
    text, begin, end = _spans([ref, ref[3:25]])
    backwards = end.copy()
    backwards[1] = begin[1] - 1
    # 2048 spans of one megabyte of text: 2^31 read bases in one call, without holding them
    mega = np.zeros(1 << 20, dtype=np.uint8)
    many_b, many_e = np.zeros(2048, dtype=np.int64), np.full(2048, 1 << 20, dtype=np.int64)
    index = gpu_ctx.seed_index([ref], 12)
    try:
        for min_len, strands, max_gap, t, b, e in ((11, 3, 200, text, begin, end), (1 << 31, 3, 200, text, begin, end), (12, 0, 200, text, begin, end),
                                                   (12, 4, 200, text, begin, end), (12, 3, -1, text, begin, end), (12, 3, 200, text, begin, backwards),
                                                   (12, 3, 200, mega, many_b, many_e)):
            rc, h = _create(index, min_len, strands, max_gap, t, b, e)
            assert rc == _lib.ERR_INVALID and h.value is None, (min_len, strands, max_gap)
        rc, h = _create(index, 12, 3, 200, text, begin, end)
        assert rc == _lib.OK and h.value
        _lib.load().npr_seed_map_destroy(h)
    finally:
        index.close()


def test_a_map_fetched_twice_gives_the_same_bytes(gpu_ctx, edge):
    from nanopore_amd.realign import SeedMap
    refs, reads = edge
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index(refs, 12)
    try:
        m = SeedMap(index, text, begin, end, 16, 3, 200)
        index.close()                      # (the map does not need its index any more)
        first, second = m.fetch(), m.fetch()
        assert m.counts() == (len(first[1]), len(first[3]), len(first[5])) and m.counts()[1] >= 5
        assert all(a.tobytes() == b.tobytes() for a, b in zip(first, second))
        assert all(np.array_equal(a, b) for a, b in zip(m.fetch(rows=False), first[2:]))
        m.close()
        m.close()
    finally:
        index.close()


def test_closing_the_context_closes_an_open_map(edge):
    from nanopore_amd import realign
    refs, reads = edge
    text, begin, end = _spans(reads)
    ctx = realign.Context(0)
    index = ctx.seed_index(refs, 12)
    m = realign.SeedMap(index, text, begin, end, 16)
    assert m.counts()[0] > 0
    ctx.close()
    assert m._h is None and index._h is None
    m.close()


# ---- the fused SeedMapper against the unfused one, byte for byte ----

def _three_files(tmp, fq, fa, k, min_len, fused):
    """(seed SAM, chained SAM, realigned SAM) of SeedMapper, SeedMapperChain, SeedMapperRealign"""
    from nanopore_amd.mappers import variants as V
    out = []
    for cls in (V.SeedMapper, V.SeedMapperChain, V.SeedMapperRealign):
        path = str(tmp / ("%s_%d.sam" % (cls.__name__, fused)))
        mapper = cls(fq, "2D", fa, path)
        mapper.k, mapper.minLength, mapper.fused = k, min_len, fused
        mapper.run()
        if fused:
            assert not os.path.exists(os.path.join(mapper.getGlobalTempDir(), "temp.sam"))
        elif cls is V.SeedMapperRealign:
            assert os.path.exists(os.path.join(mapper.getGlobalTempDir(), "temp.sam"))   # (what the fused path leaves out)
        mapper.cleanup()
        out.append(open(path, "rb").read())
    return out


def _fused_equals_unfused(tmp, fq, fa, k, min_len, records):
    want, got = _three_files(tmp, fq, fa, k, min_len, False), _three_files(tmp, fq, fa, k, min_len, True)
    for name, g, w in zip(("seed", "chained", "realigned"), got, want):
        assert g == w, name
    assert want[0] != want[1] != want[2] and want[1].count(b"\n") == want[2].count(b"\n") >= records
    return want


def test_fused_seed_mapper_on_c1(gpu_ctx, tmp_path):
    from nanopore_amd import bioio
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as fh:
        for n, s, _ in bioio.fastqRead(os.path.join(C1, "reads.fq")):
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    _fused_equals_unfused(tmp_path, fq, os.path.join(C1, "reference.fa"), 18, 24, 3)


def test_fused_seed_mapper_on_two_references_and_both_strands(gpu_ctx, tmp_path):
    """(the input of test_gpu_seed_chain's test of the same name: substitutions, deletions and insertions every few dozen bases, a read in
    lower case, one with chains on both references, one that matches nothing, names out of FASTQ order)"""
    rng = random.Random(41)
    refs = [_rand(rng, n) for n in (3000, 1800)]
    reads = []
    for i in range(12):
        ref = refs[i % 2]
        s = rng.randrange(0, len(ref) - 700)
        piece = list(ref[s:s + rng.randrange(400, 700)])
        for q in range(rng.randrange(5, 30), len(piece), rng.randrange(25, 60)):
            kind = rng.randrange(3)
            piece[q] = "ACGT"[("ACGT".index(piece[q]) + 1) % 4] if kind == 0 else ("" if kind == 1 else piece[q] + rng.choice("ACGT"))
        read = "".join(piece)
        if i == 5:
            read = read.lower()
        if i == 7:
            read = read[:200] + refs[0][100:400]
        reads.append(revcomp(read) if i % 3 == 1 else read)
    reads.append(_rand(rng, 300))
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq")
    with open(fa, "w") as fh:
        for k, ref in enumerate(refs):
            fh.write(">contig_%d some description\n%s\n" % (k, ref))
    with open(fq, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@r%02d extra words\n%s\n+\n%s\n" % ((7 * i) % 13, r, "I" * len(r)))
    seed, chained, realigned = _fused_equals_unfused(tmp_path, fq, fa, 12, 14, 15)
    flags = [rec.split(b"\t")[1] for rec in realigned.split(b"\n")[2:-1]]
    assert len(flags) >= 13 and flags.count(b"16") >= 4 and flags.count(b"0") >= 8

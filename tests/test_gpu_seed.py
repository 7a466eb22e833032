"""Exact-match seeding on the device (csrc/npr_seed.hip behind npr_seed_index_create / npr_seed_matches) and the SeedMapper classes
on top of it.  Everything is compared as exact integers or bytes."""
import os
import random

import numpy as np
import pytest

from helpers import ROOT, cigar_spans
from seed_mapper import revcomp, write_local_hits_sam
from seed_reference import DictionaryOracle, as_rows, rows_by_definition

pytestmark = pytest.mark.gpu

C1 = os.path.join(ROOT, "tests", "golden", "c1")


def _rand(rng, n):
    return "".join(rng.choice("ACGT") for _ in range(n))


def _spans(reads):
    """reads -> (uint8 text with a byte of other text between the reads, begin, end)"""
    text, begin, end = b"", [], []
    for r in reads:
        text += b"\n@x\n"
        begin.append(len(text))
        text += r.encode()
        end.append(len(text))
    return np.frombuffer(text + b"\n", dtype=np.uint8), np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


@pytest.fixture(scope="module")
def small():
    """Reference sequences and reads for every k at once, and what the definition says about them at min_len 8 (a match of a
    larger min_len is one of these).  The reads: lengths 0, k - 1, k for every k tested, 63 / 64 / 65 (a wavefront and one lane
    either side), 8191 / 8193 (33 workgroups of read positions, the last one nearly empty); matches at reference position 0, at a
    reference's last base, at a read's first and last base; the last 40 bases of reference 0 followed by the first 40 of reference
    1 (two matches, never one of 80); N at the same place in read and reference; lower case; A * 30 against A * 200 (a bucket of
    189 positions at k = 12, and a read position for every case of the start rule: i = 0 of its sequence, j = 0, the bases before
    equal, the bases before different); a block of 500 bases the reference holds twice; some reads reverse-complemented."""
    rng = random.Random(11)
    ref0, ref1 = _rand(rng, 9000), _rand(rng, 700)
    block = _rand(rng, 500)
    with_n = _rand(rng, 60) + "N" + _rand(rng, 60)
    refs = [ref0, ref1, _rand(rng, 7), _rand(rng, 20), "C" + "A" * 200 + "G", with_n, block + _rand(rng, 50) + block, ""]
    reads = [""]
    for n in (7, 8, 11, 12, 13, 15, 16, 31, 32, 63, 64, 65):
        s = rng.randrange(0, 600)
        reads.append(ref1[s:s + n])
    for n, s in ((8191, 300), (8193, 700)):  # a long stretch of reference 0 with a substitution every ~150 bases
        r = list(ref0[s:s + n])
        for q in range(70, n, 150):
            r[q] = "ACGT"[("ACGT".index(r[q]) + 1) % 4]
        reads.append("".join(r))
    reads += [ref0[:60] + _rand(rng, 20), _rand(rng, 20) + ref0[-60:], _rand(rng, 20) + ref0[300:360], ref0[400:460] + _rand(rng, 20),
              ref0[-40:] + ref1[:40], with_n[10:110], with_n[10:60] + "NN" + with_n[62:110], ref1[100:200].lower(), "A" * 30, "T" * 30, block,
              revcomp(ref0[5000:5400]), revcomp(ref1[-300:]), ref1]
    want8 = [rows_by_definition(refs, r, 8) for r in reads]
    two = [row for row in want8[reads.index(ref0[-40:] + ref1[:40])] if row[3] >= 37 and row[2] < (1 << 31)]
    assert [(r, a, b, n) for r, a, b, n in two] == [(0, 8960, 0, 40), (1, 0, 40, 40)]
    return refs, reads, want8


@pytest.mark.parametrize("k", [8, 12, 13, 16, 32])
def test_small_shapes_against_the_definition(gpu_ctx, small, k):
    refs, reads, want8 = small
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index(refs, k)
    try:
        for min_len in (k, k + 5):
            hit_off, hits = index.matches(text, begin, end, min_len, 3)
            assert hit_off[0] == 0 and hit_off[-1] == len(hits)
            n_total = 0
            for i in range(len(reads)):
                want = [row for row in want8[i] if row[3] >= min_len]
                assert as_rows(hits[hit_off[i]:hit_off[i + 1]]) == want, (k, min_len, i, len(reads[i]))
                n_total += len(want)
            assert n_total > 40
            # one strand at a time gives the two halves
            fo, fh = index.matches(text, begin, end, min_len, 1)
            ro, rh = index.matches(text, begin, end, min_len, 2)
            for i in range(len(reads)):
                assert as_rows(fh[fo[i]:fo[i + 1]]) + as_rows(rh[ro[i]:ro[i + 1]]) == as_rows(hits[hit_off[i]:hit_off[i + 1]])
        # the same reads in chunks of a few hundred bases: the chunks' rows put together are the rows of one call
        co, ch = index.matches(text, begin, end, k, 3, chunk_bases=300)
        ho, hh = index.matches(text, begin, end, k, 3)
        assert (co == ho).all() and (ch == hh).all()
    finally:
        index.close()


@pytest.fixture(scope="module")
def megabase():
    rng = random.Random(23)
    ref = _rand(rng, 1000000)
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
    oracle = DictionaryOracle(ref, 16)
    want = []
    for r in reads:
        want.append(oracle.matches(r, 20) + [(k, a, b | (1 << 31), n) for k, a, b, n in oracle.matches(revcomp(r), 20)])
    return ref, reads, want


def test_a_megabase_reference_and_200_reads(gpu_ctx, megabase):
    """Thousands of workgroups of read positions against an index of a million positions; the dictionary oracle decides."""
    ref, reads, want = megabase
    assert sum(len(w) for w in want) >= 1000
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index([ref], 16)
    try:
        hit_off, hits = index.matches(text, begin, end, 20, 3)
    finally:
        index.close()
    assert hit_off[-1] == len(hits) == sum(len(w) for w in want)
    for i in range(len(reads)):
        assert as_rows(hits[hit_off[i]:hit_off[i + 1]]) == want[i], i


def _raw_matches(index, min_len, strands, text, begin, end, cap, guard=0x5a5a5a5a):
    """npr_seed_matches as it stands: (return value, hit_off, the buffer of cap rows and one guard row behind them)"""
    from nanopore_amd._lib import ptr
    hit_off = np.full(len(begin) + 1, -7, dtype=np.int64)
    rows = np.full((cap + 1, 4), guard, dtype=np.int32)
    rc = index._L.npr_seed_matches(index._h, min_len, strands, len(begin), ptr(text), ptr(begin), ptr(end), ptr(hit_off), ptr(rows), cap)
    return rc, hit_off, rows


def test_capacity(gpu_ctx, small):
    from nanopore_amd import _lib
    refs, reads, _ = small
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index(refs, 12)
    try:
        want_off, want = index.matches(text, begin, end, 12, 3)
        total = len(want)
        assert total > 40
        rc, off, rows = _raw_matches(index, 12, 3, text, begin, end, total - 1)
        assert rc == _lib.ERR_CAPACITY and (off == want_off).all() and (rows == 0x5a5a5a5a).all()   # the offsets complete, nothing written
        rc, off, rows = _raw_matches(index, 12, 3, text, begin, end, total)
        assert rc == total and (off == want_off).all() and (rows[:total] == want).all() and (rows[total] == 0x5a5a5a5a).all()
        rc, off, rows = _raw_matches(index, 12, 3, text, begin, end, 3 * total)
        assert rc == total and (off == want_off).all() and (rows[:total] == want).all() and (rows[total:] == 0x5a5a5a5a).all()
        again_off, again = index.matches(text, begin, end, 12, 3)
        assert (again_off == want_off).all() and (again == want).all()
    finally:
        index.close()


def test_nothing_to_match(gpu_ctx):
    """No reads, empty reads, reads and references shorter than k, an index without sequences: legal, and no rows."""
    text, begin, end = _spans(["", "ACGTACG", "ACGTACGTACGTACGT"])
    for refs in ([], [""], ["ACGTACG"]):
        index = gpu_ctx.seed_index(refs, 8)
        try:
            off, hits = index.matches(text, begin, end, 8, 3)
            assert (off == 0).all() and len(off) == 4 and hits.shape == (0, 4)
            off, hits = index.matches(text, begin[:0], end[:0], 8, 3)
            assert (off == 0).all() and len(off) == 1 and hits.shape == (0, 4)
        finally:
            index.close()


def test_invalid_arguments(gpu_ctx):
    from nanopore_amd import _lib
    for k in (7, 33, 0, -1):
        with pytest.raises(_lib.NprError) as e:
            gpu_ctx.seed_index(["ACGTACGTACGTACGTACGT"], k)
        assert e.value.code == _lib.ERR_INVALID
    ref = "ACGTTGCAAGGCTAGGATCCATGCAATCGGA"
    text, begin, end = _spans([ref, ref[3:25]])
    index = gpu_ctx.seed_index([ref], 12)
    try:
        ok, off, rows = _raw_matches(index, 12, 3, text, begin, end, 8)
        assert ok == 2 and list(off) == [0, 1, 2]
        backwards = end.copy()
        backwards[1] = begin[1] - 1
        for min_len, strands, e in ((11, 3, end), (1 << 31, 3, end), (12, 0, end), (12, 4, end), (12, -1, end), (12, 3, backwards)):
            rc, off, rows = _raw_matches(index, min_len, strands, text, begin, e, 8)
            assert rc == _lib.ERR_INVALID, (min_len, strands)
            assert (off == -7).all() and (rows == 0x5a5a5a5a).all()   # outputs untouched
    finally:
        index.close()


@pytest.fixture(scope="module")
def c1_files(tmp_path_factory):
    """The c1 fixture's two reads and its reference, and the stand-in's local hits of them (both strands, k 18, min_len 24)."""
    from nanopore_amd import bioio
    d = tmp_path_factory.mktemp("seed_c1")
    reads = [(n.split()[0], s) for n, s, _ in bioio.fastqRead(os.path.join(C1, "reads.fq"))]
    rname, rseq = next(iter(bioio.fastaRead(os.path.join(C1, "reference.fa"))))
    fq = str(d / "reads.fq")
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    stand_in = str(d / "stand_in.sam")
    assert write_local_hits_sam(stand_in, {rname.split()[0]: rseq}, dict(reads), k=18, min_len=24, both_strands=True) >= 2
    return d, fq, os.path.join(C1, "reference.fa"), stand_in


def _keys(path):
    from nanopore_amd import sam
    from nanopore_amd.analyses.utils import clipLengths
    f = sam.Samfile(path, "r")
    header = list(f.header_lines)
    return header, sorted((a.qname, a.flag, f.getrname(a.rname), a.pos, sum(n for op, n in a.cigar if op == 0), clipLengths(a)) for a in f)


def test_seed_mapper_names_the_stand_ins_hits(gpu_ctx, c1_files):
    from nanopore_amd.mappers.seedMapper import SeedMapper
    d, fq, fa, stand_in = c1_files
    out = str(d / "seed.sam")
    mapper = SeedMapper(fq, "2D", fa, out)
    mapper.k, mapper.minLength = 18, 24
    mapper.run()
    mapper.cleanup()
    want_header, want = _keys(stand_in)
    header, got = _keys(out)
    assert header == want_header and got == want and len(got) >= 2


def test_seed_mapper_chain_is_the_stand_ins_chain_byte_for_byte(gpu_ctx, c1_files):
    from nanopore_amd.analyses import utils
    from nanopore_amd.mappers import variants as V
    d, fq, fa, stand_in = c1_files
    want = str(d / "stand_in_chained.sam")
    utils.chainSamFile(stand_in, want, fq, fa)
    out = str(d / "seed_chained.sam")
    mapper = V.SeedMapperChain(fq, "2D", fa, out)
    mapper.k, mapper.minLength = 18, 24
    mapper.run()
    mapper.cleanup()
    assert open(out, "rb").read() == open(want, "rb").read()


def test_seed_mapper_realign_end_to_end(gpu_ctx, tmp_path):
    """FASTQ + FASTA -> realigned mapping.sam with nothing but the device: four ~1 kb reads through a mild error channel."""
    from nanopore_amd import bioio, sam, synth
    from nanopore_amd.mappers import variants as V
    rng = np.random.default_rng(17)
    T = np.zeros((5, 5))
    T[0] = [0.94, 0.03, 0.03, 0.0, 0.0]
    T[1] = [0.7, 0.3, 0, 0, 0]
    T[2] = [0.7, 0, 0.3, 0, 0]
    T[3] = T[4] = [1.0, 0, 0, 0, 0]
    E = np.full(80, 1.0 / 16.0)
    E[:16] = (np.full((4, 4), 0.06 / 12) + np.eye(4) * (0.235 - 0.06 / 12)).reshape(-1)
    ref = rng.integers(0, 4, size=1200).astype(np.uint8)
    n = 4
    rc, roff, _, _ = synth.error_channel(rng, np.tile(ref[100:1100], n), np.arange(n + 1, dtype=np.int64) * 1000, T.reshape(-1), E)
    reads = ["".join("ACGT"[c] for c in rc[roff[i]:roff[i + 1]]) for i in range(n)]
    reads[1], reads[3] = revcomp(reads[1]), revcomp(reads[3])
    fa, fq, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), str(tmp_path / "mapping.sam")
    bioio.fastaWrite(fa, "chr synthetic", "".join("ACGT"[c] for c in ref))
    with open(fq, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@read_%d some text\n%s\n+\n%s\n" % (i, r, "I" * len(r)))
    mapper = V.SeedMapperRealignTrainedModel(fq, "2D", fa, out)
    mapper.k, mapper.minLength = 12, 14
    mapper.run()  # (raises when a record's realignment fails: every status is 0 from here on)
    mapper.cleanup()
    recs = list(sam.Samfile(out, "r"))
    assert sorted(a.qname for a in recs) == ["read_%d" % i for i in range(n)]
    for a in recs:
        i = int(a.qname.split("_")[1])
        assert cigar_spans(a.cigar) == (len(ref), len(reads[i]))
        assert a.is_reverse == bool(i % 2) and a.pos == 0
        assert a.seq == (revcomp(reads[i]) if i % 2 else reads[i])

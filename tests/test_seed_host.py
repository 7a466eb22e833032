"""Exact-match seeding, the parts that need no GPU: the definition restated against the test suite's stand-in mapper, the SAM
records of npr_seed_sam_text byte for byte, the mapper classes."""
import os
import random

import numpy as np
import pytest

from helpers import ROOT  # noqa: F401  (puts the repository on sys.path)
from seed_mapper import maximal_exact_matches, revcomp
from seed_reference import matches_by_definition, rows_by_definition


def _cases():
    """30 reference / read pairs: repeats and a homopolymer in every third reference, the read a stretch of the reference through a
    5 % substitution / 3 % deletion / 3 % insertion channel, every other one reverse-complemented."""
    rng = random.Random(5)
    for trial in range(30):
        n = rng.choice([300, 2000, 6000])
        ref = "".join(rng.choice("ACGT") for _ in range(n))
        if trial % 3 == 0:
            ref = ref[:n // 2] + ref[n // 4:n // 2] + "A" * 40 + ref[n // 2:]
        a = rng.randrange(0, len(ref) // 2)
        b = a + rng.randrange(50, len(ref) // 2)
        out = []
        for c in ref[a:b]:
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
        read = "".join(out)
        yield ref, revcomp(read) if trial % 2 else read


def test_definition_equals_the_stand_in_on_acgt_input():
    """90 cases x both strands: (k, min_len) in (8, 8), (11, 14), (16, 20).  The definition has no k: a match is min_len >= k long,
    so the stand-in's k-mer lookup finds every one."""
    total = 0
    for ref, read in _cases():
        for q in (read, revcomp(read)):
            all8 = matches_by_definition([ref], q, 8)
            assert len(all8) == len(set(all8))
            for k, m in ((8, 8), (11, 14), (16, 20)):
                want = maximal_exact_matches(ref, q, k, m)
                got = [(a, b, n) for _, a, b, n in all8 if n >= m]
                assert got == want, (k, m, len(got), len(want))
                total += len(got)
    assert total > 1000


def test_definition_rules():
    """A code 4 matches nothing, not even itself; letter case does not matter; nothing crosses two reference sequences."""
    core = "ACGTTGCAAGGCTA"
    assert matches_by_definition([core + "N" + core], core + "N" + core, 8) == [(0, 0, 0, 14), (0, 0, 15, 14), (0, 15, 0, 14), (0, 15, 15, 14)]
    assert matches_by_definition([core.lower()], core, 8) == [(0, 0, 0, 14)]
    assert matches_by_definition([core[:8], core[8:] + core[:2]], core + core[:2], 8) == [(0, 0, 0, 8), (1, 0, 8, 8)]
    assert rows_by_definition([core], revcomp(core), 8) == [(0, 0, (1 << 31), 14)]


FASTQ = b"@r1 first read\nACGTACGTAC\n+\nIIIIIIIIII\n@r2\nacgtTTGGcc\n+\nIIIIIIIIII\n"
# (read, reference index, a, b, reverse, L) and the record each must give
RECORDS = [
    (0, 0, 4, 0, 0, 4, b"r1\t0\tchrA\t5\t255\t4M6H\t*\t0\t0\tACGT\t*\n"),             # at the read's start: no leading clip
    (0, 0, 7, 0, 0, 10, b"r1\t0\tchrA\t8\t255\t10M\t*\t0\t0\tACGTACGTAC\t*\n"),        # the whole read
    (0, 1, 0, 6, 0, 4, b"r1\t0\tchr_B\t1\t255\t6H4M\t*\t0\t0\tGTAC\t*\n"),             # at the read's end, second reference
    (0, 0, 2, 1, 1, 5, b"r1\t16\tchrA\t3\t255\t1H5M4H\t*\t0\t0\tTACGT\t*\n"),          # reverse: GTACGTACGT[1:6]
    (1, 1, 9, 2, 0, 6, b"r2\t0\tchr_B\t10\t255\t2H6M2H\t*\t0\t0\tgtTTGG\t*\n"),        # letters as in the FASTQ
    (1, 1, 122, 3, 1, 4, b"r2\t16\tchr_B\t123\t255\t3H4M3H\t*\t0\t0\tCAAa\t*\n"),      # reverse of a mixed-case read: ggCCAAacgt[3:7]
]


def _fastq_spans():
    names = np.array([[FASTQ.index(b"r1"), FASTQ.index(b"r1") + 2], [FASTQ.index(b"@r2") + 1, FASTQ.index(b"@r2") + 3]], dtype=np.int64)
    seqs = np.array([[FASTQ.index(b"ACGTACGTAC"), FASTQ.index(b"ACGTACGTAC") + 10], [FASTQ.index(b"acgtTTGGcc"), FASTQ.index(b"acgtTTGGcc") + 10]],
                    dtype=np.int64)
    return names, seqs


def _sam_text():
    from nanopore_amd import realign
    names, seqs = _fastq_spans()
    hits = np.array([[r, a, b | (rev << 31), n] for _, r, a, b, rev, n, _ in RECORDS], dtype=np.int64).astype(np.uint32).view(np.int32)
    hit_off = np.array([0, 4, 6], dtype=np.int64)
    text = np.frombuffer(FASTQ, dtype=np.uint8)
    return realign.seed_sam_text(text, names, seqs[:, 0].copy(), seqs[:, 1].copy(), [b"chrA", b"chr_B"], hit_off, hits)


def test_sam_text_against_hand_written_records():
    buf, off = _sam_text()
    assert [bytes(buf[off[q]:off[q + 1]]) for q in range(len(RECORDS))] == [r[-1] for r in RECORDS]
    assert off[-1] == len(buf) == sum(len(r[-1]) for r in RECORDS)


def test_sam_text_capacity_and_invalid_rows():
    from nanopore_amd import _lib
    from nanopore_amd._lib import ptr
    L = _lib.load()
    names, seqs = _fastq_spans()
    text = np.frombuffer(FASTQ, dtype=np.uint8)
    begin, end = seqs[:, 0].copy(), seqs[:, 1].copy()
    rn, roff = np.frombuffer(b"chrAchr_B", dtype=np.uint8), np.array([0, 4, 9], dtype=np.int64)
    hit_off = np.array([0, 1, 1], dtype=np.int64)

    def call(row, out, cap):
        hits = np.array([row], dtype=np.int32)
        rec_off = np.zeros(2, dtype=np.int64)
        return L.npr_seed_sam_text(2, ptr(text), ptr(names), ptr(begin), ptr(end), ptr(rn), ptr(roff), 2, ptr(hit_off), ptr(hits), ptr(rec_off),
                                   None if out is None else ptr(out), cap)
    need = call([0, 4, 0, 4], None, 0)
    assert need == len(RECORDS[0][-1])
    out = np.full(need + 1, 0x55, dtype=np.uint8)
    assert call([0, 4, 0, 4], out, need - 1) == _lib.ERR_CAPACITY and (out == 0x55).all()
    assert call([0, 4, 0, 4], out, need) == need and out[need] == 0x55 and bytes(out[:need]) == RECORDS[0][-1]
    for bad in ([2, 4, 0, 4], [-1, 4, 0, 4], [0, -1, 0, 4], [0, 4, 7, 4], [0, 4, 0, 0]):   # reference outside the list, a < 0, past the read, empty
        assert call(bad, None, 0) == _lib.ERR_INVALID, bad


def test_sam_text_parses_with_the_clip_lengths_of_the_match(tmp_path):
    from nanopore_amd import sam
    from nanopore_amd.analyses.utils import clipLengths, getAbsoluteReadOffset
    buf, _ = _sam_text()
    path = tmp_path / "hits.sam"
    path.write_bytes(b"@SQ\tSN:chrA\tLN:50\n@SQ\tSN:chr_B\tLN:200\n" + buf.tobytes())
    reads = ["ACGTACGTAC", "acgtTTGGcc"]
    recs = list(sam.Samfile(str(path), "r"))
    assert len(recs) == len(RECORDS)
    for rec, (i, r, a, b, rev, n, _) in zip(recs, RECORDS):
        assert (rec.rname, rec.pos, rec.is_reverse, rec.mapq) == (r, a, bool(rev), 255)
        assert clipLengths(rec) == (b, 10 - b - n)
        assert rec.cigar == [(op, length) for op, length in ((5, b), (0, n), (5, 10 - b - n)) if length]
        oriented = revcomp(reads[i]) if rev else reads[i]
        assert rec.seq == rec.query == oriented[b:b + n]
        assert getAbsoluteReadOffset(rec, "", reads[i]) == (b - 9 if rev else b)


def test_seed_mapper_classes_exist():
    from nanopore_amd.mappers import variants as V
    from nanopore_amd.mappers.abstractMapper import AbstractMapper
    from nanopore_amd.mappers.seedMapper import SeedMapper
    assert V.SeedMapper is SeedMapper and issubclass(SeedMapper, AbstractMapper)
    assert (SeedMapper.k, SeedMapper.minLength, SeedMapper.bothStrands) == (16, 20, True)
    for suffix in ("Chain", "Realign", "RealignEm", "RealignTrainedModel"):
        cls = getattr(V, "SeedMapper" + suffix)
        assert issubclass(cls, SeedMapper) and cls.__name__ == "SeedMapper" + suffix
    # the reference's base mappers still have nothing to run
    with pytest.raises(RuntimeError, match="external mapper"):
        V.Last("reads.fq", "2D", "ref.fa", os.path.join(os.sep, "nonexistent", "mapping.sam")).run()


def test_seed_mapper_has_no_cpu_fallback(tmp_path):
    try:
        import torch
        has_gpu = torch.cuda.is_available()
    except Exception:
        has_gpu = False
    if has_gpu:
        pytest.skip("a GPU is present: the failure path is exercised on the CPU box")
    from nanopore_amd import _lib
    from nanopore_amd.mappers.seedMapper import SeedMapper
    fa, fq, out = tmp_path / "ref.fa", tmp_path / "reads.fq", tmp_path / "mapping.sam"
    fa.write_text(">chr\nACGTACGTACGTACGTACGTACGTACGT\n")
    fq.write_text("@r\nACGTACGTACGTACGTACGTACGT\n+\n" + "I" * 24 + "\n")
    with pytest.raises(_lib.NprError) as e:
        SeedMapper(str(fq), "2D", str(fa), str(out)).run()
    assert e.value.code == _lib.ERR_NO_DEVICE
    assert not out.exists()

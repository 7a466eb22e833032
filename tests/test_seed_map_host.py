"""The host side of the device-resident seed map (include/nprealign.h: npr_seed_map_*): the binding knows the new symbols, job.SeedSource
turns chains into records with no SAM text in between, and SeedMapper leaves the fused path off by default.  No GPU."""
import os
import re
import types

import numpy as np
import pytest

from helpers import ROOT
from nanopore_amd import _lib, job, realign
from seed_mapper import revcomp

M, I, D = _lib.OP_M, _lib.OP_I, _lib.OP_D
MAP_SYMBOLS = ["npr_seed_map_create", "npr_seed_map_counts", "npr_seed_map_fetch", "npr_seed_map_destroy"]


def test_the_binding_and_the_library_have_the_map_symbols():
    """(tests/test_abi.py compares header, table and exports as wholes; this names the four that are new)"""
    L = _lib.load()
    header = open(os.path.join(ROOT, "include", "nprealign.h")).read()
    for name in MAP_SYMBOLS:
        assert name in _lib.SIGNATURES and hasattr(L, name) and re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.SIGNATURES["npr_seed_map_destroy"][0] is None and len(_lib.SIGNATURES["npr_seed_map_create"][1]) == 9
    assert int(re.search(r"#define NPR_SEED_MAP_LDS_ROWS (\d+)", header).group(1)) == _lib.SEED_MAP_LDS_ROWS
    assert _lib.SEED_MAP_LDS_ROWS * 16 <= 64 * 1024   # a row is four int32: the tier that sorts in LDS fits one workgroup's 64 KB


def test_fused_is_off_by_default():
    from nanopore_amd.mappers import variants as V
    from nanopore_amd.mappers.seedMapper import SeedMapper
    assert SeedMapper.fused is False
    assert V.SeedMapperChain.fused is False and V.SeedMapperRealign.fused is False and V.SeedMapperRealignEm.fused is False


# ---- SeedSource on hand-made chains: two references, both strands ----

REFS = [("contig_b", "ACGTTGCAAC"), ("contig_a", "GGGTTTCC")]           # (FASTA order is index order, whatever the names say)
READS = [("r07", "ACGTNacgTT"), ("r1", "TTGCA"), ("r10", "GGGNNtcc"), ("r02", "AAAA")]   # r1 sorts before r10: a shorter name before its extensions


def _tables(reads=READS):
    """What ingest.FastaTable / FastqTable hold, made by hand: only the attributes SeedSource and the formatters read."""
    fa = types.SimpleNamespace(names=[n for n, _ in REFS], seq=np.frombuffer("".join(s for _, s in REFS).encode(), dtype=np.uint8),
                               off=np.cumsum([0] + [len(s) for _, s in REFS]).astype(np.int64))
    text, name_span, seq_span = b"", [], []
    for name, seq in reads:
        text += b"@"
        name_span.append((len(text), len(text) + len(name)))
        text += name.encode() + b" words\n"
        seq_span.append((len(text), len(text) + len(seq)))
        text += seq.encode() + b"\n+\n" + b"I" * len(seq) + b"\n"
    fq = types.SimpleNamespace(text=np.frombuffer(text, dtype=np.uint8), name_span=np.array(name_span, dtype=np.int64).reshape(-1, 2),
                               seq_span=np.array(seq_span, dtype=np.int64).reshape(-1, 2))
    fq.lengths = fq.seq_span[:, 1] - fq.seq_span[:, 0]
    return fa, fq


def _chains():
    """Chains in the order npr_seed_chains gives them (read by read, ascending reference index); guides span reference x read.
    read 0 (r07, 10 bases): reference 0 reverse, reference 1 forward; read 1 (r1, 5): reference 0 forward; read 2 (r10, 8): reference 1
    reverse; read 3 (r02, 4): none."""
    chain_off = np.array([0, 2, 3, 4, 4], dtype=np.int64)
    chains = np.array([[0, 1, 7, 2], [1, 0, 5, 1], [0, 0, 5, 1], [1, 1, 6, 1]], dtype=np.int32)
    guides = [[(M, 4), (D, 1), (I, 1), (M, 3), (D, 2), (I, 2)], [(D, 3), (I, 5), (M, 5)], [(D, 4), (M, 5), (D, 1)], [(M, 3), (I, 2), (D, 2), (M, 3)]]
    ops_off = np.cumsum([0] + [len(g) for g in guides]).astype(np.int64)
    ops = np.array([p for g in guides for p in g], dtype=np.int32)
    return chain_off, chains, ops_off, ops, guides


@pytest.fixture(scope="module")
def source():
    fa, fq = _tables()
    chain_off, chains, ops_off, ops, guides = _chains()
    return job.SeedSource(fa, fq, chain_off, chains, ops_off, ops), guides


def test_seed_source_orders_records_by_reference_then_name(source):
    src, _ = source
    # reference 0: r07 (reverse), r1 (forward); reference 1: r07 (forward), r10 (reverse) -- "r07" < "r1" < "r10" as bytes
    assert src.n == 4 and src.ref_index.tolist() == [0, 0, 1, 1]
    assert [src.names[i] for i in src.read] == [b"r07", b"r1", b"r07", b"r10"] and src.strand.tolist() == [1, 0, 0, 1]
    assert src.lengths().tolist() == [10, 5, 10, 8]
    assert src.header == b"@SQ\tSN:contig_b\tLN:10\n@SQ\tSN:contig_a\tLN:8\n"


def test_seed_source_reads_are_the_fastq_spans_or_their_reverse_complements(source):
    src, _ = source
    fq_bytes = len(_tables()[1].text)
    got = [src.text[a:b].tobytes().decode() for a, b in zip(src.read_begin, src.read_end)]
    assert got == [revcomp("ACGTNacgTT"), "TTGCA", "ACGTNacgTT", revcomp("GGGNNtcc")]
    assert got[0] == "AAcgtNACGT" and got[3] == "ggaNNCCC"          # lower case stays lower case, N stays N
    # forward reads lie where the FASTQ has them, reverse complements behind it
    assert [int(a) < fq_bytes for a in src.read_begin] == [False, True, True, False]
    assert src.text[:fq_bytes].tobytes() == _tables()[1].text.tobytes() and len(src.text) == fq_bytes + 10 + 8


def test_seed_source_slices_every_guide(source):
    src, guides = source
    want = [guides[0], guides[2], guides[1], guides[3]]             # record k is chain (0, 2, 1, 3)[k]
    assert src.guide_off.tolist() == np.cumsum([0] + [len(g) for g in want]).tolist()
    for k, g in enumerate(want):
        assert [tuple(p) for p in src.guide_ops[src.guide_off[k]:src.guide_off[k + 1]].tolist()] == g


def _packed(src, lo, hi):
    """The guides of records lo .. hi as the packed words a finished batch hands to format_block"""
    off = src.guide_off[lo:hi + 1] - src.guide_off[lo]
    ops = src.guide_ops[src.guide_off[lo]:src.guide_off[hi]]
    return off, (ops[:, 1].astype(np.uint32) << 2) | ops[:, 0].astype(np.uint32)


def test_seed_source_formats_the_records_the_chain_formatter_writes(source):
    """With the guide's own cigar in place of a realigned one, format_block writes npr_seed_chain_sam_text's records byte for byte --
    as a whole and in blocks."""
    src, _ = source
    fa, fq = _tables()
    chain_off, chains, ops_off, ops, _ = _chains()
    want, rec_off = realign.seed_chain_sam_text(fq.text, fq.name_span, fq.seq_span[:, 0], fq.seq_span[:, 1], [n.encode() for n in fa.names], chain_off, chains, ops_off, ops)
    assert bytes(src.format_block(0, 4, *_packed(src, 0, 4))) == want.tobytes()
    for lo, hi in ((0, 1), (1, 3), (3, 4)):
        assert bytes(src.format_block(lo, hi, *_packed(src, lo, hi))) == want[rec_off[lo]:rec_off[hi]].tobytes()
    assert want.tobytes().split(b"\n")[0] == b"r07\t16\tcontig_b\t1\t255\t4M1D1I3M2D2I\t*\t0\t0\tAAcgtNACGT\t*"


def test_seed_source_refuses_two_reads_of_one_name():
    fa, fq = _tables([("r1", "ACGTACGT"), ("r2", "ACGT"), ("r1", "TTTT")])
    empty = (np.zeros(4, dtype=np.int64), np.zeros((0, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32))
    with pytest.raises(_lib.NprError) as e:
        job.SeedSource(fa, fq, *empty)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.NprError):                               # ... as the chain formatter does
        realign.seed_chain_sam_text(fq.text, fq.name_span, fq.seq_span[:, 0], fq.seq_span[:, 1], [n.encode() for n in fa.names], *empty)


def test_seed_source_without_chains_is_empty_and_well_formed():
    fa, fq = _tables()
    src = job.SeedSource(fa, fq, np.zeros(5, dtype=np.int64), np.zeros((0, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32))
    assert src.n == 0 and src.guide_off.tolist() == [0] and len(src.text) == len(fq.text)

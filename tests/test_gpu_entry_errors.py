"""The error paths of the analysis entry points behind the C ABI (csrc/npr_*_api.cpp), family by family: a refused call raises NprError with
the code and the last_error() text the header's case has always given (the texts below are written out here, not taken from the library),
leaves alone what the header says it leaves alone, and the valid call that follows on the same context returns what the analysis's host
reference computes.  Inputs: three reads of at most 200 bases against one 300-base reference; k = 3 for the k-mer tables, k = 8 for the
seed index.  No case forces a failure of the device."""
import numpy as np
import pytest

import read_quality_reference
from nanopore_amd import _lib
from nanopore_amd import realign as R
from nanopore_amd._lib import NprError, ptr
from nanopore_amd.analyses.marginAlignSnpCaller import FLAT_ERROR_MATRIX, NULL_MATRIX
from seed_chain_reference import as_chains, chains_by_rule
from seed_mapper import revcomp
from seed_reference import as_rows, rows_by_definition
from snp_calls_reference import snp_calls_reference
from snp_variants_reference import snp_variants_reference
from test_gpu_stats import _count_by_hand
from test_kmer_host import fold, indel_kmer_counters, table_of, window_counter
from test_pileup_host import WORDS, count_columns

pytestmark = pytest.mark.gpu

INVALID = _lib.ERR_INVALID
K, SEED_K, EDGE = 3, 8, 1e-9


def _inputs():
    """One reference of 300 bases; three reads cut from it with a substitution, an insertion and a deletion each (the third reversed for the
    seeding cases), their cigars and where they start."""
    rng = np.random.default_rng(5)
    ref = "".join("ACGT"[c] for c in rng.integers(0, 4, size=300))
    reads, cigars, starts = [], [], []
    for s, (m0, ins, m1, dele, m2) in zip((0, 60, 120), ((40, 2, 50, 3, 57), (70, 1, 30, 5, 60), (25, 3, 90, 1, 50))):
        body = list(ref[s:s + m0] + "".join("ACGT"[c] for c in rng.integers(0, 4, size=ins)) + ref[s + m0:s + m0 + m1] + ref[s + m0 + m1 + dele:s + m0 + m1 + dele + m2])
        body[7] = "ACGT"[("ACGT".index(body[7]) + 1) % 4]
        reads.append("".join(body))
        cigars.append([(0, m0), (1, ins), (0, m1), (2, dele), (0, m2)])
        starts.append((s, 0))
    assert len(ref) == 300 and all(len(r) <= 200 for r in reads)
    return ref, reads, cigars, starts


REF, READS, CIGARS, STARTS = _inputs()


def _refused(ctx, text, call, *args, **kw):
    """`call` raises NprError(NPR_ERR_INVALID) and the context's last error is `text`."""
    with pytest.raises(NprError) as e:
        call(*args, **kw)
    assert e.value.code == INVALID, e.value
    assert ctx.last_error() == text
    assert text in str(e.value)


def _pileup_table():
    table = np.zeros((300, WORDS), dtype=np.int32)
    for read, cigar, (sx, sy) in zip(READS, CIGARS, STARTS):
        count_columns(table, sx, [("MID"[op], n) for op, n in cigar], read, y=sy)
    return table


def test_align_stats(gpu_ctx):
    _refused(gpu_ctx, "npr_align_stats: without ref_index, n_refs must equal n_reads", gpu_ctx.align_stats, [REF], READS, CIGARS, start=STARTS)
    got = gpu_ctx.align_stats([REF], READS, CIGARS, ref_index=[0, 0, 0], start=STARTS)
    for i in range(3):
        assert np.array_equal(got[i].astype(np.int64), _count_by_hand(REF, READS[i], CIGARS[i], *STARTS[i])), i


def test_kmer_counts_and_groups(gpu_ctx):
    L, seq = gpu_ctx._L, np.frombuffer("".join(READS).encode(), dtype=np.uint8)
    out = np.full(4 ** K + 1, -7, dtype=np.int64)
    off = np.array([0, 100, 50, 120], dtype=np.int64)   # a decreasing offset
    assert L.npr_kmer_counts(gpu_ctx._h, K, 3, ptr(seq), ptr(off), ptr(out)) == INVALID
    assert gpu_ctx.last_error() == "npr_kmer_counts: sequence offsets decrease"
    assert gpu_ctx.kmer_counts(READS, K).tolist() == table_of(window_counter(READS, K), K).tolist()

    lens = [len(r) for r in READS]
    begin = np.array([0, lens[0], lens[0] + lens[1]], dtype=np.int64)
    end = begin + np.array(lens, dtype=np.int64)
    tables = np.full((2, 4 ** K + 1), -7, dtype=np.int64)
    group = np.array([0, 2, 1], dtype=np.int32)         # a group outside its range
    assert L.npr_kmer_counts_groups(gpu_ctx._h, K, 3, ptr(seq), ptr(begin), ptr(end), ptr(group), 2, ptr(tables)) == INVALID
    assert gpu_ctx.last_error() == "npr_kmer_counts_groups: a group outside -1 .. n_groups - 1"
    assert (tables == -7).all()                          # no table touched when an argument is wrong
    _refused(gpu_ctx, "npr_kmer_counts_groups: a group outside -1 .. n_groups - 1", gpu_ctx.kmer_counts_groups, seq, begin, end, [0, 2, 1], 2, K)
    got = gpu_ctx.kmer_counts_groups(seq, begin, end, [0, 1, 0], 2, K)
    assert got[0].tolist() == table_of(window_counter([READS[0], READS[2]], K), K).tolist()
    assert got[1].tolist() == table_of(window_counter([READS[1]], K), K).tolist()


def test_indel_kmers(gpu_ctx):
    _refused(gpu_ctx, "npr_align_indel_kmers: without ref_index, n_refs must equal n_reads", gpu_ctx.align_indel_kmers, [REF], READS, CIGARS, k=K, start=STARTS)
    with pytest.raises(NprError) as e:                  # k outside its range: refused without a text of its own
        gpu_ctx.align_indel_kmers([REF] * 3, READS, CIGARS, k=7, start=STARTS)
    assert e.value.code == INVALID
    rd, rf = gpu_ctx.align_indel_kmers([REF], READS, CIGARS, k=K, ref_index=[0, 0, 0], start=STARTS)
    want_rd, want_rf = indel_kmer_counters([(fold(REF[sx:]), fold(read[sy:]), cigar) for read, cigar, (sx, sy) in zip(READS, CIGARS, STARTS)], K)
    assert rd.sum() > 0 and rf.sum() > 0
    assert rd.tolist() == table_of(want_rd, K).tolist() and rf.tolist() == table_of(want_rf, K).tolist()


def test_read_quality(gpu_ctx):
    rng = np.random.default_rng(9)
    reads = [(r.encode(), bytes(int(q) for q in rng.integers(35, 75, size=len(r)))) for r in READS]
    text, seq, qual = read_quality_reference.fastq_text(reads)
    text, seq, qual = np.asarray(text, dtype=np.uint8), np.asarray(seq, dtype=np.int64).reshape(-1, 2), np.asarray(qual, dtype=np.int64).reshape(-1, 2)
    out = R.ReadQuality.zeros(2)
    for a in out.arrays():
        a[...] = -7
    cols = [np.ascontiguousarray(a) for a in (seq[:, 0], seq[:, 1], qual[:, 0], qual[:, 1])]
    group = np.array([0, 2, 1], dtype=np.int32)
    assert gpu_ctx._L.npr_read_quality(gpu_ctx._h, 3, ptr(text), *map(ptr, cols), ptr(group), 2, *map(ptr, out.arrays())) == INVALID
    assert gpu_ctx.last_error() == "npr_read_quality: a group outside -1 .. n_groups - 1"
    assert all((a == -7).all() for a in out.arrays())   # no table touched when an argument is wrong
    _refused(gpu_ctx, "npr_read_quality: a group outside -1 .. n_groups - 1", gpu_ctx.read_quality, text, seq, qual, [0, 2, 1], 2)
    got = gpu_ctx.read_quality(text, seq, qual, [0, 1, 0], 2)
    for g, w in zip(got.arrays(), read_quality_reference.tables(text, seq, qual, [0, 1, 0], 2)):
        assert g.shape == w.shape and np.array_equal(g, w)


def test_pileup_create_and_add(gpu_ctx):
    _refused(gpu_ctx, "npr_pileup_create: a reference length is negative or 2^31 and more", gpu_ctx.pileup, [300, -1])
    pl = gpu_ctx.pileup([300])
    try:
        read = np.frombuffer("".join(READS).encode(), dtype=np.uint8)
        read_off = np.concatenate([[0], np.cumsum([len(r) for r in READS])]).astype(np.int64)
        ops = np.array([op for c in CIGARS for op in c], dtype=np.int32)
        _refused(gpu_ctx, "npr_pileup_add: operation offsets decrease", pl.add_csr, read, read_off, None, ops, [0, 10, 5, 15], [0, 0, 0], STARTS)
        assert not pl.counts().any()                    # the refused call added nothing
        pl.add(READS, CIGARS, [0, 0, 0], start=STARTS)
        want = _pileup_table()
        assert np.array_equal(pl.counts(), want)
        depth, covered = pl.depth()
        assert np.array_equal(depth, want[:, :5].sum(axis=1)) and np.array_equal(covered, (want[:, :6].sum(axis=1) > 0))
    finally:
        pl.close()


def _snp_table():
    """Base weights of the 300 positions: the three reads' aligned-base counts plus a seeded fraction, which keeps every posterior away
    from the edges the references guard; two positions nobody has seen."""
    counts = _pileup_table()
    rng = np.random.default_rng(21)
    weights = counts[:, :4].astype(np.float64) + 0.5 * rng.random((300, 4))
    seen = counts[:, :5].sum(axis=1) > 0
    weights[~seen] = 0.0
    ref_code = np.array(["ACGT".index(c) for c in REF], dtype=np.uint8)
    true_code = ref_code.copy()
    true_code[::37] = (true_code[::37] + 1) % 4
    return weights, seen, ref_code, true_code


def test_snp_calls_table(gpu_ctx):
    weights, seen, ref_code, true_code = _snp_table()
    bad = weights.copy()
    bad[150, 2] = -1.0
    _refused(gpu_ctx, "npr_snp_calls_table: a weight is negative or not finite", gpu_ctx.snp_calls_table, bad, seen, ref_code, true_code, NULL_MATRIX, (FLAT_ERROR_MATRIX,))
    want, edge = snp_calls_reference(weights, seen, ref_code, true_code, (FLAT_ERROR_MATRIX,))
    assert edge > EDGE and want[0][3] > 200 and 0 < want[0][2] < 100
    got = gpu_ctx.snp_calls_table(weights, seen, ref_code, true_code, NULL_MATRIX, (FLAT_ERROR_MATRIX,))
    assert len(got) == 1
    assert np.array_equal(got[0][0], want[0][0]) and np.array_equal(got[0][1], want[0][1]) and got[0][2:] == want[0][2:]


def test_snp_variants_table(gpu_ctx):
    weights, seen, ref_code, _ = _snp_table()
    bad = weights.copy()
    bad[150, 2] = -1.0
    _refused(gpu_ctx, "npr_snp_variants_table: a weight is negative or not finite", gpu_ctx.snp_variants_table, bad, seen, ref_code, NULL_MATRIX, FLAT_ERROR_MATRIX, 0.3)
    want = snp_variants_reference(weights, seen, ref_code, FLAT_ERROR_MATRIX, 0.3)
    assert want["threshold_gap"] > EDGE and want["qual_gap"] > EDGE and want["lp_gap"] > EDGE and len(want["call_row"]) > 0
    best, qual, call_row, call_alt, call_p = gpu_ctx.snp_variants_table(weights, seen, ref_code, NULL_MATRIX, FLAT_ERROR_MATRIX, 0.3)
    assert np.array_equal(best, want["best"]) and np.array_equal(qual, want["qual"])
    assert np.array_equal(call_row, want["call_row"]) and np.array_equal(call_alt, want["call_alt"])
    assert np.abs(call_p - want["call_p"]).max() <= 1e-12   # (the bound of tests/test_gpu_snp_variants.py, argued there)


def _seed_reads():
    reads = [READS[0], READS[1], revcomp(READS[2])]
    text = np.frombuffer("".join(reads).encode(), dtype=np.uint8)
    begin = np.concatenate([[0], np.cumsum([len(r) for r in reads])[:-1]]).astype(np.int64)
    return reads, text, begin, begin + np.array([len(r) for r in reads], dtype=np.int64)


def test_seed_index_and_matches(gpu_ctx):
    reads, text, begin, end = _seed_reads()
    _refused(gpu_ctx, "npr_seed_index_create: k outside 8 .. 32", gpu_ctx.seed_index, [REF], k=7)
    ix = gpu_ctx.seed_index([REF], k=SEED_K)
    try:
        _refused(gpu_ctx, "npr_seed_matches: strands outside 1 .. 3", ix.matches, text, begin, end, min_len=12, strands=0)
        hit_off, hits = ix.matches(text, begin, end, min_len=12, strands=3)
        assert hit_off[-1] == len(hits) > 0
        for i, r in enumerate(reads):
            assert as_rows(hits[hit_off[i]:hit_off[i + 1]]) == rows_by_definition([REF], r, 12), i
    finally:
        ix.close()


def test_seed_map_and_chains(gpu_ctx):
    reads, text, begin, end = _seed_reads()
    read_len, ref_len = [len(r) for r in reads], [300]
    ix = gpu_ctx.seed_index([REF], k=SEED_K)
    try:
        _refused(gpu_ctx, "npr_seed_map_create: strands outside 1 .. 3", ix.map, text, begin, end, min_len=12, strands=0)
        hit_off, hits, chain_off, chains, ops_off, ops = ix.map(text, begin, end, min_len=12, strands=3, max_gap=50, rows=True)
    finally:
        ix.close()
    want_rows = [rows_by_definition([REF], r, 12) for r in reads]
    assert [as_rows(hits[hit_off[i]:hit_off[i + 1]]) for i in range(3)] == want_rows
    want = chains_by_rule(read_len, ref_len, hit_off, hits, 50)
    assert sum(len(w) for w in want) >= 3
    assert as_chains(chain_off, chains, ops_off, ops) == want

    _refused(gpu_ctx, "npr_seed_chains: a negative max_gap", gpu_ctx.seed_chains, read_len, ref_len, hit_off, hits, -1)
    down = hit_off.copy()
    down[1], down[2] = hit_off[2], hit_off[1]           # a decreasing offset
    assert down[2] < down[1]
    _refused(gpu_ctx, "npr_seed_chains: row offsets decrease, or a read length outside 0 .. 2^31 - 1", gpu_ctx.seed_chains, read_len, ref_len, down, hits, 50)
    assert as_chains(*gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, 50)) == want


def test_cigar_text_packed(gpu_ctx):
    words = np.array([n << 2 | op for c in CIGARS for op, n in c], dtype=np.uint32)
    n_ops = np.array([len(c) for c in CIGARS], dtype=np.int64)
    word_off = np.concatenate([[0], np.cumsum(n_ops)[:-1]]).astype(np.int64)
    bad = n_ops.copy()
    bad[1] = -1
    str_off = np.full(4, -7, dtype=np.int64)
    out = np.full(64, 0x21, dtype=np.uint8)
    assert gpu_ctx._L.npr_cigar_text_packed(gpu_ctx._h, 3, ptr(word_off), ptr(bad), ptr(words), ptr(str_off), ptr(out), 64) == INVALID
    assert gpu_ctx.last_error() == "npr_cigar_text_packed: a negative count or offset"
    assert (str_off == -7).all() and (out == 0x21).all()
    _refused(gpu_ctx, "npr_cigar_text_packed: a negative count or offset", R.cigar_text_packed, gpu_ctx, word_off, bad, words)
    got, got_off = R.cigar_text_packed(gpu_ctx, word_off, n_ops, words)
    want, want_off = R.format_cigars_packed(word_off, n_ops, words)
    assert bytes(got) == bytes(want) == b"40M2I50M3D57M70M1I30M5D60M25M3I90M1D50M" and got_off.tolist() == want_off.tolist()

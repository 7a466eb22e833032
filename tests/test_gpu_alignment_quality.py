"""The alignment-quality tables on the device (include/nprealign.h: npr_pileup_coverage, npr_align_quality; csrc/npr_alnqual.hip;
nanopore_amd/analyses/qualimap.py): every table against the restatement of the header's text (tests/alignment_quality_reference.py), count for
count.  The pileup tables the coverage pass is compared on come from the column counter of tests/test_pileup_host.py, not from the device."""
import os

import numpy as np
import pytest

import alignment_quality_reference as ref
from alignment_quality_reference import OP_D as D, OP_I as I, OP_M as M, record
from nanopore_amd import _lib
from nanopore_amd.realign import AlignQuality, Coverage, NprError
from test_pileup_host import SETS, count_columns, fixture

pytestmark = pytest.mark.gpu

TILE = _lib.AQ_TILE
MARK = -7777


def _seq(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _records(rng, refs, per_kb=12, max_ops=9):
    """random records that fit their sequences: M runs of 1 .. 40 with I and D runs of 1 .. 6 between them"""
    out = []
    for k, seq in enumerate(refs):
        for _ in range(max(1, len(seq) * per_kb // 1000)):
            x = int(rng.integers(0, len(seq)))
            room, cigar, read = len(seq) - x, [], b""
            for j in range(int(rng.integers(1, max_ops + 1))):
                if j and rng.integers(0, 2):
                    n = int(rng.integers(1, 7))
                    if rng.integers(0, 2):
                        cigar.append((I, n))
                        read += _seq(rng, n, "ACGTN")
                    elif room > n:
                        cigar.append((D, n))
                        room -= n
                n = min(int(rng.integers(1, 41)), room)
                if n == 0:
                    break
                cigar.append((M, n))
                read += _seq(rng, n, "ACGTacgtN")
                room -= n
            out.append(record(k, read, cigar, mapq=int(rng.integers(0, 256)), clip=(int(rng.integers(0, 3)) * 5, int(rng.integers(0, 2)) * 7), start=(x, 0)))
    return out


def _counted_table(refs, records):
    """the pileup table of the records from the column counter"""
    first = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int64)
    table = np.zeros((int(first[-1]), 8), dtype=np.int64)
    for rec in records:
        if rec["use"]:
            count_columns(table, int(first[rec["ref_index"]]) + rec["start"][0], [("MID"[op], n) for op, n in rec["cigar"]], rec["read"].decode(), y=rec["start"][1])
    return table


def _device_pileup(ctx, refs, records):
    a = ref.arrays_of(records, refs)
    pileup = ctx.pileup([len(r) for r in refs])
    if records:
        pileup.add_csr(a["read"], a["read_begin"], a["read_end"], a["ops"], a["ops_off"], a["ref_index"], start=a["start"], use=a["use"])
    return pileup, a


def _same(got, want, what):
    for name, g, w in zip(got.FIELDS, got.arrays(), want):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:8].tolist(), g[g != w][:8].tolist(), w[g != w][:8].tolist())


def _check_coverage(ctx, refs, records, windows):
    pileup, a = _device_pileup(ctx, refs, records)
    try:
        table = _counted_table(refs, records)
        assert np.array_equal(pileup.counts(), table)   # (the device's table is the counter's: what the coverage pass runs over)
        for W in windows:
            _same(pileup.coverage(a["ref_text"], a["ref_off"], W), ref.coverage(table, b"".join(refs), W), "W = %d" % W)
    finally:
        pileup.close()


def _quality(ctx, refs, records, W, **kw):
    a = ref.arrays_of(records, refs)
    return ctx.align_quality(a["read"], a["read_begin"], a["read_end"], a["ops"], a["ops_off"], a["ref_index"], a["mapq"], a["clip"], a["ref_text"], a["ref_off"],
                             start=a["start"], use=a["use"], n_windows=W, **kw)


def _check_quality(ctx, refs, records, windows, invalid=False):
    for W in windows:
        want, want_invalid = ref.quality(records, refs, W)
        assert want_invalid == invalid
        got = _quality(ctx, refs, records, W, allow_invalid=True)
        assert got.invalid == invalid
        _same(got, want, "W = %d" % W)
        if invalid:
            with pytest.raises(NprError) as e:
                _quality(ctx, refs, records, W)
            assert e.value.code == _lib.ERR_INVALID


SHAPES = [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3]


@pytest.mark.parametrize("T", SHAPES)
def test_coverage_shapes_each_alone(gpu_ctx, T):
    rng = np.random.default_rng(T)
    refs = [_seq(rng, T, "ACGTacgtN")]
    records = _records(rng, refs)
    _check_coverage(gpu_ctx, refs, records, [1, 2, 7, 400, T, T + 3])
    _check_quality(gpu_ctx, refs, records, [1, 2, 7, 400, T, T + 3])


def test_coverage_shapes_in_one_call(gpu_ctx):
    """the eight shapes as the sequences of one pileup: the boundaries fall inside windows and inside tiles"""
    rng = np.random.default_rng(11)
    refs = [_seq(rng, T, "ACGTacgtN") for T in SHAPES]
    records = _records(rng, refs, per_kb=6)
    T = sum(SHAPES)
    _check_coverage(gpu_ctx, refs, records, [1, 2, 7, 400, T, T + 3])
    _check_quality(gpu_ctx, refs, records, [7, 400, T + 3])


@pytest.mark.parametrize("lengths", [(TILE - 37, 90), (700, TILE - 650, 301)])
def test_sequence_boundaries_inside_a_window_and_a_tile(gpu_ctx, lengths):
    rng = np.random.default_rng(len(lengths))
    refs = [_seq(rng, n) for n in lengths]
    records = _records(rng, refs)
    # ... with records that end on the last row of their sequence and begin on its first
    records += [record(k, _seq(rng, 30), [(M, 30)], mapq=9, start=(len(s) - 30, 0)) for k, s in enumerate(refs)]
    records += [record(k, _seq(rng, 12), [(M, 12)], mapq=200, start=(0, 0)) for k, s in enumerate(refs)]
    _check_coverage(gpu_ctx, refs, records, [1, 2, 3, 7, 400])
    _check_quality(gpu_ctx, refs, records, [1, 2, 3, 7, 400])


def test_stacked_records_reach_the_bin_edges(gpu_ctx):
    """33 identical 40-base records on one start (the worst case for the atomics), and stacks of 15, 16, 17, 31 and 32 beside it: the depth
    and start bins on either side of 16 and of 32"""
    rng = np.random.default_rng(5)
    refs = [_seq(rng, 400)]
    read = _seq(rng, 40)
    records = []
    for j, k in enumerate((33, 15, 16, 17, 31, 32)):
        records += [record(0, read, [(M, 40)], mapq=60, start=(10 + 60 * j, 0)) for _ in range(k)]
    table = _counted_table(refs, records)
    assert sorted(set(table[:, :5].sum(axis=1).tolist())) == [0, 15, 16, 17, 31, 32, 33] and sorted(set(table[:, 7].tolist())) == [0, 15, 16, 17, 31, 32, 33]
    _check_coverage(gpu_ctx, refs, records, [1, 7, 400])
    _check_quality(gpu_ctx, refs, records, [1, 7, 400])


def test_deletions_across_window_and_tile_boundaries(gpu_ctx):
    rng = np.random.default_rng(6)
    T = TILE + 100
    refs = [_seq(rng, T)]
    records = [record(0, _seq(rng, 10), [(M, 5), (D, 20), (M, 5)], mapq=30, start=(TILE - 10, 0)),     # the D run lies across the tile boundary
               record(0, _seq(rng, 8), [(M, 4), (D, T // 2), (M, 4)], mapq=31, start=(T // 4, 0)),     # ... and across the boundary of two windows
               record(0, _seq(rng, 2), [(D, 7), (M, 2)], mapq=32, start=(40, 0))]                      # positions 40 .. 46 lie under a deletion only
    table = _counted_table(refs, records)
    assert table[40:47, :5].sum() == 0 and (table[40:47, 5] == 1).all()
    _check_coverage(gpu_ctx, refs, records, [1, 2, 7, 400, T])
    _check_quality(gpu_ctx, refs, records, [1, 2, 7, 400, T])


# reference sequences for the record shapes and the homopolymer rules: the first two end in AA, the second begins with AAA, the third with AC
REF0 = b"CGTACGAAGTCATTTGCAGCnnATGCAcgtaGGCTAGCTAGGATCCATCGATCGGTACCAGTGAA"
REF1 = b"AAAGCTTGCATGCCTGCAGGTCGACTCTAGAGGATCCCCGGGTACCGAGCTCGAATTCGTAATCATGGTCATAGCTGTTTCCTGTGTGAAATTGTTATCCGCTC" * 3 + b"AA"
REF2 = b"ACGGTCAAGCTT"
REFS = [REF0, REF1, REF2]


def _m(k, x, n, **kw):
    """n columns of M at position x of sequence k, the read equal to the reference"""
    return record(k, REFS[k][x:x + n], [(M, n)], start=(x, 0), **kw)


SHAPE_CASES = {
    "m_runs_of_length_one": [record(1, "ACGTA", [(M, 1), (I, 1), (M, 1), (D, 1), (M, 1), (D, 2), (M, 1)], mapq=3, start=(7, 0))],
    "m_run_over_three_windows": [_m(1, 20, 200, mapq=17)],
    "ends_on_the_last_row": [_m(0, len(REF0) - 9, 9, mapq=1), _m(2, 0, len(REF2), mapq=2)],
    "lower_case_and_n": [record(0, "acgtNnACGTxx", [(M, 12)], mapq=4, start=(16, 0))],
    "two_i_runs_in_a_row": [record(1, "ACGGTTTAC", [(M, 2), (I, 2), (I, 3), (M, 2)], mapq=5, start=(3, 0))],
    "d_then_i": [record(1, "ACGTT", [(M, 2), (D, 4), (I, 1), (M, 2)], mapq=6, start=(30, 0))],
    "leading_and_trailing_i": [record(1, "GGACGTCC", [(I, 2), (M, 4), (I, 2)], mapq=7, start=(50, 0))],
    "mapq_0_and_255": [_m(1, 5, 20, mapq=0), _m(1, 6, 20, mapq=255)],
    "clips": [_m(1, 10, 30, mapq=8, clip=(0, 0)), _m(1, 11, 30, mapq=8, clip=(5, 0)), _m(1, 12, 30, mapq=8, clip=(0, 7)), _m(1, 13, 30, mapq=8, clip=(3000, 2500))],
    "empty_aligned_span": [record(1, "", [], mapq=9, start=(4, 0)), record(1, "", [(D, 3)], mapq=10, clip=(2, 0), start=(4, 0)), record(0, "NNNN", [(I, 4)], mapq=11)],
    "starts_inside_its_read": [record(1, "TTTACGTACGT", [(M, 4), (I, 2), (M, 2)], mapq=12, clip=(6, 1), start=(40, 3))],
    "not_selected": [_m(1, 0, 10, mapq=13), record(1, "ACGT", [(M, 40)], mapq=999, clip=(-1, 0), start=(0, 0), use=False), _m(1, 3, 10, mapq=14)],
    "zero_length_runs": [record(1, "ACGTAC", [(M, 3), (I, 0), (D, 0), (M, 0), (M, 3)], mapq=15, start=(9, 0))],
}
HOMOPOLYMER_CASES = {
    # REF0: AA at 6-7, TTT at 12-14, AA at the end; an I run at x has the bases x - 1, x - 2, .. to its left and x, x + 1, .. to its right
    "i_after_aa": [record(0, b"GA" + b"A" + b"GT", [(M, 2), (I, 1), (M, 2)], start=(6, 0))],            # x = 8: l = 2, r = 0
    "i_after_ttt": [record(0, b"TT" + b"T" + b"GC", [(M, 2), (I, 1), (M, 2)], start=(13, 0))],          # x = 15: l = 3
    "i_before_aa": [record(0, b"CG" + b"AA" + b"AA", [(M, 2), (I, 2), (M, 2)], start=(4, 0))],          # x = 6: r = 2
    "i_before_ttt": [record(0, b"CA" + b"T" + b"TT", [(M, 2), (I, 1), (M, 2)], start=(10, 0))],         # x = 12: r = 3
    "i_inside_aa": [record(0, b"GA" + b"A" + b"AG", [(M, 2), (I, 1), (M, 2)], start=(5, 0))],           # x = 7: l = 1, r = 1
    "i_inside_ttt": [record(0, b"AT" + b"t" + b"TT", [(M, 2), (I, 1), (M, 2)], start=(11, 0))],         # x = 13: l = 1, r = 2, lower case
    "d_of_a_whole_run_of_three": [record(0, b"CAGC", [(M, 2), (D, 3), (M, 2)], start=(10, 0))],
    "d_of_part_of_a_run_of_two": [record(0, b"CGAG", [(M, 2), (D, 1), (M, 2)], start=(4, 0)), record(0, b"CGAG", [(M, 3), (D, 1), (M, 1)], start=(4, 0))],
    "d_of_mixed_bases": [record(0, b"CGGC", [(M, 2), (D, 9), (M, 2)], start=(4, 0))],
    "mixed_base_insertion": [record(0, b"TT" + b"TA" + b"TG", [(M, 2), (I, 2), (M, 2)], start=(12, 0))],
    "insertion_of_n": [record(0, b"TT" + b"N" + b"TG", [(M, 2), (I, 1), (M, 2)], start=(12, 0))],
    "i_before_the_first_column_of_the_second_sequence": [record(1, b"A" + b"AAAG", [(I, 1), (M, 4)], start=(0, 0))],   # l must be 0 (r = 3)
    "i_before_the_first_column_of_the_third_sequence": [record(2, b"A" + b"ACGG", [(I, 1), (M, 4)], start=(0, 0))],    # l = 0, r = 1: not a homopolymer
    "d_ending_on_the_last_base_of_a_sequence": [record(0, b"GT", [(M, 2), (D, 2)], start=(len(REF0) - 4, 0))],         # l = 0, 2 deleted, r = 0 although AAA follows
    "i_at_the_end_of_a_sequence": [record(0, b"AA" + b"A", [(M, 2), (I, 1)], start=(len(REF0) - 2, 0))],                # l = 2, r = 0
}
WINDOWS = [1, 7, 50, 400]


@pytest.mark.parametrize("case", sorted(SHAPE_CASES))
def test_record_shapes(gpu_ctx, case):
    _check_quality(gpu_ctx, REFS, SHAPE_CASES[case], WINDOWS)


@pytest.mark.parametrize("case", sorted(HOMOPOLYMER_CASES))
def test_homopolymer_rules(gpu_ctx, case):
    _check_quality(gpu_ctx, REFS, HOMOPOLYMER_CASES[case], [1, 7])


def test_all_cases_in_one_call(gpu_ctx):
    records = [r for case in sorted(SHAPE_CASES) for r in SHAPE_CASES[case]] + [r for case in sorted(HOMOPOLYMER_CASES) for r in HOMOPOLYMER_CASES[case]]
    _check_quality(gpu_ctx, REFS, records, WINDOWS + [len(REF0) + len(REF1) + len(REF2) + 3])
    _check_coverage(gpu_ctx, REFS, records, WINDOWS)


def test_long_cigars_and_many_records(gpu_ctx):
    """cigars of more than 64 operations, more records than one workgroup takes, reads long enough to leave the narrow bins"""
    rng = np.random.default_rng(21)
    refs = [_seq(rng, 3000, "ACGTN"), _seq(rng, 2 * TILE + 500, "AACCGGTTn")]
    records = _records(rng, refs, per_kb=20, max_ops=90)
    assert max(len(r["cigar"]) for r in records) > 128 and len(records) > 100
    _check_quality(gpu_ctx, refs, records, [7, 400])
    _check_coverage(gpu_ctx, refs, records, [7, 400])


INVALID = {
    "operation_outside_m_i_d": record(1, "ACGTACGT", [(M, 4), (3, 2), (M, 2)], mapq=20, start=(5, 0)),
    "cigar_past_its_read": record(1, "ACGT", [(M, 3), (I, 2)], mapq=20, start=(5, 0)),
    "cigar_past_its_sequence": record(2, "ACGGTCAAGCTTA", [(M, 4), (D, 6), (M, 3)], mapq=20, start=(0, 0)),
    "mapq_256": record(1, "ACGT", [(M, 4)], mapq=256, start=(5, 0)),
    "negative_clip": record(1, "ACGT", [(M, 4)], mapq=20, clip=(0, -1), start=(5, 0)),
}


@pytest.mark.parametrize("case", sorted(INVALID))
def test_an_invalid_record_adds_nothing(gpu_ctx, case):
    valid = SHAPE_CASES["clips"] + SHAPE_CASES["d_then_i"]
    records = valid[:3] + [INVALID[case]] + valid[3:]
    assert not ref.record_is_valid(INVALID[case], REFS)
    _check_quality(gpu_ctx, REFS, records, [7], invalid=True)
    want_without, _ = ref.quality(valid, REFS, 7)
    _same(_quality(gpu_ctx, REFS, records, 7, allow_invalid=True), want_without, case)


def _marked(tables):
    for a in tables.arrays():
        a[...] = MARK
    return tables


def _untouched(tables):
    return all((a == MARK).all() for a in tables.arrays())


def test_what_the_host_refuses_writes_nothing(gpu_ctx):
    records = SHAPE_CASES["clips"]
    pileup, a = _device_pileup(gpu_ctx, REFS, records)
    try:
        for W in (0, -1, _lib.AQ_MAX_WINDOWS + 1):
            out = _marked(Coverage.zeros(4))
            with pytest.raises(NprError) as e:
                pileup.coverage(a["ref_text"], a["ref_off"], W, out=out)
            assert e.value.code == _lib.ERR_INVALID and _untouched(out)
            out = _marked(AlignQuality.zeros(4))
            with pytest.raises(NprError) as e:
                _quality(gpu_ctx, REFS, records, W, out=out)
            assert e.value.code == _lib.ERR_INVALID and _untouched(out)
        # a sequence that is not as long as the pileup's
        out, off = _marked(Coverage.zeros(4)), a["ref_off"].copy()
        off[1] -= 1
        with pytest.raises(NprError) as e:
            pileup.coverage(a["ref_text"], off, 4, out=out)
        assert e.value.code == _lib.ERR_INVALID and _untouched(out)
        # a null pointer where the call needs one
        L, arrays = _lib.load(), out.arrays()
        assert L.npr_pileup_coverage(pileup._h, _lib.ptr(a["ref_text"]), None, 4, *map(_lib.ptr, arrays)) == _lib.ERR_INVALID
        assert L.npr_pileup_coverage(pileup._h, _lib.ptr(a["ref_text"]), _lib.ptr(a["ref_off"]), 4, None, *map(_lib.ptr, arrays[1:])) == _lib.ERR_INVALID
        assert _untouched(out)
    finally:
        pileup.close()
    # reference offsets that decrease, operation offsets that decrease
    for key, at in (("ref_off", 1), ("ops_off", 2)):
        b = dict(a)
        b[key] = a[key].copy()
        b[key][at] = b[key][at + 1] + 1
        out = _marked(AlignQuality.zeros(4))
        with pytest.raises(NprError) as e:
            gpu_ctx.align_quality(b["read"], b["read_begin"], b["read_end"], b["ops"], b["ops_off"], b["ref_index"], b["mapq"], b["clip"], b["ref_text"], b["ref_off"],
                                  start=b["start"], use=b["use"], n_windows=4, out=out)
        assert e.value.code == _lib.ERR_INVALID and _untouched(out)


def test_the_same_call_twice_gives_equal_arrays(gpu_ctx):
    rng = np.random.default_rng(31)
    refs = [_seq(rng, TILE + 77), _seq(rng, 500)]
    records = _records(rng, refs, per_kb=30)
    pileup, a = _device_pileup(gpu_ctx, refs, records)
    try:
        one, two = pileup.coverage(a["ref_text"], a["ref_off"], 400), pileup.coverage(a["ref_text"], a["ref_off"], 400)
        assert all(np.array_equal(x, y) for x, y in zip(one.arrays(), two.arrays())) and one.totals[1] > 0
    finally:
        pileup.close()
    one, two = _quality(gpu_ctx, refs, records, 400), _quality(gpu_ctx, refs, records, 400)
    assert all(np.array_equal(x, y) for x, y in zip(one.arrays(), two.arrays())) and one.totals[0] == len(records)


def test_nothing_to_count(gpu_ctx):
    """n_reads == 0, a pileup with nothing added, and a reference without a base"""
    for refs in (REFS, [b""], []):
        _check_quality(gpu_ctx, refs, [], [1, 5])
        _check_coverage(gpu_ctx, refs, [], [1, 5])
    got = _quality(gpu_ctx, REFS, [], 5, out=_marked(AlignQuality.zeros(5)))
    assert all((x == 0).all() for x in got.arrays())


@pytest.mark.parametrize("name", SETS)
def test_qualimap_end_to_end(gpu_ctx, tmp_path, name):
    """QualiMap(...).run(ctx) writes every file; each is the text the report writer makes of the restatement's tables for the same records, and
    coverage_across_reference.txt sums to what `samtools depth` printed"""
    from nanopore_amd.analyses import qualimap
    from test_alignment_quality_host import _Tables, _depth_file, _parse
    fx = fixture(name)
    out_dir = str(tmp_path / "out")
    os.makedirs(out_dir)
    analysis = qualimap.QualiMap(None, "2D", fx["fa_path"], fx["sam_path"], out_dir)
    analysis.run(gpu_ctx)
    assert qualimap.QualiMap.isFinished(out_dir)
    names, records = ref.records_of_sam(fx["sam"])
    seqs = ref.fasta_sequences(open(fx["fa_path"]).read())
    refs = [seqs[n] for n in names]
    W = qualimap.QualiMap.n_windows
    cov = _Tables(**dict(zip(Coverage.FIELDS, ref.coverage(_counted_table(refs, records), b"".join(refs), W))))
    qual = _Tables(**dict(zip(AlignQuality.FIELDS, ref.quality(records, refs, W)[0])))
    want = qualimap.reportTexts(cov, qual, os.path.basename(fx["sam_path"]), os.path.basename(fx["fa_path"]), len(names))
    assert len(want) == 11
    for rel, text in want.items():
        assert open(os.path.join(out_dir, rel)).read() == text, rel
    _, rows, _ = _parse(open(os.path.join(out_dir, qualimap.RAW_DIR, "coverage_across_reference.txt")).read())
    assert len(rows) == W and sum(int(r[2]) for r in rows) == _depth_file(fx["depth"])[0] > 0

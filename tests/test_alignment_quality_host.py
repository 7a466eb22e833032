"""The alignment-quality tables without a device: the restatement of the header's definitions (tests/alignment_quality_reference.py) against
what samtools printed for the fixtures of tests/golden/pileup/, the two window formulas, the NPR_ERR_CAPACITY arithmetic, the report writer of
nanopore_amd/analyses/qualimap.py on hand-made tables, and how the pipeline finds the class."""
import math
import os

import numpy as np
import pytest

import alignment_quality_reference as ref
from test_pileup_host import SETS, counter_of_sam, fixture


def _depth_file(text):
    """(sum of the depth column, lines with depth >= 1)"""
    depths = [int(line.split("\t")[2]) for line in text.split("\n") if line]
    return sum(depths), sum(d >= 1 for d in depths)


def _fixture_tables(name):
    fx = fixture(name)
    names, lengths, table = counter_of_sam(fx["sam"])
    seqs = ref.fasta_sequences(open(fx["fa_path"]).read())
    refs = [seqs[n] for n in names]
    assert [len(r) for r in refs] == list(lengths)
    return fx, refs, table


@pytest.mark.parametrize("name", SETS)
@pytest.mark.parametrize("W", [1, 7, 400])
def test_restatement_against_samtools_depth(name, W):
    fx, refs, table = _fixture_tables(name)
    win, depth_hist, start_hist, totals = ref.coverage(table, b"".join(refs), W)
    total, lines = _depth_file(fx["depth"])
    assert total > 0 and int(win[:, 1].sum()) == total == int(totals[1])
    assert int(win[:, 3].sum()) == lines == int(totals[3])
    T = len(table)
    assert int(win[:, 0].sum()) == T == int(depth_hist.sum()) == int(start_hist.sum()) == int(totals[0])
    assert [int(v) for v in win[:, 0]] == [hi - lo for lo, hi in (ref.window_rows(w, T, W) for w in range(W))]
    assert int(depth_hist[0]) == T - lines


@pytest.mark.parametrize("name", SETS)
def test_the_two_restatements_agree_on_the_m_columns(name):
    """per window, the M columns the per-record walk counts are the depth the per-row walk sums; the records are the pileup's starts"""
    fx, refs, table = _fixture_tables(name)
    names, records = ref.records_of_sam(fx["sam"])
    (mapq_hist, win_mapq, pos_base, clip_hist, gc_hist, indel, indel_len, totals), invalid = ref.quality(records, refs, 7)
    win, _, _, ctot = ref.coverage(table, b"".join(refs), 7)
    assert not invalid and np.array_equal(win_mapq[:, 0], win[:, 1]) and int(totals[1]) == int(ctot[1])
    assert int(totals[0]) == len(records) == int(mapq_hist.sum()) >= int(ctot[5])
    assert int(pos_base.sum()) == int(totals[1] + totals[3]) and int(clip_hist.sum()) == int(totals[6])
    assert int(indel[0].sum()) == int(totals[2]) == int(indel_len[0].sum()) and int(indel[1].sum()) == int(totals[4]) == int(indel_len[1].sum())
    assert int(totals[5]) == int(ctot[6])  # deleted bases = deletion columns


@pytest.mark.parametrize("T", [1, 5, 64, 1000])
def test_window_formulas_agree(T):
    for W in sorted({1, 2, 7, T, T + 3, 65536}):
        by_range = np.full(T, -1, dtype=np.int64)
        for w in range(W):
            lo, hi = ref.window_rows(w, T, W)
            assert 0 <= lo <= hi <= T
            assert (by_range[lo:hi] == -1).all()
            by_range[lo:hi] = w
        assert by_range.tolist() == [ref.window_of_row(r, T, W) for r in range(T)]
        assert ref.longest_window(T, W) == -(-T // W)


def test_capacity_rule_arithmetic():
    assert not ref.capacity_refuses(0, 10, 3) and not ref.capacity_refuses(1 << 31, 1, 1)
    # depth^2 x rows of the longest window against 2^63, on either side of the bound
    assert not ref.capacity_refuses((1 << 31) - 1, 2, 1) and ref.capacity_refuses(1 << 31, 2, 1) and not ref.capacity_refuses(1 << 31, 2, 2)
    assert ref.capacity_refuses(3037000500, 1, 1) and not ref.capacity_refuses(3037000499, 1, 1)  # floor(sqrt(2^63)) = 3037000499
    table = np.zeros((4, 8), dtype=np.int64)
    table[2, 0] = 1 << 31
    assert ref.coverage(table, b"ACGT", 1) == ref.ERR_CAPACITY and ref.coverage(table, b"ACGT", 2) == ref.ERR_CAPACITY
    got = ref.coverage(table, b"ACGT", 4)
    assert int(got[0][2, 2]) == 1 << 62 and int(got[3][2]) == 1 << 31
    assert ref.coverage(table, b"ACGT", 0) == ref.ERR_INVALID and ref.coverage(table, b"ACGT", 65537) == ref.ERR_INVALID


def test_homopolymer_classes_of_the_restatement():
    """the rules of the header on cases worked by hand"""
    seq = b"CAAGTTTGCC"
    assert ref.indel_class(seq, 2, [0], False) == 4           # A inserted inside AA: l = 1, r = 1
    assert ref.indel_class(seq, 5, [3], False) == 3           # T inserted inside TTT: l = 1, r = 2
    assert ref.indel_class(seq, 4, [3], False) == 3           # before TTT: l = 0, r = 3
    assert ref.indel_class(seq, 7, [3, 3], False) == 3        # after TTT: l = 3
    assert ref.indel_class(seq, 7, [3, 0], False) == 4        # mixed bases
    assert ref.indel_class(seq, 7, [4], False) == 4           # N
    assert ref.indel_class(seq, 4, [3, 3, 3], True) == 3      # the whole run of three deleted
    assert ref.indel_class(seq, 1, [0], True) == 4            # one of AA deleted: 0 + 1 + 1
    assert ref.indel_class(seq, 9, [1], True) == 4            # the last base of CC: l = 1, nothing to its right
    assert ref.indel_class(b"AAA", 0, [0], False) == 0        # at a sequence's start: l = 0 whatever lies before it elsewhere, r = 3
    assert ref.indel_class(b"AAT", 0, [0], False) == 4        # ... and r = 2 is not enough


def test_the_gpu_cases_say_what_their_names_say():
    """the record shapes and homopolymer cases of tests/test_gpu_alignment_quality.py reach what they are there for, by the restatement"""
    from test_gpu_alignment_quality import HOMOPOLYMER_CASES, REFS, SHAPE_CASES
    (mapq_hist, win_mapq, _, clip_hist, _, _, _, totals), _ = ref.quality(SHAPE_CASES["m_run_over_three_windows"], REFS, 5)
    assert (win_mapq[:, 0] > 0).sum() == 3 and win_mapq[:, 1].tolist() == (17 * win_mapq[:, 0]).tolist()
    (_, _, _, clip_hist, _, _, _, totals), _ = ref.quality(SHAPE_CASES["clips"], REFS, 5)
    assert totals[6] == 5 + 7 + 5500 and totals[7] == 3 and (clip_hist[128:] > 0).sum() > 16   # (the long clips go across octaves)
    want = {"i_after_aa": (0, 4), "i_after_ttt": (0, 3), "i_before_aa": (0, 4), "i_before_ttt": (0, 3), "i_inside_aa": (0, 4), "i_inside_ttt": (0, 3),
            "d_of_a_whole_run_of_three": (1, 3), "d_of_mixed_bases": (1, 4), "mixed_base_insertion": (0, 4), "insertion_of_n": (0, 4),
            "i_before_the_first_column_of_the_second_sequence": (0, 0), "i_before_the_first_column_of_the_third_sequence": (0, 4),
            "d_ending_on_the_last_base_of_a_sequence": (1, 4), "i_at_the_end_of_a_sequence": (0, 4)}
    for case, (kind, cls) in want.items():
        (_, _, _, _, _, indel, _, _), invalid = ref.quality(HOMOPOLYMER_CASES[case], REFS, 1)
        assert not invalid and indel.sum() == 1 and indel[kind, cls] == 1, case
    (_, _, _, _, _, indel, _, _), _ = ref.quality(HOMOPOLYMER_CASES["d_of_part_of_a_run_of_two"], REFS, 1)
    assert indel[1].tolist() == [0, 0, 0, 0, 2]


class _Tables(object):
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _hand_tables(W=4, empty=False):
    B = ref.POS_BINS
    cov = _Tables(win=np.zeros((W, 8), dtype=np.int64), depth_hist=np.zeros(B, dtype=np.int64), start_hist=np.zeros(B, dtype=np.int64),
                  totals=np.zeros(8, dtype=np.int64))
    qual = _Tables(mapq_hist=np.zeros(256, dtype=np.int64), win_mapq=np.zeros((W, 2), dtype=np.int64), pos_base=np.zeros((B, 5), dtype=np.int64),
                   clip_hist=np.zeros(B, dtype=np.int64), gc_hist=np.zeros(102, dtype=np.int64), indel=np.zeros((2, 5), dtype=np.int64),
                   indel_len=np.zeros((2, B), dtype=np.int64), totals=np.zeros(8, dtype=np.int64))
    if empty:
        return cov, qual
    # 10 rows in 4 windows of 2, 3, 2, 3 rows; window 2 is left without coverage
    cov.win[:] = [[2, 7, 29, 2, 1, 2, 1, 0], [3, 30, 302, 3, 2, 3, 2, 1], [2, 0, 0, 0, 0, 1, 0, 2], [3, 18, 110, 2, 3, 3, 0, 0]]
    cov.depth_hist[[0, 2, 5, 9, 10, 11, 33]] = [3, 1, 1, 2, 1, 1, 1]   # bin 33 = depths 34-35
    cov.start_hist[[0, 1, 2]] = [8, 1, 1]
    cov.totals[:] = [10, 55, 35, 7, 2, 3, 3, 4]
    qual.mapq_hist[[0, 60, 255]] = [1, 1, 1]
    qual.win_mapq[:] = [[7, 420], [30, 1800], [0, 0], [18, 0]]
    qual.pos_base[0], qual.pos_base[1], qual.pos_base[20] = [3, 0, 0, 0, 0], [1, 1, 1, 0, 0], [10, 20, 30, 36, 4]
    qual.clip_hist[[0, 1, 40]] = [2, 1, 5]
    qual.gc_hist[[40, 50, 101]] = [1, 1, 1]
    qual.indel[:] = [[1, 0, 0, 2, 3], [0, 1, 0, 0, 1]]
    qual.indel_len[0, [1, 2]], qual.indel_len[1, [1, 16]] = [4, 2], [1, 1]
    qual.totals[:] = [3, 55, 6, 8, 2, 17, 8, 2]
    return cov, qual


def _parse(text):
    lines = text.split("\n")
    assert lines[0].startswith("#") and lines[-1] == ""
    return lines[0][1:].split("\t"), [line.split("\t") for line in lines[1:-1] if not line.startswith("#")], [line for line in lines[1:-1] if line.startswith("#")]


def _results(text):
    out, section = {}, None
    for line in text.split("\n"):
        if line.startswith(">>>>>>> "):
            section = line[8:]
        elif " = " in line:
            k, v = line.lstrip().split(" = ", 1)
            out[(section, k)] = v
    return out


def test_report_writer_on_hand_made_tables(tmp_path):
    from nanopore_amd.analyses import qualimap
    cov, qual = _hand_tables()
    texts = qualimap.reportTexts(cov, qual, "x.sam", "x.fa", 2)
    assert sorted(texts) == sorted(["genome_results.txt"] + [os.path.join(qualimap.RAW_DIR, f) for f in qualimap.RAW_FILES])
    raw = lambda name: _parse(texts[os.path.join(qualimap.RAW_DIR, name)])  # noqa: E731

    head, rows, _ = raw("coverage_across_reference.txt")
    assert head == ["Position (bp)", "Rows", "Mapped bases", "Coverage", "Std", "GC (%)", "Starts", "Deletion columns"] and len(rows) == 4
    assert [int(r[0]) for r in rows] == [1, 3, 6, 8]   # w * 10 // 4 + 1
    for w, r in enumerate(rows):
        n, total, squares, _, gc, acgt, starts, dels = (int(v) for v in cov.win[w])
        assert [int(r[1]), int(r[2]), int(r[6]), int(r[7])] == [n, total, starts, dels]
        assert float(r[3]) == total / n and float(r[4]) == math.sqrt(max(0.0, squares / n - (total / n) ** 2))
        assert float(r[5]) == (100.0 * (gc / acgt) if acgt else 0.0)
    assert float(rows[2][3]) == 0.0 and float(rows[2][4]) == 0.0

    _, rows, _ = raw("coverage_histogram.txt")
    assert [(r[0], int(r[1])) for r in rows] == [("0", 3), ("2", 1), ("5", 1), ("9", 2), ("10", 1), ("11", 1), ("34-35", 1)]
    _, rows, _ = raw("genome_fraction_coverage.txt")
    assert [r[0] for r in rows] == ["%d" % d for d in range(1, 32)] + ["32-33", "34-35"]
    assert [float(r[1]) for r in rows][:3] == [70.0, 70.0, 60.0] and float(rows[-1][1]) == 10.0 and float(rows[8][1]) == 100.0 * (5 / 10)
    _, rows, _ = raw("duplication_rate_histogram.txt")
    assert [(r[0], int(r[1])) for r in rows] == [("1", 1), ("2", 1)]
    _, rows, _ = raw("mapping_quality_across_reference.txt")
    assert [(int(r[0]), int(r[1]), float(r[2])) for r in rows] == [(1, 7, 60.0), (3, 30, 60.0), (6, 0, 0.0), (8, 18, 0.0)]
    _, rows, _ = raw("mapping_quality_histogram.txt")
    assert [(int(r[0]), int(r[1])) for r in rows] == [(0, 1), (60, 1), (255, 1)]
    _, rows, tail = raw("mapped_reads_gc-content_distribution.txt")
    assert [int(r[0]) for r in rows] == list(range(101)) and [int(r[1]) for r in rows] == [int(v) for v in qual.gc_hist[:101]]
    assert tail == ["#Records without A C G T\t1"]
    _, rows, _ = raw("mapped_reads_nucleotide_content.txt")
    assert [(r[0], int(r[1])) for r in rows] == [("1", 3), ("2", 3), ("21", 100)]
    assert [float(v) for v in rows[2][2:]] == [10.0, 20.0, 30.0, 36.0, 4.0] and [float(v) for v in rows[1][2:]] == [100.0 * (1 / 3)] * 3 + [0.0, 0.0]
    _, rows, _ = raw("mapped_reads_clipping_profile.txt")
    assert [(r[0], int(r[1]), float(r[2])) for r in rows] == [("1", 2, 100.0 * (2 / 5)), ("2", 1, 25.0), ("21", 0, 0.0), ("49-50", 5, 100.0)]
    _, rows, _ = raw("homopolymer_indels.txt")
    assert [(r[0], int(r[1]), int(r[2]), int(r[3])) for r in rows] == [("polyA", 1, 1, 0), ("polyC", 1, 0, 1), ("polyG", 0, 0, 0), ("polyT", 2, 2, 0),
                                                                      ("Non-homopolymer indels", 4, 3, 1)]

    res = _results(texts["genome_results.txt"])
    assert [s for s in ("Input", "Reference", "Globals", "ACGT Content", "Coverage", "Mapping Quality", "Mismatches and indels")
            if any(k[0] == s for k in res)] == ["Input", "Reference", "Globals", "ACGT Content", "Coverage", "Mapping Quality", "Mismatches and indels"]
    assert not any("nsert size" in k[0] for k in res)
    assert res[("Reference", "number of bases")] == "10 bp" and res[("Reference", "number of contigs")] == "2"
    assert res[("Globals", "number of mapped reads")] == "3" and res[("Globals", "number of mapped bases")] == "55 bp"
    assert res[("Globals", "number of clipped reads")] == "2" and res[("Globals", "number of clipped bases")] == "8 bp"
    assert res[("Globals", "duplication rate")] == repr(100.0 * ((3 - 2) / 3)) + "%"
    assert res[("ACGT Content", "number of A's")] == "14 bp (%s%%)" % repr(100.0 * (14 / 106))
    assert res[("ACGT Content", "GC percentage")] == repr(100.0 * ((21 + 31) / 102)) + "%"
    mean = 55 / 10
    assert res[("Coverage", "mean coverageData")] == repr(mean) + "X"
    assert res[("Coverage", "std coverageData")] == repr(math.sqrt(441 / 10 - mean * mean)) + "X"
    assert res[("Coverage", "genome fraction covered")] == "70.0%" and res[("Coverage", "largest depth")] == "35"
    assert res[("Mapping Quality", "mean mapping quality")] == repr((60 + 255) / 3)
    assert res[("Mismatches and indels", "number of insertions")] == "6" and res[("Mismatches and indels", "number of deleted bases")] == "17 bp"
    assert res[("Mismatches and indels", "homopolymer indels")] == repr(100.0 * (4 / 8)) + "%"

    qualimap.writeReport(str(tmp_path), texts)
    for name, text in texts.items():
        assert open(os.path.join(str(tmp_path), name)).read() == text


def test_report_writer_on_an_empty_mapping():
    """no record, no row: every ratio prints 0 and nothing divides by zero"""
    from nanopore_amd.analyses import qualimap
    cov, qual = _hand_tables(W=3, empty=True)
    texts = qualimap.reportTexts(cov, qual)
    _, rows, _ = _parse(texts[os.path.join(qualimap.RAW_DIR, "coverage_across_reference.txt")])
    assert [[float(v) for v in r] for r in rows] == [[0.0] * 8] * 3
    _, rows, _ = _parse(texts[os.path.join(qualimap.RAW_DIR, "mapping_quality_across_reference.txt")])
    assert [[float(v) for v in r] for r in rows] == [[0.0] * 3] * 3
    for name in ("coverage_histogram.txt", "genome_fraction_coverage.txt", "duplication_rate_histogram.txt", "mapping_quality_histogram.txt",
                 "mapped_reads_nucleotide_content.txt", "mapped_reads_clipping_profile.txt"):
        assert _parse(texts[os.path.join(qualimap.RAW_DIR, name)])[1] == []
    res = _results(texts["genome_results.txt"])
    assert res[("Coverage", "mean coverageData")] == "0.0X" and res[("Coverage", "std coverageData")] == "0.0X"
    assert res[("Globals", "duplication rate")] == "0.0%" and res[("Mapping Quality", "mean mapping quality")] == "0.0"
    assert res[("ACGT Content", "GC percentage")] == "0.0%" and res[("Mismatches and indels", "homopolymer indels")] == "0.0%"


def test_pipeline_finds_the_class_by_name_and_not_by_default():
    from nanopore_amd import pipeline
    from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
    from nanopore_amd.analyses.qualimap import QualiMap
    assert pipeline.resolveClasses("QualiMap", "nanopore_amd.analyses", AbstractAnalysis) == [QualiMap]
    assert QualiMap not in pipeline.analyses and "QualiMap" not in [c.__name__ for c in pipeline.analyses]


def test_binding_constants_are_the_headers():
    import re
    from helpers import ROOT
    from nanopore_amd import _lib
    text = open(os.path.join(ROOT, "include", "nprealign.h")).read()
    value = lambda name: int(re.search(r"#define %s (\d+)" % name, text).group(1))  # noqa: E731
    assert (_lib.AQ_MAX_WINDOWS, _lib.AQ_WIN_WORDS, _lib.AQ_TOTALS, _lib.AQ_HOMOPOLYMER, _lib.AQ_TILE) == tuple(
        value("NPR_AQ_" + n) for n in ("MAX_WINDOWS", "WIN_WORDS", "TOTALS", "HOMOPOLYMER", "TILE"))
    assert (ref.MAX_WINDOWS, ref.WIN_WORDS, ref.TOTALS, ref.HOMOPOLYMER) == (_lib.AQ_MAX_WINDOWS, _lib.AQ_WIN_WORDS, _lib.AQ_TOTALS, _lib.AQ_HOMOPOLYMER)

"""The device pileup's host side (nanopore_amd/analyses/pileup.py, nanopore_amd/metaAnalyses/) against fixtures RECORDED FROM THE REFERENCE'S
PROGRAM: tests/golden/pileup/ holds two sets of SAM records and what samtools 0.1.19 -- built from the source the reference ships, by
tests/golden/make_pileup_golden.py -- printed for them with `samtools depth` and `samtools mpileup -B -Q 0 -q 0 -d 1000000`.

This module also holds what tests/test_gpu_pileup.py compares the device table with: the parser of mpileup's text and an independent counter
that walks a SAM text one alignment column at a time (no run arithmetic).  What the parser knows about mpileup's fifth column: `*` is a
deletion column; `^` and one mapping quality character mark a record's first column, `$` its last; `+<n><n characters>` an insertion and
`-<n><n characters>` an announced deletion after the column they follow; every other character is the read base of an M column.  The
characters mpileup prints for an insertion that follows a deletion column are garbage, so only the NUMBER of `+<n>` markers is used."""
import os

import numpy as np
import pytest

from helpers import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", "pileup")
SETS = ("local", "global")
WORDS = 8
DROPPED_FLAGS = 0x4 | 0x100 | 0x200 | 0x400   # what samtools' pileup leaves out (BAM_DEF_MASK); stated here, not taken from the product


def fixture(name):
    def text(suffix):
        with open(os.path.join(GOLD, name + suffix)) as f:
            return f.read()
    return dict(sam=text(".sam"), depth=text(".depth.txt"), mpileup=text(".mpileup.txt"), sam_path=os.path.join(GOLD, name + ".sam"),
                fa_path=os.path.join(GOLD, name + ".fa"))


def sam_contigs(sam_text):
    """(names, lengths) of the @SQ lines, in order."""
    names, lengths = [], []
    for line in sam_text.split("\n"):
        if line.startswith("@SQ"):
            tags = dict(f.split(":", 1) for f in line.split("\t")[1:])
            names.append(tags["SN"]), lengths.append(int(tags["LN"]))
    return names, lengths


def sam_records(sam_text):
    """(flag, contig name, 0-based position, [(op letter, length)], SEQ) of every alignment line."""
    out = []
    for line in sam_text.split("\n"):
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        cigar, num = [], ""
        for ch in f[5]:
            if ch.isdigit():
                num += ch
            else:
                cigar.append((ch, int(num)))
                num = ""
        out.append((int(f[1]), f[2], int(f[3]) - 1, cigar, f[9]))
    return out


def count_columns(table, row0, cigar, seq, y=0):
    """One record into table[row][WORDS], one alignment column at a time: cigar = [(op letter M I D S H, length)], row0 = the row of its first
    reference position, seq[y] = the read base of its first column that has one."""
    x, have_column, previous = row0, False, None
    for ch in "".join(op * n for op, n in cigar):
        if ch == "H":
            continue
        if ch == "S":
            y += 1
            continue
        if ch == "M":
            table[x, "ACGT".find(seq[y].upper()) if seq[y].upper() in "ACGT" else 4] += 1
        elif ch == "D":
            table[x, 5] += 1
        if ch in "MD":
            if not have_column:
                table[x, 7] += 1
            have_column = True
            x += 1
        if ch in "MI":
            y += 1
        if ch == "I" and have_column and previous != "I":
            table[x - 1, 6] += 1
        previous = ch


def counter_of_sam(sam_text):
    """(names, lengths, table[sum lengths][WORDS]) over the records samtools' pileup keeps."""
    names, lengths = sam_contigs(sam_text)
    first = dict(zip(names, np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()))
    table = np.zeros((sum(lengths), WORDS), dtype=np.int64)
    for flag, contig, pos, cigar, seq in sam_records(sam_text):
        if flag & DROPPED_FLAGS or contig == "*":
            continue
        count_columns(table, first[contig] + pos, cigar, seq)
    return names, lengths, table


def parse_mpileup(text, names, lengths):
    """table[sum lengths][WORDS] from the text of `samtools mpileup`, and per row the depth its fourth column states (-1: no line)."""
    first = dict(zip(names, np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()))
    table = np.zeros((sum(lengths), WORDS), dtype=np.int64)
    stated = np.full(sum(lengths), -1, dtype=np.int64)
    for line in text.split("\n"):
        if not line:
            continue
        f = line.split("\t")
        row, s = first[f[0]] + int(f[1]) - 1, f[4]
        assert stated[row] == -1, "two lines for one position"
        stated[row] = int(f[3])
        i = 0
        while i < len(s):
            c = s[i]
            if c == "^":
                table[row, 7] += 1
                i += 2
            elif c == "$":
                i += 1
            elif c in "+-":
                j = i + 1
                while s[j].isdigit():
                    j += 1
                table[row, 6] += c == "+"
                i = j + int(s[i + 1:j])
            elif c == "*":
                table[row, 5] += 1
                i += 1
            else:
                assert c.isalpha(), (line, c)
                table[row, "ACGT".find(c.upper()) if c.upper() in "ACGT" else 4] += 1
                i += 1
    return table, stated


@pytest.mark.parametrize("name", SETS)
def test_fixture_base_characters_number_the_depth(name):
    """The parser against the other program's output: at every position the base characters of mpileup's fifth column number exactly the
    depth `samtools depth` prints, the two programs list the same positions, and the fourth column is bases + deletion columns."""
    fx = fixture(name)
    names, lengths = sam_contigs(fx["sam"])
    table, stated = parse_mpileup(fx["mpileup"], names, lengths)
    first = dict(zip(names, np.concatenate([[0], np.cumsum(lengths)[:-1]]).tolist()))
    depth = np.full(sum(lengths), -1, dtype=np.int64)
    for line in fx["depth"].split("\n"):
        if line:
            f = line.split("\t")
            depth[first[f[0]] + int(f[1]) - 1] = int(f[2])
    assert (depth >= 0).sum() > 500
    assert ((depth >= 0) == (stated >= 0)).all()
    listed = depth >= 0
    assert (table[listed, :5].sum(axis=1) == depth[listed]).all()
    assert (table[listed, :6].sum(axis=1) == stated[listed]).all() and (table[~listed] == 0).all()
    assert (table[listed, :6].sum(axis=1) > 0).all()
    kept = [r for r in sam_records(fx["sam"]) if not r[0] & DROPPED_FLAGS]
    assert table[:, 7].sum() == len(kept) and table[:, 5].sum() > 0 and table[:, 6].sum() > 0 and table[:, 4].sum() > 0
    if name == "global":
        assert (depth[listed] == 0).any()  # positions under deletions alone have a line with depth 0
    else:
        assert stated[first["ctgNone"]:].max() == -1 and {4, 256, 512, 1024, 2048} <= {r[0] & ~16 for r in sam_records(fx["sam"])}


@pytest.mark.parametrize("name", SETS)
def test_column_counter_equals_mpileup(name):
    """The definition of the eight words (include/nprealign.h), walked one column at a time, is what mpileup printed: every word, every position."""
    fx = fixture(name)
    names, lengths, table = counter_of_sam(fx["sam"])
    want, _ = parse_mpileup(fx["mpileup"], names, lengths)
    assert np.array_equal(table, want), np.argwhere(table != want)[:10]


@pytest.mark.parametrize("name", SETS)
def test_depth_text_reproduces_samtools_depth(name):
    from nanopore_amd.analyses.pileup import depth_text
    fx = fixture(name)
    names, lengths, table = counter_of_sam(fx["sam"])
    got = depth_text(names, lengths, table[:, :5].sum(axis=1), table[:, :6].sum(axis=1) != 0)
    assert got == fx["depth"]


def test_flag_mask():
    from nanopore_amd.analyses import pileup
    assert pileup.FLAG_MASK == 0x4 | 0x100 | 0x200 | 0x400 == DROPPED_FLAGS
    flags = [0, 16, 4, 256, 512, 1024, 2048, 2048 | 16, 4 | 16, 1, 2, 32, 64, 128, 256 | 2048, 0x4 | 0x100 | 0x200 | 0x400]
    want = [True, True, False, False, False, False, True, True, False, True, True, True, True, True, False, False]
    assert pileup.kept_by_samtools(flags).tolist() == want
    # ... and that is what samtools did with the fixture's records: mpileup shows one `^` per kept record
    fx = fixture("local")
    names, lengths = sam_contigs(fx["sam"])
    table, _ = parse_mpileup(fx["mpileup"], names, lengths)
    assert table[:, 7].sum() == int(pileup.kept_by_samtools([r[0] for r in sam_records(fx["sam"])]).sum()) < len(sam_records(fx["sam"]))


def test_coverage_stats_selection_and_header():
    """_Stats.out on a depth vector worked by hand.  Depths 2 2 6 6 10 1 5 (one contig, positions 1 2 3 7 8 9 10): mean 32 / 7, population
    variance (4 + 4 + 36 + 36 + 100 + 1 + 25) / 7 - (32 / 7)^2 = 206 / 7 - 1024 / 49 = 418 / 49, sd = sqrt(418) / 7 = 2.9207..., threshold
    5.8414...: no line qualifies, the first one included (2 - 0 < 5.84)."""
    from nanopore_amd.metaAnalyses.coverageDepth import coverageStats
    seqs = {"c": "acgtTGCAAC", "d": "GGGGGGGGGG"}
    text = "".join("c\t%d\t%d\n" % pd for pd in [(1, 2), (2, 2), (3, 6), (7, 6), (8, 10), (9, 1), (10, 5)])
    assert coverageStats(text, seqs) == "Position\tCoverage (mu=4.57142857143X, sd=2.92072118575X)\tKmer\n"
    # depths 4 0 4 0 (mean 2, sd 2, threshold 4): a jump of EXACTLY 2 sd is kept; the first line compares against 0; positions below 5 take
    # the short k-mer, position 5 and beyond the five bases that end there; the k-mer comes from the line's own contig, upper case
    text = "c\t2\t4\nc\t3\t0\nc\t7\t4\nd\t1\t0\n"
    assert coverageStats(text, seqs) == "Position\tCoverage (mu=2.0X, sd=2.0X)\tKmer\n2\t4\tAC\n7\t4\tGTTGC\n"
    # depths 1 9 1 9 9 (mean 29 / 5 = 5.8, variance 245 / 5 - 5.8^2 = 15.36, sd 3.919..., threshold 7.838...: a jump of 8): lines 2 and 4; the line after a kept one compares
    # against that line's depth
    text = "d\t1\t1\nc\t5\t9\nc\t6\t1\nd\t4\t9\nd\t5\t9\n"
    assert coverageStats(text, seqs) == "Position\tCoverage (mu=5.8X, sd=3.91918358845X)\tKmer\n5\t9\tACGTT\n4\t9\tGGGG\n"


def test_meta_analysis_base_class():
    from nanopore_amd.metaAnalyses.abstractMetaAnalysis import AbstractMetaAnalysis
    from nanopore_amd.metaAnalyses.coverageDepth import CoverageDepth

    class LastzParams(object):
        pass

    class Bwa(object):
        pass

    ex = [("r.fq", "2D", "ref.fa", LastzParams, [], "/out/exp1"), ("r.fq", "2D", "ref.fa", Bwa, [], "/out/exp2")]
    m = AbstractMetaAnalysis("/out", ex)
    assert m.baseMappers == {"Lastz", "Bwa"} and m.readTypes == {"2D"} and m.readFastqFiles == {("r.fq", "2D")}
    assert m.experimentHash[(("r.fq", "2D"), "ref.fa", Bwa)] == ([], "/out/exp2") and m.outputDir == "/out"
    assert issubclass(CoverageDepth, AbstractMetaAnalysis)

"""QualiMap: genome_results.txt and raw_data_qualimapReport/*.txt -- QualiMap bamqc's layout, this build's definitions.

nanopore/analyses/qualimap.py converts the SAM file to BAM, sorts it and hands it to the Java program `qualimap bamqc`, which
this build cannot run.  Here the records are counted on the device where the pileup already lies: `npr_pileup_coverage` reduces
the pileup's table to windows of the concatenated reference, `npr_align_quality` makes one pass over the records with the
reference bases beside them (include/nprealign.h defines every table in exact integer terms: windows, the position bins of
sixteen per octave, base codes, homopolymer classes).  Both run from one parse of the SAM file (`alignment_quality_of_sam`,
analyses/pileup.py) over the records samtools' pileup keeps.  The report is written from the tables by `reportTexts`, pure
Python.  The file names and the `>>>>>>> Section` layout of genome_results.txt are bamqc's (QualimapManual, "Output"); every
number is this build's and is defined below -- no file is byte-comparable with the Java tool's.  No CPU fallback.

Left out: the sections that need paired ends (insert size), the error rate and mismatch counts (they need NM / MD tags) and the
per-chromosome statistics (the windows ignore sequence boundaries, as QualiMap's do); plots and HTML.
Unlike the reference's wrapper, a file whose records carry no quality line is NOT skipped: no table needs one.

In every file a line that begins with `#` names the tab-separated columns.  x / y is float division printed with repr(), and 0
when y is 0.  `bin` is a position bin of the header: its label is `lo` when it holds one value, else `lo-hi`, both inclusive
(positions in a read are printed 1-based, depths and counts as they are).

genome_results.txt
  Input: the two file names and the number of windows.
  Reference: number of bases = T (rows), number of contigs.
  Globals: number of mapped reads = records the per-record pass counted; number of mapped bases = sum of depth (M columns);
    number of clipped reads / bases = records with a soft clip / soft-clipped bases; duplication rate = 100 x (records -
    positions that begin at least one record) / records, from the start histogram.
  ACGT Content: the read bases M and I runs consume, by code, each with 100 x n / all such bases; GC percentage =
    100 x (C + G) / (A + C + G + T).
  Coverage: mean = depth sum / T; std = sqrt(max(0, sum of depth^2 / T - mean^2)), the population value; genome fraction covered
    = 100 x rows with depth >= 1 / T; largest depth.
  Mapping Quality: mean = sum of q x mapq_hist[q] / records.
  Mismatches and indels: I runs, inserted bases, D runs, deleted bases, and homopolymer indels = 100 x runs of class 0..3 /
    all I and D runs.
raw_data_qualimapReport/
  coverage_across_reference.txt  per window: 1-based first row, rows, mapped bases (depth sum), mean = depth sum / rows, std as above
    over the window's rows, GC = 100 x reference (G + C) / (A + C + G + T), record starts, deletion columns.  An empty window is zeros.
  coverage_histogram.txt  per non-empty depth bin: rows.
  genome_fraction_coverage.txt  per depth bin from depth 1 to the last non-empty one: 100 x rows in this bin and above / T -- the
    fraction of the reference covered at least `lo` times, exact at a bin's lower edge.
  duplication_rate_histogram.txt  per non-empty bin of k >= 1: positions that begin k records.
  mapping_quality_across_reference.txt  per window: 1-based first row, M columns, mean = sum of MAPQ over them / M columns.
  mapping_quality_histogram.txt  per MAPQ with a record: records.
  mapped_reads_gc-content_distribution.txt  per G + C percentage 0..100 (rounded half up): records; the records without an A C G T
    base are the line `#Records without A C G T` after it.
  mapped_reads_nucleotide_content.txt  per non-empty position bin: bases, then A C G T N as 100 x n / bases.
  mapped_reads_clipping_profile.txt  per position bin with a clipped or an aligned base: clipped positions, and 100 x clipped /
    (clipped + read bases an M or I run consumes there).
  homopolymer_indels.txt  polyA polyC polyG polyT and `Non-homopolymer indels`: I runs + D runs of the class, then the two alone.
"""
import math
import os

import numpy as np

from .abstractAnalysis import AbstractAnalysis
from .fastqc import POS_BINS, binRange

RAW_DIR = "raw_data_qualimapReport"
RAW_FILES = ("coverage_across_reference.txt", "coverage_histogram.txt", "genome_fraction_coverage.txt", "duplication_rate_histogram.txt",
             "mapping_quality_across_reference.txt", "mapping_quality_histogram.txt", "mapped_reads_gc-content_distribution.txt",
             "mapped_reads_nucleotide_content.txt", "mapped_reads_clipping_profile.txt", "homopolymer_indels.txt")
INDEL_CLASSES = ("polyA", "polyC", "polyG", "polyT", "Non-homopolymer indels")


def ratio(x, y):
    """x / y, 0.0 when y is 0"""
    return float(x) / float(y) if y else 0.0


def meanStd(total, squares, n):
    """(mean, population standard deviation) of n values with this sum and sum of squares; (0, 0) when n is 0"""
    if not n:
        return 0.0, 0.0
    mean = float(total) / n
    return mean, math.sqrt(max(0.0, float(squares) / n - mean * mean))


def windowStart(w, T, W):
    """first row of window w"""
    return w * T // W


def binLabel(b, one_based=False):
    lo, hi = binRange(b)
    lo, hi = (lo + 1, hi) if one_based else (lo, hi - 1)
    return "%d" % lo if hi == lo else "%d-%d" % (lo, hi)


def _table(header, rows, tail=()):
    return "".join(["#" + "\t".join(header) + "\n"] + ["\t".join(x if isinstance(x, str) else repr(x) if isinstance(x, float) else "%d" % x for x in row) + "\n"
                                                         for row in rows] + [line + "\n" for line in tail])


def reportTexts(coverage, quality, samFile="", referenceFastaFile="", n_contigs=1):
    """{relative path: text} of the whole report, from a Coverage and an AlignQuality (realign.py; any objects with those fields)."""
    win, depth_hist, start_hist, ctot = (np.asarray(x) for x in (coverage.win, coverage.depth_hist, coverage.start_hist, coverage.totals))
    win_mapq, pos_base, clip_hist = np.asarray(quality.win_mapq), np.asarray(quality.pos_base), np.asarray(quality.clip_hist)
    qtot = [int(x) for x in quality.totals]
    W, T = len(win), int(ctot[0])
    out = {}

    def raw(name, text):
        out[os.path.join(RAW_DIR, name)] = text

    rows = []
    for w in range(W):
        n, total, squares, _, gc, acgt, starts, dels = (int(x) for x in win[w])
        mean, std = meanStd(total, squares, n)
        rows.append((windowStart(w, T, W) + 1 if n else 0, n, total, mean, std, 100.0 * ratio(gc, acgt), starts, dels))
    raw("coverage_across_reference.txt", _table(("Position (bp)", "Rows", "Mapped bases", "Coverage", "Std", "GC (%)", "Starts", "Deletion columns"), rows))
    raw("coverage_histogram.txt", _table(("Coverage", "Number of genomic locations"), [(binLabel(b), int(c)) for b, c in enumerate(depth_hist) if c]))
    nonzero = [b for b in range(1, POS_BINS) if depth_hist[b]]
    above = np.cumsum(depth_hist[::-1])[::-1]
    raw("genome_fraction_coverage.txt", _table(("Coverage (X)", "Coverage (%)"), [(binLabel(b), 100.0 * ratio(int(above[b]), T)) for b in range(1, (nonzero[-1] + 1) if nonzero else 1)]))
    raw("duplication_rate_histogram.txt", _table(("Duplication rate", "Start positions"), [(binLabel(b), int(start_hist[b])) for b in range(1, POS_BINS) if start_hist[b]]))
    raw("mapping_quality_across_reference.txt", _table(("Position (bp)", "Columns", "Mean mapping quality"),
                                                       [(windowStart(w, T, W) + 1 if int(win[w, 0]) else 0, int(win_mapq[w, 0]), ratio(int(win_mapq[w, 1]), int(win_mapq[w, 0])))
                                                        for w in range(W)]))
    raw("mapping_quality_histogram.txt", _table(("Mapping quality", "Records"), [(q, int(c)) for q, c in enumerate(quality.mapq_hist) if c]))
    raw("mapped_reads_gc-content_distribution.txt", _table(("GC Content (%)", "Records"), [(p, int(quality.gc_hist[p])) for p in range(101)],
                                                           tail=["#Records without A C G T\t%d" % int(quality.gc_hist[101])]))
    rows, clip_rows = [], []
    for b in range(POS_BINS):
        counts = [int(x) for x in pos_base[b]]
        bases, clipped = sum(counts), int(clip_hist[b])
        if bases:
            rows.append((binLabel(b, True), bases) + tuple(100.0 * ratio(x, bases) for x in counts))
        if bases or clipped:
            clip_rows.append((binLabel(b, True), clipped, 100.0 * ratio(clipped, clipped + bases)))
    raw("mapped_reads_nucleotide_content.txt", _table(("Position (bp)", "Bases", "A", "C", "G", "T", "N"), rows))
    raw("mapped_reads_clipping_profile.txt", _table(("Position (bp)", "Clipped bases", "Clipping profile (%)"), clip_rows))
    indel = np.asarray(quality.indel)
    raw("homopolymer_indels.txt", _table(("Type of indel", "Number of indels", "Insertions", "Deletions"),
                                         [(name, int(indel[0, c] + indel[1, c]), int(indel[0, c]), int(indel[1, c])) for c, name in enumerate(INDEL_CLASSES)]))

    # genome_results.txt
    by_code = [int(x) for x in pos_base.sum(axis=0)]
    all_bases = sum(by_code)
    records = qtot[0]
    mean, std = meanStd(int(ctot[1]), int(win[:, 2].sum()) if W else 0, T)
    begun = int(start_hist[1:].sum())
    runs = int(indel.sum())
    lines = ["BamQC report", "-----------------------------------", ""]

    def section(name, pairs):
        lines.extend([">>>>>>> " + name, ""])
        lines.extend("     %s = %s" % (k, v) for k, v in pairs)
        lines.extend(["", ""])

    pct = lambda x, y: repr(100.0 * ratio(x, y)) + "%"  # noqa: E731
    section("Input", [("sam file", samFile), ("reference file", referenceFastaFile), ("number of windows", W)])
    section("Reference", [("number of bases", "%d bp" % T), ("number of contigs", n_contigs)])
    section("Globals", [("number of mapped reads", records), ("number of mapped bases", "%d bp" % int(ctot[1])), ("number of clipped reads", qtot[7]),
                        ("number of clipped bases", "%d bp" % qtot[6]), ("duplication rate", pct(records - begun, records))])
    section("ACGT Content", [("number of %s's" % name, "%d bp (%s)" % (n, pct(n, all_bases))) for name, n in zip("ACGTN", by_code)] +
            [("GC percentage", pct(by_code[1] + by_code[2], sum(by_code[:4])))])
    section("Coverage", [("mean coverageData", repr(mean) + "X"), ("std coverageData", repr(std) + "X"), ("genome fraction covered", pct(int(ctot[3]), T)),
                         ("largest depth", int(ctot[2]))])
    section("Mapping Quality", [("mean mapping quality", repr(ratio(sum(q * int(c) for q, c in enumerate(quality.mapq_hist)), records)))])
    section("Mismatches and indels", [("number of insertions", qtot[2]), ("number of inserted bases", "%d bp" % qtot[3]), ("number of deletions", qtot[4]),
                                      ("number of deleted bases", "%d bp" % qtot[5]), ("homopolymer indels", pct(int(indel[:, :4].sum()), runs))])
    out["genome_results.txt"] = "\n".join(lines)
    return out


def writeReport(outputDir, texts):
    os.makedirs(os.path.join(outputDir, RAW_DIR), exist_ok=True)
    for name, text in texts.items():
        with open(os.path.join(outputDir, name), "w") as outf:
            outf.write(text)


class QualiMap(AbstractAnalysis):
    """Alignment-quality report of the experiment's mapping: coverage, mapping quality, clipping, GC and indels, counted on the device"""
    n_windows = 400  # bamqc's default

    def run(self, ctx=None):
        AbstractAnalysis.run(self)
        from .pileup import alignment_quality_of_sam
        from .utils import _context
        ctx = ctx or _context()
        names, _, coverage, quality = alignment_quality_of_sam(ctx, self.samFile, self.referenceFastaFile, self.n_windows)
        writeReport(self.outputDir, reportTexts(coverage, quality, os.path.basename(self.samFile), os.path.basename(self.referenceFastaFile), len(names)))
        self.finish()

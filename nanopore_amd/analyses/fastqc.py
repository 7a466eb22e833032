"""FastQC: fastqc_data.txt, fastqc_data_mapped.txt, fastqc_data_unmapped.txt -- FastQC's layout, this build's definitions.

nanopore/analyses/fastqc.py hands the read file to the Java program `fastqc`, which this build cannot run.  Here the reads'
base and quality bytes are counted on the device in one pass (`npr_read_quality`, include/nprealign.h, which defines every
table in exact integer terms: position bins of sixteen per octave, 95 quality columns, five base columns, per-read length,
mean quality and G + C percentage, totals), split into the reads the experiment's SAM file maps and those it does not --
the join of FASTQ names with SAM QNAMEs the unmapped-read meta-analyses use (`npr_names_mark`).  The report is written from
the tables by `writeFastqcData`, pure Python: the text layout of FastQC's fastqc_data.txt (`##FastQC` line, then per module
`>>Name<TAB>status`, a `#` header line, tab-separated rows, `>>END_MODULE`), with the statistics and the pass / warn / fail
rules stated beside each module below.  No file is byte-comparable with the Java tool's: the position bins, the percentile
rule and the thresholds are this build's.  The duplication, over-represented-sequence and k-mer modules are left out: long
reads do not repeat, and KmerAnalysis counts the k-mers.  A record whose quality line is not as long as its sequence is
left out of every table and counted in the `#Malformed records` line of Basic Statistics.  No CPU fallback.
"""
import os

import numpy as np

from .. import realign
from ..ingest import FastqTable, SamText
from .abstractAnalysis import AbstractAnalysis

VERSION = "nanopore_amd read-quality tables 1"
POS_BINS, QUAL_COLS = 336, 95


def posBin(p):
    """The position bin of p (include/nprealign.h): p below 16, then sixteen bins per octave; 335 from 2^24 on."""
    if p < 16:
        return p
    if p >= 1 << 24:
        return POS_BINS - 1
    e = p.bit_length() - 1
    return 16 * (e - 3) + ((p >> (e - 4)) & 15)


def binRange(b):
    """[lo, hi) of the positions of bin b."""
    if b < 16:
        return b, b + 1
    lo, width = (16 + b % 16) << (b // 16 - 1), 1 << (b // 16 - 1)
    return lo, lo + width


def percentile(hist, k):
    """The smallest value whose cumulative count reaches ceil(total * k / 100); hist: counts per value, total > 0."""
    total = int(sum(int(c) for c in hist))
    need, cum = (total * k + 99) // 100, 0
    for value, count in enumerate(hist):
        cum += int(count)
        if cum >= need and cum > 0:
            return value
    raise ValueError("an empty histogram has no percentile")


def mergeTables(a, b):
    """The tables of the union of two disjoint sets of reads: counts add; of the extremes the smaller / larger that is set."""
    out = realign.ReadQuality(*[x + y for x, y in zip(a.arrays(), b.arrays())])
    for w, pick in ((2, min), (3, max), (4, min), (5, max)):
        have = [int(t[w]) for t in (a.totals, b.totals) if t[w] >= 0]
        out.totals[w] = pick(have) if have else -1
    return out


def _worst(flags):
    """[(warn?, fail?)] -> status"""
    return "fail" if any(f for _, f in flags) else "warn" if any(w for w, _ in flags) else "pass"


def _label(b, one_based):
    lo, hi = binRange(b)
    if one_based:
        return "%d" % (lo + 1) if hi - lo == 1 else "%d-%d" % (lo + 1, hi)
    return "%d-%d" % (lo, hi - 1)


def fastqcDataText(tables, filename, malformed=0):
    """The report of one set of tables (ReadQuality without a group axis) as text."""
    pos_qual, pos_base, totals = np.asarray(tables.pos_qual), np.asarray(tables.pos_base), [int(x) for x in tables.totals]
    out = ["##FastQC\t%s" % VERSION]

    def module(name, status, header, rows):
        out.append(">>%s\t%s" % (name, status))
        out.append("#" + "\t".join(header))
        out.extend("\t".join(str(x) for x in row) for row in rows)
        out.append(">>END_MODULE")

    # Basic Statistics (no rule)
    acgt, gc = int(pos_base[:, :4].sum()), int(pos_base[:, 1:3].sum())
    module("Basic Statistics", "pass", ["Measure", "Value"], [
        ("Filename", filename), ("File type", "Conventional base calls"),
        ("Encoding", "Sanger / Illumina 1.9" if totals[4] < 64 else "Illumina 1.5"), ("Total Sequences", totals[0]),
        ("Sequence length", "%d-%d" % (max(totals[2], 0), max(totals[3], 0))), ("%GC", (200 * gc + acgt) // (2 * acgt) if acgt else 0),
        ("#Malformed records", malformed)])

    # Per base sequence quality: per non-empty bin, over the quality columns 0..93; warn: lower quartile < 10 or median < 25, fail: < 5 or < 20
    rows, flags = [], []
    for b in range(POS_BINS):
        h = [int(c) for c in pos_qual[b, :QUAL_COLS - 1]]
        total = sum(h)
        if total == 0:
            continue
        mean = float(sum(q * c for q, c in enumerate(h))) / total
        med, lq, uq, p10, p90 = (percentile(h, k) for k in (50, 25, 75, 10, 90))
        rows.append((_label(b, True), repr(mean), med, lq, uq, p10, p90))
        flags.append((lq < 10 or med < 25, lq < 5 or med < 20))
    module("Per base sequence quality", _worst(flags), ["Base", "Mean", "Median", "Lower Quartile", "Upper Quartile", "10th Percentile", "90th Percentile"], rows)

    # Per sequence quality scores: warn when the most frequent mean is < 27, fail when < 20
    meanq = [int(c) for c in tables.meanq_hist[:QUAL_COLS - 1]]
    top = max(range(len(meanq)), key=lambda q: (meanq[q], -q)) if sum(meanq) else None
    module("Per sequence quality scores", _worst([(top < 27, top < 20)] if top is not None else []), ["Quality", "Count"],
           [(q, c) for q, c in enumerate(meanq) if c])

    # Per base sequence content: percentages of A + C + G + T per bin; warn when |A - T| or |G - C| exceeds 10 points in a bin, fail over 20
    rows, flags = [], []
    n_rows = []
    for b in range(POS_BINS):
        a, c, g, t, other = (int(x) for x in pos_base[b])
        n = a + c + g + t
        if n + other == 0:
            continue
        pg, pa, pt, pc = ((100.0 * x / n if n else 0.0) for x in (g, a, t, c))
        rows.append((_label(b, True), repr(pg), repr(pa), repr(pt), repr(pc)))
        diff = max(abs(pa - pt), abs(pg - pc))
        flags.append((diff > 10, diff > 20))
        n_rows.append((_label(b, True), 100.0 * other / (n + other)))
    module("Per base sequence content", _worst(flags), ["Base", "G", "A", "T", "C"], rows)

    # Per sequence GC content (no rule)
    module("Per sequence GC content", "pass", ["GC Content", "Count"], [(p, int(tables.gc_hist[p])) for p in range(101)])

    # Per base N content: warn when any bin is over 5 %, fail over 20 %
    module("Per base N content", _worst([(p > 5, p > 20) for _, p in n_rows]), ["Base", "N-Count"], [(label, repr(p)) for label, p in n_rows])

    # Sequence Length Distribution: warn when more than one bin is non-empty, fail when any read is empty
    rows = [(_label(b, False), int(c)) for b, c in enumerate(tables.len_hist) if c]
    module("Sequence Length Distribution", _worst([(len(rows) > 1, totals[6] > 0)]), ["Length", "Count"], rows)
    return "\n".join(out) + "\n"


def writeFastqcData(path, tables, filename, malformed=0):
    with open(path, "w") as outf:
        outf.write(fastqcDataText(tables, filename, malformed))


class FastQC(AbstractAnalysis):
    """Read-quality report of the experiment's reads, and of those its mapping places and does not place"""

    def run(self, ctx=None):
        AbstractAnalysis.run(self)
        from .utils import _context
        ctx = ctx or _context()
        table, sam = FastqTable(self.readFastqFile), SamText(self.samFile)
        mapped = np.zeros(len(table), dtype=np.uint8)
        try:
            realign.names_mark(table.text, table.name_span, sam.text, sam.span, sam.parse(), mapped)
        except realign.NprError:
            raise ValueError("%s: an alignment line that does not parse, or an RNAME that is not among the header's @SQ lines" % sam.path)
        qual = table.qual_span
        group = np.where(mapped != 0, 0, 1).astype(np.int32)
        bad = (qual[:, 1] - qual[:, 0]) != table.lengths
        group[bad] = -1
        both = ctx.read_quality(table.text, table.seq_span, qual, group, 2)
        name = os.path.basename(self.readFastqFile)
        malformed = [int((bad & (mapped != 0)).sum()), int((bad & (mapped == 0)).sum())]
        writeFastqcData(os.path.join(self.outputDir, "fastqc_data.txt"), mergeTables(both.group(0), both.group(1)), name, sum(malformed))
        writeFastqcData(os.path.join(self.outputDir, "fastqc_data_mapped.txt"), both.group(0), name, malformed[0])
        writeFastqcData(os.path.join(self.outputDir, "fastqc_data_unmapped.txt"), both.group(1), name, malformed[1])
        self.finish()

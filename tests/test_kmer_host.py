"""KmerAnalysis / IndelKmerAnalysis, the parts that need no GPU (nanopore/analyses/kmerAnalysis.py, indelKmerAnalysis.py).

The yardstick of the device tests (tests/test_gpu_kmer.py) lives here: `literal_walk` restates the reference's column walk
through an ordered set word for word, `run_length_walk` is the formulation k_indel_kmers implements (csrc/npr_kmer.hip), and
the two are pinned against each other on random cigars.  The host composition -- reverse-complement / reversal permutations
of the bins, fractions, Inf cases, row order, file-written-or-not -- is checked against `collections.Counter` over strings,
the way the reference counts, with the device replaced by Python slices."""
import ctypes
import itertools
import os
import random
from collections import Counter
from math import log

import numpy as np
import pytest

from nanopore_amd import _lib, bioio
from nanopore_amd.analyses import indelKmerAnalysis as IK
from nanopore_amd.analyses import kmerAnalysis as KA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = "kmer\trefCount\trefFraction\treadCount\treadFraction\tlogFoldChange\n"


# ---- the reference's definitions, restated ----

def fold(seq):
    """The library's alphabet: letter case folded, everything outside ACGT is N."""
    return "".join(c if c in "ACGT" else "N" for c in seq.upper())


def columns(cigar, side):
    """Alignment columns of one side (0: read -- a position for M / I, None for D; 1: reference -- M / D, None for I)."""
    gap = 2 if side == 0 else 1
    out, p = [], 0
    for op, ln in cigar:
        for _ in range(ln):
            if op == gap:
                out.append(None)
            else:
                out.append(p)
                p += 1
    return out


def literal_walk(aligned, k):
    """indelKmerAnalysis.py:11-19 with UniqueList (an ordered set: `add` of a present element is a no-op) as a list."""
    r, s, out = [], k + 1, []
    for e in aligned:
        if e not in r:
            r.append(e)
        if r[0] is None or (len(r) == s and r[k] is None) or (None not in r and len(r) == s):
            r.pop(0)
        elif None in r and len(r) == s:
            out.append((r[0], r[k]))
            r.pop(0)
    return out


def run_length_walk(cigar, side, k):
    """The same k-mers from the run-length cigar, as csrc/npr_kmer.hip finds them: O(1) per operation."""
    gap = 2 if side == 0 else 1
    total = sum(ln for op, ln in cigar if op != gap)
    live, b, c, pos, out = False, 0, 0, 0, []
    for op, g in cigar:
        if g == 0:
            continue
        if op == gap:
            if live:
                if c != k - 1:
                    continue
                live, b, g = False, k - 1, g - 1
            if g > 0 and b >= 1:
                b0 = min(b, k - 1)
                count = max(0, min(min(total - pos, k - 1) - (k - b0) + 1, b0))
                out += [(pos - b0 + j, pos - b0 + j + k - 1) for j in range(count)]
                live, c = True, 0
        else:
            if live:
                if c + g <= k - 1:
                    c += g
                else:
                    live, b = False, k
            else:
                b = min(b + g, k)
            pos += g
    return out


def indel_kmer_counters(records, k):
    """(read-side Counter, reference-side Counter) over strings: records = (reference window, read window, cigar), sequences folded."""
    rd, rf = Counter(), Counter()
    for ref, read, cigar in records:
        for a, b in literal_walk(columns(cigar, 0), k):
            rd[read[a:b + 1]] += 1
        for a, b in literal_walk(columns(cigar, 1), k):
            rf[ref[a:b + 1]] += 1
    return rd, rf


def window_counter(seqs, k):
    """kmerAnalysis.py:16-17 forward strand only, N-windows included: Counter over strings of the folded sequences."""
    c = Counter()
    for seq in seqs:
        seq = fold(seq)
        for i in range(k, len(seq)):
            c[seq[i - k:i]] += 1
    return c


def table_of(counter, k):
    """A Counter over folded strings as a device table: 4^k + 1 bins, the last one for k-mers with an N."""
    t = np.zeros(4 ** k + 1, dtype=np.int64)
    for s, v in counter.items():
        assert len(s) == k
        t[4 ** k if "N" in s else KA.kmerBin(s)] += v
    return t


def format_table(refKmers, readKmers, k):
    """kmerAnalysis.py:33-46 / indelKmerAnalysis.py:45-57 over Counters keyed by strings."""
    refSize, readSize = sum(refKmers.values()), sum(readKmers.values())
    out = [HEADER]
    for kmer in itertools.product("ATGC", repeat=k):
        kmer = "".join(kmer)
        refFraction, readFraction = 1.0 * refKmers[kmer] / refSize, 1.0 * readKmers[kmer] / readSize
        if refFraction == 0:
            foldChange = "-Inf"
        elif readFraction == 0:
            foldChange = "Inf"
        else:
            foldChange = -log(readFraction / refFraction)
        out.append("\t".join(map(str, [kmer, refKmers[kmer], refFraction, readKmers[kmer], readFraction, foldChange])) + "\n")
    return "".join(out)


def expected_all_bases(refSeqs, readSeqs, k):
    """kmerAnalysis.py:12-30 + :57 on folded sequences: the file's text, or None when it is not written."""
    counters = []
    for seqs in (refSeqs, readSeqs):
        c = Counter()
        for s, v in window_counter(seqs, k).items():
            if "N" not in s:
                c[s] += v
                c[bioio.reverseComplement(s)] += v
        counters.append(c)
    if len(counters[0]) > 0 and len(counters[1]) > 0:
        return format_table(counters[0], counters[1], k)
    return None


def expected_indel_bases(records, k):
    """indelKmerAnalysis.py:29-41 + :68 on folded windows."""
    rd, rf = indel_kmer_counters(records, k)
    refKmers, readKmers = Counter(), Counter()
    for s, v in rd.items():
        readKmers[s] += v
        refKmers[s[::-1]] += v
    for s, v in rf.items():
        refKmers[s] += v
        refKmers[s[::-1]] += v
    if len(refKmers) > 0 and len(readKmers) > 0:
        return format_table(refKmers, readKmers, k)
    return None


def sam_records(samFile, referenceFastaFile):
    """(reference window, read window, M / I / D cigar) of every record with a reference, sequences folded."""
    from nanopore_amd import sam as pysam
    from nanopore_amd.analyses.utils import getFastaDictionary, samIterator
    refs = getFastaDictionary(referenceFastaFile)
    sam = pysam.Samfile(samFile, "r")
    out = []
    for aR in samIterator(sam):
        cigar = [(op, ln) for op, ln in aR.cigar if op in (0, 1, 2)]
        span = sum(ln for op, ln in cigar if op != 1)
        out.append((fold(refs[sam.getrname(aR.rname)][aR.pos:aR.pos + span]), fold(aR.query), cigar))
    sam.close()
    return out


class SliceContext(object):
    """Stands in for realign.Context where no GPU is at hand: the two device tables from Python slices and the literal walk."""

    def kmer_counts(self, seqs, k=5):
        return table_of(window_counter(seqs, k), k)

    def align_indel_kmers(self, refs, reads, cigars, k=5, ref_index=None, start=None):
        records = []
        for i, (read, cigar) in enumerate(zip(reads, cigars)):
            x0, y0 = start[i] if start is not None else (0, 0)
            records.append((fold(refs[ref_index[i] if ref_index is not None else i][x0:]), fold(read[y0:]), cigar))
        rd, rf = indel_kmer_counters(records, k)
        return table_of(rd, k), table_of(rf, k)


def random_cigar(rng, max_ops=12, max_len=9):
    return [(rng.choice([0, 0, 1, 2]), rng.choice([0, 1, 1, 2, 3, rng.randint(0, max_len)])) for _ in range(rng.randint(0, max_ops))]


# ---- tests ----

def test_run_length_walk_equals_the_literal_walk():
    rng = random.Random(1)
    emitted = 0
    for _ in range(20000):
        k = rng.randint(1, 6)
        cigar = random_cigar(rng)
        for side in (0, 1):
            want = literal_walk(columns(cigar, side), k)
            assert sorted(run_length_walk(cigar, side, k)) == sorted(want), (k, cigar, side)
            assert all(b - a == k - 1 for a, b in want)     # k consecutive bases
            emitted += len(want)
    assert emitted > 20000


def test_what_the_walk_does_with_gaps():
    k = 5
    # a gap emits at most k - 1 k-mers, each with a base on either side of the gap point
    assert literal_walk(columns([(0, 20), (2, 3), (0, 20)], 0), k) == [(16, 20), (17, 21), (18, 22), (19, 23)]
    # a second gap that opens while the first one's None is in the window is swallowed
    assert literal_walk(columns([(0, 20), (2, 1), (0, 2), (2, 7), (0, 20)], 0), k) == [(16, 20), (17, 21), (18, 22), (19, 23)]
    # a gap before the first or after the last position of its side emits nothing
    assert literal_walk(columns([(2, 4), (0, 20), (2, 4)], 0), k) == []
    # an I followed by a D: the read side's gap has the insertion's bases before it
    assert literal_walk(columns([(1, 3), (2, 2), (0, 10)], 0), k) == [(0, 4), (1, 5), (2, 6)]
    assert literal_walk(columns([(0, 9), (2, 1), (0, 9)], 0), 1) == []


def test_bin_permutations_against_strings():
    for k in (1, 2, 5):
        rev, rc = KA.reversedBins(k), KA.reverseComplementBins(k)
        for b, kmer in enumerate(itertools.product("ACGT", repeat=k)):
            kmer = "".join(kmer)
            assert KA.kmerBin(kmer) == b
            assert rev[b] == KA.kmerBin(kmer[::-1]) and rc[b] == KA.kmerBin(bioio.reverseComplement(kmer))


def test_composition_of_hand_made_tables():
    k = 2
    fwd = table_of(Counter({"AC": 3, "GT": 1, "TT": 2, "AN": 5}), k)
    both = KA.bothStrands(fwd, k)
    want = Counter({"AC": 3 + 1, "GT": 1 + 3, "TT": 2, "AA": 2})         # GT is AC's reverse complement, AA is TT's
    assert {"".join(m): int(both[KA.kmerBin("".join(m))]) for m in itertools.product("ACGT", repeat=k) if both[KA.kmerBin("".join(m))]} == dict(want)
    R = table_of(Counter({"AC": 2, "NA": 1}), k)
    X = table_of(Counter({"AC": 1, "GG": 4, "CN": 2}), k)
    refKmers, readKmers, refSize, readSize = IK.composeIndelCounters(R, X, k)
    want_ref = Counter({"AC": 1, "CA": 1 + 2, "GG": 8})                  # the read side's reversed k-mers land in refKmers
    assert {m: int(refKmers[KA.kmerBin(m)]) for m in ("AC", "CA", "GG", "TT")} == {"AC": 1, "CA": 3, "GG": 8, "TT": 0} and refKmers.sum() == sum(want_ref.values())
    assert int(readKmers[KA.kmerBin("AC")]) == 2 and readKmers.sum() == 2
    assert readSize == 3 and refSize == 2 * 7 + 3                        # k-mers with an N count in the sizes


def test_table_text_rows_fractions_and_inf(tmp_path):
    k = 2
    ref = Counter({"AC": 3, "GG": 1})
    read = Counter({"AC": 1, "TT": 3})
    path = str(tmp_path / "t.txt")
    KA.writeCounts(path, table_of(ref, k), table_of(read, k), 4, 4, k)
    text = open(path).read()
    assert text == format_table(ref, read, k)
    lines = text.splitlines()
    assert lines[0] == HEADER.rstrip("\n") and [ln.split("\t")[0] for ln in lines[1:]] == ["".join(m) for m in itertools.product("ATGC", repeat=k)]
    rows = {ln.split("\t")[0]: ln.split("\t")[1:] for ln in lines[1:]}
    assert rows["AC"] == ["3", "0.75", "1", "0.25", str(-log(0.25 / 0.75))]
    assert rows["GG"][-1] == "Inf" and rows["TT"][-1] == "-Inf" and rows["AA"] == ["0", "0.0", "0", "0.0", "-Inf"]


def _write_inputs(tmp_path, refs, reads, sam_lines):
    fa, fq, samp = tmp_path / "ref.fa", tmp_path / "reads.fq", tmp_path / "m.sam"
    with open(str(fa), "w") as fh:
        for name, seq in refs:
            fh.write(">%s\n%s\n" % (name, seq))
    fq.write_text("".join("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)) for n, s in reads))
    samp.write_text("".join("@SQ\tSN:%s\tLN:%d\n" % (n, len(s)) for n, s in refs) + "".join("\t".join(ln) + "\n" for ln in sam_lines))
    return str(fa), str(fq), str(samp)


def test_analyses_write_the_reference_tables(tmp_path):
    ref = "ACGTTGCANNACGGTCATGCATGCCGTAAGCTTAGC" * 3
    read = "GTTGCAACGGTCATCATGCCGTTTAAGC"
    fa, fq, samp = _write_inputs(tmp_path, [("ref1", ref)], [("r1", read), ("r2", "ACGTNNACGTAC")],
                                 [["r1", "0", "ref1", "3", "60", "2S6M2D8M3I9M", "*", "0", "0", "AA" + read[:26], "*"],
                                  ["r2", "4", "*", "0", "0", "*", "*", "0", "0", "ACGTNNACGTAC", "*"]])
    for k in (3, 5):
        out = tmp_path / ("out%d" % k)
        out.mkdir()
        KA.KmerAnalysis(fq, "2D", fa, samp, str(out)).run(kmerSize=k, ctx=SliceContext())
        assert (out / "all_bases_kmer_counts.txt").read_text() == expected_all_bases([ref], [read, "ACGTNNACGTAC"], k)
        assert (out / "DONE").exists()
        out2 = tmp_path / ("indel%d" % k)
        out2.mkdir()
        IK.IndelKmerAnalysis(fq, "2D", fa, samp, str(out2)).run(kmerSize=k, ctx=SliceContext())
        want = expected_indel_bases(sam_records(samp, fa), k)
        assert want is not None and want.count("\n") == 4 ** k + 1
        assert (out2 / "indel_bases_kmer_counts.txt").read_text() == want and (out2 / "DONE").exists()


def test_files_are_written_only_under_the_reference_conditions(tmp_path):
    # reads too short for a window (kmerAnalysis.py:57: readKmers is empty); a record without gaps (indelKmerAnalysis.py:68)
    fa, fq, samp = _write_inputs(tmp_path, [("ref1", "ACGTACGTACGTACGT")], [("r1", "ACGTA")],
                                 [["r1", "0", "ref1", "1", "60", "5M", "*", "0", "0", "ACGTA", "*"]])
    out = tmp_path / "out"
    out.mkdir()
    KA.KmerAnalysis(fq, "2D", fa, samp, str(out)).run(ctx=SliceContext())
    IK.IndelKmerAnalysis(fq, "2D", fa, samp, str(out)).run(ctx=SliceContext())
    assert sorted(os.listdir(str(out))) == ["DONE"]
    assert expected_all_bases(["ACGTACGTACGTACGT"], ["ACGTA"], 5) is None and expected_indel_bases(sam_records(samp, fa), 5) is None
    # only N windows on one side: nothing either
    fa, fq, samp = _write_inputs(tmp_path, [("ref1", "NNNNNNNNNNNN")], [("r1", "ACGTACGTAC")], [])
    KA.KmerAnalysis(fq, "2D", fa, samp, str(out)).run(ctx=SliceContext())
    assert sorted(os.listdir(str(out))) == ["DONE"]


def test_library_holds_the_kmer_kernels_and_entry_points():
    """The gfx950 build of the library has npr_kmer.hip in it: its kernels are registered and the C ABI exports the three calls."""
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("npr_kmer_counts", "npr_align_indel_kmers", "npr_batch_indel_kmers"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"k_kmer_spectrum" in blob and b"k_indel_kmers" in blob
    with open(os.path.join(ROOT, "nanopore_amd", "csrc", "Makefile")) as fh:
        assert "npr_kmer.hip" in fh.read()
    # arguments are checked before any device is touched
    L = _lib.load()
    one = np.zeros(4 ** 6 + 1, dtype=np.int64)
    for k in (0, 7):
        assert L.npr_kmer_counts(None, k, 0, None, None, _lib.ptr(one)) == _lib.ERR_INVALID
        assert L.npr_batch_indel_kmers(None, k, _lib.ptr(one), _lib.ptr(one)) == _lib.ERR_INVALID

"""KmerAnalysis: all_bases_kmer_counts.txt.

Schema of nanopore/analyses/kmerAnalysis.py: every window `seq[i - k : i]`, `i` in `k .. len(seq) - 1`, of every reference
and every read sequence that holds no N is counted together with its reverse complement (:15-28), and the two counters
are written side by side with their fractions and `-log(readFraction / refFraction)` per k-mer (:32-46).  The windows
are counted on the device (`npr_kmer_counts`, include/nprealign.h: one forward-strand table of 4^k + 1 bins per set of
sequences); the reverse complement is a permutation of the bins and is added here.  No CPU fallback.

Differences from the reference: the library folds letter case and maps every letter outside ACGT to N, where the
reference keys lower-case and IUPAC windows as strings of their own (which its table, written over `"ATGC"` products,
never lists, but which count in `refSize` / `readSize`); for upper-case ACGTN input the files are identical.  The table
has one row per k-mer of `kmerSize` bases (the reference hard-codes 5 in its row loop).  The `Rscript` step is left out,
as the other analyses here leave their plots out.
"""
import itertools
import os
from math import log

import numpy as np

from ..bioio import fastaRead, fastqRead
from .abstractAnalysis import AbstractAnalysis

HEADER = "kmer\trefCount\trefFraction\treadCount\treadFraction\tlogFoldChange\n"
_CODE = {"A": 0, "C": 1, "G": 2, "T": 3}


def kmerBin(kmer):
    """Bin of an ACGT k-mer in a device table: its base-4 number, first base most significant."""
    b = 0
    for ch in kmer:
        b = 4 * b + _CODE[ch]
    return b


def _digits(k):
    """[4^k, k] base-4 digits of every bin, first base first."""
    bins = np.arange(4 ** k, dtype=np.int64)
    return np.stack([(bins >> (2 * (k - 1 - j))) & 3 for j in range(k)], axis=1)


def _number(digits):
    k = digits.shape[1]
    return sum(digits[:, j] << (2 * (k - 1 - j)) for j in range(k))


def reversedBins(k):
    """perm[b] = bin of the k-mer of bin b read backwards."""
    return _number(_digits(k)[:, ::-1])


def reverseComplementBins(k):
    """perm[b] = bin of the reverse complement of the k-mer of bin b (A <-> T, C <-> G: digit d -> 3 - d)."""
    return _number(3 - _digits(k)[:, ::-1])


def writeCounts(path, refCounts, readCounts, refSize, readSize, kmerSize, rows=True):
    """The reference's table (kmerAnalysis.py:34-47, indelKmerAnalysis.py:46-58): refCounts / readCounts are tables over the
    4^k ACGT bins; one row per k-mer in itertools.product("ATGC") order."""
    with open(path, "w") as outf:
        outf.write(HEADER)
        if not rows:
            return
        for kmer in itertools.product("ATGC", repeat=kmerSize):
            kmer = "".join(kmer)
            b = kmerBin(kmer)
            refCount, readCount = int(refCounts[b]), int(readCounts[b])
            refFraction, readFraction = 1.0 * refCount / refSize, 1.0 * readCount / readSize
            if refFraction == 0:
                foldChange = "-Inf"
            elif readFraction == 0:
                foldChange = "Inf"
            else:
                foldChange = -log(readFraction / refFraction)
            outf.write("\t".join(map(str, [kmer, refCount, refFraction, readCount, readFraction, foldChange])) + "\n")


def bothStrands(forward, k):
    """The reference's counter from a forward-strand device table: every N-free window and its reverse complement."""
    f = np.asarray(forward[:4 ** k], dtype=np.int64)
    return f + f[reverseComplementBins(k)]


class KmerAnalysis(AbstractAnalysis):
    """Runs kmer analysis"""

    def countKmers(self, ctx=None):
        from .utils import _context
        ctx = ctx or _context()
        k = self.kmerSize
        refKmers = bothStrands(ctx.kmer_counts([seq for _, seq in fastaRead(self.referenceFastaFile)], k), k)
        readKmers = bothStrands(ctx.kmer_counts([seq for _, seq, _ in fastqRead(self.readFastqFile)], k), k)
        return refKmers, readKmers

    def analyzeCounts(self, refKmers, readKmers, name):
        writeCounts(os.path.join(self.outputDir, name + "kmer_counts.txt"), refKmers, readKmers, int(refKmers.sum()), int(readKmers.sum()),
                    self.kmerSize)

    def run(self, kmerSize=5, ctx=None):
        AbstractAnalysis.run(self)
        self.kmerSize = kmerSize
        refKmers, readKmers = self.countKmers(ctx=ctx)
        if refKmers.sum() > 0 and readKmers.sum() > 0:  # (the reference: both counters hold a k-mer, kmerAnalysis.py:57)
            self.analyzeCounts(refKmers, readKmers, "all_bases_")
        self.finish()

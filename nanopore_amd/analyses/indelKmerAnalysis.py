"""IndelKmerAnalysis: indel_bases_kmer_counts.txt.

Schema of nanopore/analyses/indelKmerAnalysis.py: for every SAM record the k-mers of the read that straddle a deletion
and the k-mers of the reference that straddle an insertion are found by walking the record's aligned pairs through an
ordered set (:11-19, :29-40), counted, and written like KmerAnalysis' table (:44-58).  The walk is done on the device
(`npr_align_indel_kmers`, include/nprealign.h: one wavefront per record over its run-length cigar; a read-side and a
reference-side table of 4^k + 1 bins); the counters are composed from the two tables here.  No CPU fallback.

Differences from the reference: letter case is folded and every letter outside ACGT is N, as in kmerAnalysis; positions
count from the first aligned base of the read, where the reference indexes `record.query` with positions that count from
the start of SEQ -- the same for records without soft clips (every chained or realigned record).  `refSize` / `readSize`
include the k-mers with a non-ACGT base, as the reference's counters hold them (its table does not list them).
"""
import os

import numpy as np

from .. import sam as pysam
from .abstractAnalysis import AbstractAnalysis
from .kmerAnalysis import reversedBins, writeCounts
from .utils import getFastaDictionary, samIterator


def composeIndelCounters(readSide, refSide, k):
    """(refKmers, readKmers, refSize, readSize) of indelKmerAnalysis.py:33-40 from the device tables (4^k + 1 bins, the last one for
    k-mers with a base outside ACGT): the tables over the ACGT bins and the sums over all k-mers."""
    readSide, refSide = np.asarray(readSide, dtype=np.int64), np.asarray(refSide, dtype=np.int64)
    n, rev = 4 ** k, reversedBins(k)
    R, X = readSide[:n], refSide[:n]
    # the reference adds the read side's reversed k-mers to refKmers, not to readKmers (indelKmerAnalysis.py:36): kept as it is
    refKmers = X + X[rev] + R[rev]
    return refKmers, R.copy(), int(2 * refSide.sum() + readSide.sum()), int(readSide.sum())


class IndelKmerAnalysis(AbstractAnalysis):
    """Runs kmer analysis"""

    def countIndelKmers(self, ctx=None):
        """The device tables (read side, reference side) over the records of self.samFile that have a reference."""
        from .utils import _context
        refSequences = getFastaDictionary(self.referenceFastaFile)
        sam = pysam.Samfile(self.samFile, "r")
        records = list(samIterator(sam))
        for aR in records:
            assert all(op in (0, 1, 2, 4, 5) for op, _ in aR.cigar), "unsupported cigar operation in %s" % aR.qname
        names = sorted(refSequences)
        index = {n: i for i, n in enumerate(names)}
        refIndex = [index[sam.getrname(aR.rname)] for aR in records]
        sam.close()
        if not records:
            nb = 4 ** self.kmerSize + 1
            return np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
        ctx = ctx or _context()
        return ctx.align_indel_kmers([refSequences[n] for n in names], [aR.query for aR in records],
                                     [[(op, ln) for op, ln in aR.cigar if op in (0, 1, 2)] for aR in records], k=self.kmerSize,
                                     ref_index=refIndex, start=[(int(aR.pos), 0) for aR in records])

    def analyzeCounts(self, refKmers, readKmers, refSize, readSize, name):
        writeCounts(os.path.join(self.outputDir, name + "kmer_counts.txt"), refKmers, readKmers, refSize, readSize, self.kmerSize,
                    rows=refSize > 0 and readSize > 0)

    def run(self, kmerSize=5, ctx=None):
        AbstractAnalysis.run(self)
        self.kmerSize = kmerSize
        readSide, refSide = self.countIndelKmers(ctx=ctx)
        refKmers, readKmers, refSize, readSize = composeIndelCounters(readSide, refSide, kmerSize)
        if refSize > 0 and readSize > 0:  # (the reference: both counters hold a k-mer, indelKmerAnalysis.py:68)
            self.analyzeCounts(refKmers, readKmers, refSize, readSize, "indel_bases_")
        self.finish()

"""UnmappedKmerAnalysis: <readType>_kmer_counts.txt, the k-mers of the reads some mapper placed against those of the reads
no mapper placed.

Schema of nanopore/metaAnalyses/unmappedKmerAnalysis.py: per read type every window `seq[i - k : i]`, `i` in
`k .. len(seq) - 1`, without an N, of the mapped and of the unmapped reads, forward strand only (:12-27), written side by
side with their fractions and `-log(mappedFraction / unmappedFraction)` (:29-48).  The reference slices every window of
every read in Python and adds one Counter per read; here one device pass per FASTQ file counts the reads where they lie in
the mapped file into one table per (read type, mapped / unmapped) (`npr_kmer_counts_groups`, include/nprealign.h;
csrc/npr_kmer.hip: k_kmer_spectrum_groups), and the tables of the files are summed in int64.  No CPU fallback.

Differences from the reference: letter case is folded and every letter outside ACGT is an N, as in analyses/kmerAnalysis.py
here (the reference keys lower-case and IUPAC windows as strings of their own, which its table never lists but which count
in the sizes); for upper-case ACGTN reads the files are identical.  The table has one row per k-mer of `kmerSize` bases
(the reference hard-codes 5 in its row loop) and is written into outputDir; rows and reads come in a defined order
(abstractUnmappedAnalysis.py); the `Rscript` step is left out.
"""
import itertools
import os
from math import log

import numpy as np

from ..analyses.kmerAnalysis import kmerBin
from .abstractUnmappedAnalysis import AbstractUnmappedMetaAnalysis

HEADER = "kmer\tmappableCount\tmappableFraction\tunmappableCount\tunmappableFraction\tlogFoldChange\n"


def writeUnmappedCounts(path, mappedCounts, unmappedCounts, kmerSize):
    """The reference's table (unmappedKmerAnalysis.py:29-48) from two tables over the 4^k ACGT bins (a device table's last
    bin, the windows with an N, is not looked at)."""
    mappedCounts, unmappedCounts = np.asarray(mappedCounts)[:4 ** kmerSize], np.asarray(unmappedCounts)[:4 ** kmerSize]
    mappedSize, unmappedSize = int(mappedCounts.sum()), int(unmappedCounts.sum())
    with open(path, "w") as outf:
        outf.write(HEADER)
        for kmer in itertools.product("ATGC", repeat=kmerSize):
            kmer = "".join(kmer)
            b = kmerBin(kmer)
            mapped, unmapped = int(mappedCounts[b]), int(unmappedCounts[b])
            mappedFraction = 1.0 * mapped / mappedSize if mappedSize > 0 else 0
            unmappedFraction = 1.0 * unmapped / unmappedSize if unmappedSize > 0 else 0
            if unmappedFraction == 0:
                foldChange = "-Inf"
            elif mappedFraction == 0:
                foldChange = "Inf"
            else:
                foldChange = -log(mappedFraction / unmappedFraction)
            outf.write("\t".join(map(str, [kmer, mapped, mappedFraction, unmapped, unmappedFraction, foldChange])) + "\n")


class UnmappedKmerAnalysis(AbstractUnmappedMetaAnalysis):
    """Calculates kmer statistics for all reads (in all samples) not mapped by any mapper"""

    def countKmers(self, ctx=None):
        """int64 [2 * read types, 4^k + 1]: rows 2 t (mapped) and 2 t + 1 (unmapped) for the t-th of the sorted read types."""
        from ..analyses.utils import _context
        ctx = ctx or _context()
        types = sorted(self.readTypes)
        tables = np.zeros((2 * len(types), 4 ** self.kmerSize + 1), dtype=np.int64)
        for rf in self.readFiles:
            group = (2 * types.index(rf.readType) + 1 - rf.is_mapped.astype(np.int32)).astype(np.int32)
            tables += ctx.kmer_counts_groups(rf.table.text, rf.table.seq_span[:, 0], rf.table.seq_span[:, 1], group, 2 * len(types), self.kmerSize)
        return tables

    def run(self, kmerSize=5, ctx=None):
        self.kmerSize = kmerSize
        tables = self.countKmers(ctx=ctx)
        for t, readType in enumerate(sorted(self.readTypes)):
            writeUnmappedCounts(os.path.join(self.outputDir, readType + "_kmer_counts.txt"), tables[2 * t], tables[2 * t + 1], kmerSize)

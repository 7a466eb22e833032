"""UnmappedLengthDistributionAnalysis: the read lengths of the mapped and of the unmapped reads, one per line.

Schema of nanopore/metaAnalyses/unmappedLengthDistributionAnalysis.py:9-29: <readType>_mapped.txt / _unmapped.txt per read
type and <basename(reference)>_mapped.txt / _unmapped.txt per reference FASTA file.  The lengths come from the span arrays
of the read database (abstractUnmappedAnalysis.py), not from a Python object per read.

The reference's per-reference files do not filter by reference (:24-28): each holds every read of every FASTQ file, split
by whether ANY mapper placed it on ANY reference.  That is kept.  Differences: the lines come in the defined order of the
read database; the `Rscript` plots are left out.
"""
import os

import numpy as np

from .abstractUnmappedAnalysis import AbstractUnmappedMetaAnalysis


def _writeLengths(path, lengths):
    with open(path, "w") as f:
        f.write("".join("%d\n" % n for n in lengths.tolist()))


class UnmappedLengthDistributionAnalysis(AbstractUnmappedMetaAnalysis):
    """runs length distribution analysis on all mapped/unmapped per read Type as well as per reference"""

    def _lengths(self, readFiles, mapped):
        parts = [rf.table.lengths[rf.is_mapped == mapped] for rf in readFiles]
        return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)

    def run(self):
        for readType in sorted(self.readTypes):
            mine = [rf for rf in self.readFiles if rf.readType == readType]
            _writeLengths(os.path.join(self.outputDir, readType + "_unmapped.txt"), self._lengths(mine, 0))
            _writeLengths(os.path.join(self.outputDir, readType + "_mapped.txt"), self._lengths(mine, 1))
        for reference in sorted(self.referenceFastaFiles):
            _writeLengths(os.path.join(self.outputDir, os.path.basename(reference) + "_unmapped.txt"), self._lengths(self.readFiles, 0))
            _writeLengths(os.path.join(self.outputDir, os.path.basename(reference) + "_mapped.txt"), self._lengths(self.readFiles, 1))

"""CoverageDepth: <experiment>_Depth.txt and <experiment>_Stats.out per experiment.

Schema of nanopore/metaAnalyses/coverageDepth.py:35-98.  The reference converts resultsDir/mapping.sam to BAM, sorts and
indexes it and runs `samtools depth` (:49-65); here the depth comes from the device pileup of mapping.sam
(analyses/pileup.py, csrc/npr_pileup.hip): no bam, no sort, no index, the same text.  _Stats.out (:74-92): a header with the
mean and the population standard deviation (numpy.std) of the depth lines, then every depth line whose depth exceeds the
previous LINE's depth by at least two standard deviations (the first line compares against 0), with the five reference
bases that end at the position (the first `pos` bases when pos < 5).  Floats are written as Python 2 wrote str(float)
(hmm.py: 12 significant digits).  The R plots are not made.  No CPU fallback.

Two deliberate differences: the reference takes the k-mer from the LAST sequence of the FASTA whatever contig the line
names -- here it comes from the line's own contig (the same thing for one contig); and the reference skips an experiment
that already has resultsDir/mapping.sorted -- there is no such file here, so an experiment whose _Depth.txt exists is
skipped.
"""
import os

import numpy as np

from ..analyses.pileup import depth_text, pileup_of_sam
from ..analyses.utils import getFastaDictionary
from ..hmm import _fmt
from .abstractMetaAnalysis import AbstractMetaAnalysis


def coverageStats(depthText, sequences):
    """The text of _Stats.out from the text of _Depth.txt and {name: sequence} (coverageDepth.py:74-92)."""
    lines = [ln.split("\t") for ln in depthText.split("\n") if ln]
    cov = np.array([int(f[2]) for f in lines], dtype=np.int64)
    mean, sd = (float(np.mean(cov)), float(np.std(cov))) if len(cov) else (float("nan"), float("nan"))
    out = ["Position\tCoverage (mu=" + _fmt(mean) + "X, sd=" + _fmt(sd) + "X)\tKmer\n"]
    previous = 0
    for (name, pos, _), c in zip(lines, cov.tolist()):
        pos = int(pos)
        if c - previous >= 2 * sd:
            seq = sequences[name].upper()
            out.append("%d\t%d\t%s\n" % (pos, c, seq[pos - 5:pos] if pos >= 5 else seq[0:pos]))
        previous = c
    return "".join(out)


class CoverageDepth(AbstractMetaAnalysis):
    """Coverage depth per base across the reference, from the device pileup"""

    def run(self, ctx=None):
        from ..analyses.utils import _context
        for readFastqFile, readType, referenceFastaFile, mapper, analyses, resultsDir in self.experiments:
            experiment = resultsDir.rstrip("/").split("/")[-1]
            samFile = os.path.join(resultsDir, "mapping.sam")
            depthFile = os.path.join(self.outputDir, experiment + "_Depth.txt")
            if os.path.isfile(depthFile) or not os.path.isfile(samFile):
                continue
            ctx = ctx or _context()
            names, lengths, pileup = pileup_of_sam(ctx, samFile, referenceFastaFile)
            try:
                depth, covered = pileup.depth()
            finally:
                pileup.close()
            text = depth_text(names, lengths, depth, covered)
            stats = coverageStats(text, getFastaDictionary(referenceFastaFile))
            with open(os.path.join(self.outputDir, experiment + "_Stats.out"), "w") as f:
                f.write(stats)
            with open(depthFile, "w") as f:  # written last: its presence marks the experiment as done
                f.write(text)

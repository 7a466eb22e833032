"""Consensus: where the sample differs from the reference, and what its sequence looks like (nanopore/analyses/consensus.py:50-62 names
the two files and the layout of the FASTQ).

The reference pipes `samtools mpileup | bcftools view -cg | vcfutils.pl vcf2fq`.  None of the three exists here and bcftools' genotype
model is NOT restated: the calls are those of the marginAlign SNP caller's own posterior (include/nprealign.h: npr_snp_variants_table) over
the frequencies of aligned bases, made on the device (csrc/npr_snpcall.hip) from a pileup of all records of the SAM file
(Pileup.snp_variants).  Evolution is NULL_MATRIX; the error matrix is that of the experiment's `hmm.txt` when the mapper trained one,
else of blasr_hmm_20.txt, the model MarginAlignSnpCaller takes.

  <reads>_<reference>_Consensus.fastq   one four-line record per reference sequence, in the order of the reference file: `@name`, the
                                        best base per position (ACGT; N where no call is possible), `+`, chr(33 + quality), upper case
                                        and unwrapped -- the form formatConsensusFastq leaves
  <reads>_<reference>_Consensus.vcf     ##fileformat=VCFv4.1, one ##contig per reference sequence, ##INFO for PP; then one line per
                                        candidate base other than the reference's whose posterior reaches `threshold`, in ascending
                                        (sequence, position, base): CHROM POS(1-based) . REF ALT QUAL . PP=<posterior>, QUAL = min(93,
                                        floor(-10 log10(1 - p))), 93 at p = 1
"""
import math
import os

import numpy as np

from .. import sam as pysam
from .abstractAnalysis import AbstractAnalysis
from .marginAlignSnpCaller import NULL_MATRIX, errorMatrixOfHmm
from .utils import getFastaDictionary, samIterator, stageRecordsForPileup, trainedModelPath

_BASES = np.frombuffer(b"ACGTN", dtype=np.uint8)
_PHRED = np.arange(33, 33 + 256, dtype=np.int64).clip(0, 255).astype(np.uint8)
MAX_QUAL = 93


def consensusFastq(names, refLengths, best, qual):
    """The FASTQ text of the per-row best bases (codes 0..4) and qualities (0..93): rows in the order of the sequences."""
    bases, quals = _BASES[np.asarray(best, dtype=np.uint8)].tobytes().decode("ascii"), _PHRED[np.asarray(qual, dtype=np.uint8)].tobytes().decode("ascii")
    out, row = [], 0
    for name, length in zip(names, refLengths):
        out.append("@%s\n%s\n+\n%s\n" % (name, bases[row:row + length], quals[row:row + length]))
        row += length
    return "".join(out)


def callQuality(p):
    """QUAL of a call made with posterior p."""
    return MAX_QUAL if p >= 1.0 else min(MAX_QUAL, int(math.floor(-10.0 * math.log10(1.0 - p))))


def consensusVcf(names, refLengths, refCodes, callRow, callAlt, callP):
    """The VCF text of the calls, in array order."""
    out = ["##fileformat=VCFv4.1\n"]
    out += ["##contig=<ID=%s,length=%d>\n" % (name, length) for name, length in zip(names, refLengths)]
    out.append('##INFO=<ID=PP,Number=1,Type=Float,Description="Posterior probability of the alternative base">\n')
    out.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\n")
    firstRow = np.concatenate([[0], np.cumsum(refLengths)]).astype(np.int64)
    callRow = np.asarray(callRow, dtype=np.int64)
    which = np.searchsorted(firstRow, callRow, side="right") - 1
    for k, row, alt, p in zip(which.tolist(), callRow.tolist(), np.asarray(callAlt).tolist(), np.asarray(callP, dtype=np.float64).tolist()):
        out.append("%s\t%d\t.\t%s\t%s\t%d\t.\tPP=%.6f\n" % (names[k], row - firstRow[k] + 1, "ACGTN"[refCodes[row]], "ACGT"[alt], callQuality(p), p))
    return "".join(out)


class Consensus(AbstractAnalysis):
    """Variant calls and a consensus sequence from the SNP caller's posteriors"""
    threshold = 0.5

    def errorMatrix(self):
        hmmFile = os.path.join(os.path.split(self.samFile)[0], "hmm.txt")
        return errorMatrixOfHmm(hmmFile if os.path.exists(hmmFile) else trainedModelPath("blasr_hmm_20.txt"))

    def run(self, ctx=None):
        AbstractAnalysis.run(self)
        from .utils import _context
        ctx = ctx or _context()
        refSequences = getFastaDictionary(self.referenceFastaFile)
        refNames = list(refSequences)
        sam = pysam.Samfile(self.samFile, "r")
        records = list(samIterator(sam))
        for aR in records:
            assert all(op in (0, 1, 2, 4, 5) for op, _ in aR.cigar), "%s has cigar operations other than M / I / D / S / H" % aR.qname
        staged = stageRecordsForPileup(sam, records, refSequences, refNames)
        sam.close()
        pileup = ctx.pileup(staged["refLengths"])
        try:
            pileup.add_csr(staged["read"], staged["readOff"], None, staged["ops"], staged["opsOff"], staged["refIndex"], staged["start"])
            best, qual, callRow, callAlt, callP = pileup.snp_variants(staged["refCodes"], NULL_MATRIX, self.errorMatrix(), self.threshold)
        finally:
            pileup.close()
        # <reads>_<reference>: each path up to its first ".fastq" / ".fa", without its directories
        header = "%s_%s" % (os.path.basename(self.readFastqFile.split(".fastq")[0]), os.path.basename(self.referenceFastaFile.split(".fa")[0]))
        with open(os.path.join(self.outputDir, header + "_Consensus.vcf"), "w") as fh:
            fh.write(consensusVcf(refNames, staged["refLengths"], staged["refCodes"], callRow, callAlt, callP))
        with open(os.path.join(self.outputDir, header + "_Consensus.fastq"), "w") as fh:
            fh.write(consensusFastq(refNames, staged["refLengths"], best, qual))
        self.finish()
        return best, qual, callRow, callAlt, callP

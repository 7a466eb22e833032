"""SeedMapper: the build's own base mapper.  The reference's base mappers (last, bwa, lastz, blasr) are external binaries and out of
scope here (abstractMapper.py); this one needs nothing but the device: every maximal exact match of at least `minLength` bases between a
read (either strand) and a reference sequence becomes one local-hit SAM record, found by the seed index of csrc/npr_seed.hip
(include/nprealign.h, "exact-match seeding").  The records are what chainSamFile and realignSamFile expect of a base mapper: POS, a
CIGAR of one M run between hard clips, FLAG 16 and reverse-complemented bases for the reverse strand.  No gapped extension: that is the
realigner's part.

The chain step of a SeedMapper does not read those records back: run() keeps the tables and the hit arrays, and chainSamFile() /
realignSamFile() make the chained SAM from them -- the chains and their guide alignments on the device (Context.seed_chains,
csrc/npr_seedchain.hip), the records by the threaded host formatter (realign.seed_chain_sam_text) -- byte for byte the file
utils.chainSamFile writes from the records.  SAM files of external mappers keep going through utils.chainSamFile.
"""
import os

import numpy as np

from .abstractMapper import AbstractMapper


class SeedMapper(AbstractMapper):
    k = 16             # index window: positions whose next k bases are all A C G T are indexed
    minLength = 20     # shortest match reported (>= k)
    bothStrands = True
    maxGap = 200       # chainFn's maxGap: the largest summed gap between two blocks of a chain
    _seeds = None      # what run() found: (FastaTable, FastqTable, begin, end, hit_off, hits)

    def run(self):
        """Reference FASTA + read FASTQ -> self.outputSamFile: an @SQ line per reference sequence in FASTA order (names cut at the
        first blank), then the records in FASTQ order, a read's sorted by (strand, reference, reference position, read position).  A
        read without a match gets no record."""
        from .. import ingest, realign
        from ..analyses.utils import _context
        ctx = _context()  # raises NprError NPR_ERR_NO_DEVICE without a GPU: there is no host fallback
        fa = ingest.FastaTable(self.referenceFastaFile)
        fq = ingest.FastqTable(self.readFastqFile)
        begin, end = np.ascontiguousarray(fq.seq_span[:, 0]), np.ascontiguousarray(fq.seq_span[:, 1])
        index = ctx.seed_index_csr(fa.seq, fa.off, self.k)
        try:
            hit_off, hits = index.matches(fq.text, begin, end, self.minLength, 3 if self.bothStrands else 1)
        finally:
            index.close()
        self._seeds = (fa, fq, begin, end, hit_off, hits)
        records, _ = realign.seed_sam_text(fq.text, fq.name_span, begin, end, [name.encode() for name in fa.names], hit_off, hits)
        with open(self.outputSamFile, "wb") as fh:
            for name, length in zip(fa.names, np.diff(fa.off)):
                fh.write(("@SQ\tSN:%s\tLN:%d\n" % (name, length)).encode())
            fh.write(records.tobytes())

    def _writeChainedSam(self, path):
        """The chained SAM of the hits run() kept: the header run() wrote, then one global alignment per (read, reference), in the order
        utils.chainSamFile writes them."""
        from .. import realign
        from ..analyses.utils import _context
        fa, fq, begin, end, hit_off, hits = self._seeds
        chain_off, chains, ops_off, ops = _context().seed_chains(fq.lengths, np.diff(fa.off), hit_off, hits, self.maxGap)
        records, _ = realign.seed_chain_sam_text(fq.text, fq.name_span, begin, end, [name.encode() for name in fa.names], chain_off, chains, ops_off, ops)
        with open(path, "wb") as fh:
            for name, length in zip(fa.names, np.diff(fa.off)):
                fh.write(("@SQ\tSN:%s\tLN:%d\n" % (name, length)).encode())
            fh.write(records.tobytes())

    def chainSamFile(self):
        """AbstractMapper.chainSamFile from the arrays of run() instead of its records (without a run(): the inherited path)."""
        if self._seeds is None:
            return AbstractMapper.chainSamFile(self)
        self._writeChainedSam(self.outputSamFile)

    def realignSamFile(self, gapGamma=0.5, matchGamma=0.0, doEm=False, useTrainedModel=False, trainedModelFile="blasr_hmm_0.txt"):
        """AbstractMapper.realignSamFile with the chained SAM made from the arrays of run(); what follows the chaining is what
        utils.realignSamFileTargetFn does after its own (without a run(): the inherited path)."""
        from ..analyses import utils
        if self._seeds is None:
            return AbstractMapper.realignSamFile(self, gapGamma, matchGamma, doEm, useTrainedModel, trainedModelFile)
        hmmFile = self.selectHmmFile(doEm, useTrainedModel, trainedModelFile)
        tempSamFile = os.path.join(self.getGlobalTempDir(), "temp.sam")
        self._writeChainedSam(tempSamFile)
        if hmmFile is not None and doEm:
            utils.learnModelFromSamFileTargetFn(self, tempSamFile, self.readFastqFile, self.referenceFastaFile, hmmFile)
        else:
            assert not doEm
        return utils.realignSamFile(tempSamFile, self.outputSamFile, self.readFastqFile, self.referenceFastaFile, hmmFile, gapGamma, matchGamma)

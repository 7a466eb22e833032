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

`fused` (off by default; the files are the same byte for byte either way): run() makes the rows, the chains and their guides in one
call with the rows never leaving the device (SeedIndex.map, csrc/npr_seedmap.hip), chainSamFile() formats those chains, and
realignSamFile() hands them to the job pipeline as arrays (job.SeedSource): no temp.sam is written and parsed back for the realign step.
"""
import os

import numpy as np

from .abstractMapper import AbstractMapper


class SeedMapper(AbstractMapper):
    k = 16             # index window: positions whose next k bases are all A C G T are indexed
    minLength = 20     # shortest match reported (>= k)
    bothStrands = True
    maxGap = 200       # chainFn's maxGap: the largest summed gap between two blocks of a chain
    fused = False      # True: rows, chains and guides in one device-resident call, and the guides to the realigner as arrays (see above)
    _seeds = None      # what run() found: (FastaTable, FastqTable, begin, end, hit_off, hits)
    _chains = None     # ... and with `fused` the chains of those rows: (chain_off, chains, ops_off, ops)

    def run(self):
        """Reference FASTA + read FASTQ -> self.outputSamFile: an @SQ line per reference sequence in FASTA order (names cut at the
        first blank), then the records in FASTQ order, a read's sorted by (strand, reference, reference position, read position).  A
        read without a match gets no record."""
        from .. import ingest, realign
        from ..analyses.utils import _context
        ctx = _context()  # raises NprError NPR_ERR_NO_DEVICE without a GPU: there is no host fallback
        self._seeds = self._chains = None  # (a second run() keeps nothing of the first)
        fa = ingest.FastaTable(self.referenceFastaFile)
        fq = ingest.FastqTable(self.readFastqFile)
        begin, end = np.ascontiguousarray(fq.seq_span[:, 0]), np.ascontiguousarray(fq.seq_span[:, 1])
        index = ctx.seed_index_csr(fa.seq, fa.off, self.k)
        strands = 3 if self.bothStrands else 1
        try:
            if self.fused:
                hit_off, hits, *chains = index.map(fq.text, begin, end, self.minLength, strands, self.maxGap, rows=True)
                self._chains = tuple(chains)
            else:
                hit_off, hits = index.matches(fq.text, begin, end, self.minLength, strands)
        finally:
            index.close()
        self._seeds = (fa, fq, begin, end, hit_off, hits)
        records, _ = realign.seed_sam_text(fq.text, fq.name_span, begin, end, [name.encode() for name in fa.names], hit_off, hits)
        with open(self.outputSamFile, "wb") as fh:
            for name, length in zip(fa.names, np.diff(fa.off)):
                fh.write(("@SQ\tSN:%s\tLN:%d\n" % (name, length)).encode())
            fh.write(records.tobytes())

    def _chainsOfRun(self):
        """(chain_off, chains, ops_off, ops) of the hits run() kept: what a fused run() made with them, else made of them now."""
        from ..analyses.utils import _context
        fa, fq, begin, end, hit_off, hits = self._seeds
        return self._chains or _context().seed_chains(fq.lengths, np.diff(fa.off), hit_off, hits, self.maxGap)

    def _writeChainedSam(self, path):
        """The chained SAM of the hits run() kept: the header run() wrote, then one global alignment per (read, reference), in the order
        utils.chainSamFile writes them."""
        from .. import realign
        fa, fq, begin, end, hit_off, hits = self._seeds
        chain_off, chains, ops_off, ops = self._chainsOfRun()
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
        if not self.fused or doEm:  # (the trainer reads its alignments from a SAM file, fused or not)
            self._writeChainedSam(tempSamFile)
        if hmmFile is not None and doEm:
            utils.learnModelFromSamFileTargetFn(self, tempSamFile, self.readFastqFile, self.referenceFastaFile, hmmFile)
        else:
            assert not doEm
        if not self.fused:
            return utils.realignSamFile(tempSamFile, self.outputSamFile, self.readFastqFile, self.referenceFastaFile, hmmFile, gapGamma, matchGamma)
        from .. import job
        results = job.realign_source(job.SeedSource(self._seeds[0], self._seeds[1], *self._chainsOfRun()), self.outputSamFile, hmm=hmmFile,
                                     gapGamma=gapGamma, matchGamma=matchGamma)["results"]
        return utils.raiseForFailedRecords(results, self.outputSamFile)

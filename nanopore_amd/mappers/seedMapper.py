"""SeedMapper: the build's own base mapper.  The reference's base mappers (last, bwa, lastz, blasr) are external binaries and out of
scope here (abstractMapper.py); this one needs nothing but the device: every maximal exact match of at least `minLength` bases between a
read (either strand) and a reference sequence becomes one local-hit SAM record, found by the seed index of csrc/npr_seed.hip
(include/nprealign.h, "exact-match seeding").  The records are what chainSamFile and realignSamFile expect of a base mapper: POS, a
CIGAR of one M run between hard clips, FLAG 16 and reverse-complemented bases for the reverse strand.  No gapped extension: that is the
realigner's part.
"""
import numpy as np

from .abstractMapper import AbstractMapper


class SeedMapper(AbstractMapper):
    k = 16             # index window: positions whose next k bases are all A C G T are indexed
    minLength = 20     # shortest match reported (>= k)
    bothStrands = True

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
        records, _ = realign.seed_sam_text(fq.text, fq.name_span, begin, end, [name.encode() for name in fa.names], hit_off, hits)
        with open(self.outputSamFile, "wb") as fh:
            for name, length in zip(fa.names, np.diff(fa.off)):
                fh.write(("@SQ\tSN:%s\tLN:%d\n" % (name, length)).encode())
            fh.write(records.tobytes())

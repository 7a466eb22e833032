"""The per-position pileup of a SAM file on the device: host glue, no DP.

The reference gets these numbers from samtools after converting the SAM to BAM, sorting and indexing it
(`samtools depth`, nanopore/metaAnalyses/coverageDepth.py:49-65; `samtools mpileup`, analyses/consensus.py).  Here the
records go from the file's bytes through the whole-file scanners (ingest.py / csrc/npr_io.cpp) to `Pileup.add_csr`
(include/nprealign.h: npr_pileup_add; csrc/npr_pileup.hip) without a Python object per record, and the table comes
back from the device.  No CPU fallback.

Not reproduced: samtools 0.1.19 admits at most 8000 records to a position's pileup (bam_pileup.c, maxcnt), which
depends on the order of the file; the device table has no cap.
"""
import numpy as np

from .. import ingest

# what samtools' pileup leaves out: unmapped, secondary, QC-fail and duplicate records (BAM_DEF_MASK); a supplementary
# record (0x800) is counted, and the reference's call sets no mapping or base quality threshold
FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400


def kept_by_samtools(flags):
    """Boolean mask of the records whose FLAG samtools' pileup keeps."""
    return (np.asarray(flags, dtype=np.int64) & FLAG_MASK) == 0


def pileup_of_sam(ctx, samFile, referenceFastaFile):
    """-> (names, ref_lengths, Pileup): the table of the records of `samFile` that samtools' pileup would keep, rows in the
    order of the header's @SQ lines.  The sequences of `referenceFastaFile` must be the ones the header names (their
    lengths are compared); the caller closes the Pileup."""
    sam = ingest.SamText(samFile)
    names, lengths = list(sam.references), np.asarray(sam.lengths, dtype=np.int64)
    fasta = ingest.FastaTable(referenceFastaFile)
    for name, length in zip(names, lengths):
        if name not in fasta.index:
            raise KeyError("%s: @SQ sequence %r is not in %s" % (samFile, name, referenceFastaFile))
        k = fasta.index[name]
        if int(fasta.off[k + 1] - fasta.off[k]) != int(length):
            raise ValueError("%s: @SQ sequence %r has LN %d, %s holds %d bases" % (samFile, name, length, referenceFastaFile, fasta.off[k + 1] - fasta.off[k]))
    pileup = ctx.pileup(lengths)
    try:
        fields = sam.parse()
        if len(fields):
            with_reference = sam.records_with_a_reference(fields, sam.span)
            use = with_reference & kept_by_samtools(fields[:, ingest.F_FLAG])
            ops_off, ops = sam.guides(fields)
            start = np.zeros((len(fields), 2), dtype=np.int64)
            start[:, 0] = fields[:, ingest.F_POS]
            pileup.add_csr(sam.text, fields[:, ingest.F_QUERY_LO], fields[:, ingest.F_QUERY_HI], ops, ops_off,
                           np.where(with_reference, fields[:, ingest.F_TID], 0), start=start, use=use)
    except Exception:
        pileup.close()
        raise
    return names, lengths, pileup


def depth_text(names, ref_lengths, depth, covered):
    """The text of `samtools depth`: `name\\t1-based position\\tdepth\\n` for every covered position (one with an M or a
    deletion column; a position under deletions alone has depth 0), sequences in the given order."""
    depth, covered = np.asarray(depth), np.asarray(covered, dtype=bool)
    out, row = [], 0
    for name, length in zip(names, ref_lengths):
        length = int(length)
        pos = np.nonzero(covered[row:row + length])[0]
        out.append("".join("%s\t%d\t%d\n" % (name, p + 1, d) for p, d in zip(pos.tolist(), depth[row + pos].tolist())))
        row += length
    return "".join(out)

"""The per-position pileup of a SAM file on the device: host glue, no DP.

The reference gets these numbers from samtools after converting the SAM to BAM, sorting and indexing it
(`samtools depth`, nanopore/metaAnalyses/coverageDepth.py:49-65; `samtools mpileup`, analyses/consensus.py).  Here the
records go from the file's bytes through the whole-file scanners (ingest.py / csrc/npr_io.cpp) to `Pileup.add_csr`
(include/nprealign.h: npr_pileup_add; csrc/npr_pileup.hip) without a Python object per record, and the table comes
back from the device.  A BAM file does not become text first: `pileup_of_bam` opens it on the device and its records
are added where they lie (`Pileup.add_bam`; npr_bam_open, npr_pileup_add_bam; csrc/npr_bampile.hip).  No CPU fallback.

Not reproduced: samtools 0.1.19 admits at most 8000 records to a position's pileup (bam_pileup.c, maxcnt), which
depends on the order of the file; the device table has no cap.
"""
import os

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


def region_index(bamFile, region, index=None, ctx=None, data=None):
    """The bytes of the BAI file that serves a region query on bamFile, or None: `index` (a path) when given, else bamFile + ".bai" when
    there is a region and that file exists; else, with a context, the index of the file as it stands, made in memory on the device
    (Context.bam_index; data: the file image when the caller has read it) -- a file the indexer refuses because its records are not in
    coordinate order has no index: None, and the caller restricts the whole file, which works in any order.  Any other refusal raises."""
    if region is None:
        return None
    if index is None and os.path.exists(bamFile + ".bai"):
        index = bamFile + ".bai"
    if index is not None:
        return np.fromfile(index, dtype=np.uint8)
    if ctx is None:
        return None
    from .._lib import NprError
    try:
        return ctx.bam_index(np.fromfile(bamFile, dtype=np.uint8) if data is None else data)
    except NprError as e:
        if "coordinate order" in str(e):
            return None
        raise


def pileup_of_bam(ctx, bamFile, referenceFastaFile=None, region=None, index=None):
    """-> (names, ref_lengths, Pileup): the table of the records of `bamFile` that samtools' pileup would keep, rows in the order
    of the BAM header's reference sequences, whose names and lengths are the ones returned.  The file is inflated and walked on
    the device and its records are added where they lie (Pileup.add_bam; include/nprealign.h: npr_pileup_add_bam): no SAM text,
    no parse on the host.  With `referenceFastaFile`, its sequences must be the ones the header names (their lengths are
    compared, as pileup_of_sam compares them); the caller closes the Pileup.
    region (Context.bam_open says how one is written; `samtools mpileup -r`): only the records that overlap it are added -- found
    through the BAI file `index` (default: bamFile + ".bai" when it exists, else an index made in memory: region_index), so that only
    the blocks it names are inflated; a file that is not coordinate-sorted is restricted whole on the device.  WHOLE records are added: the table still has all rows, and it is complete inside
    [beg, end) of the region's sequence and partial outside it (a record that reaches out of the region adds its columns there too)."""
    data = np.fromfile(bamFile, dtype=np.uint8)
    with ctx.bam_open(data, index=region_index(bamFile, region, index, ctx=ctx, data=data), region=region) as stream:
        names, lengths = list(stream.references), np.asarray(stream.lengths, dtype=np.int64)
        if referenceFastaFile is not None:
            fasta = ingest.FastaTable(referenceFastaFile)
            for name, length in zip(names, lengths):
                if name not in fasta.index:
                    raise KeyError("%s: reference sequence %r is not in %s" % (bamFile, name, referenceFastaFile))
                k = fasta.index[name]
                if int(fasta.off[k + 1] - fasta.off[k]) != int(length):
                    raise ValueError("%s: reference sequence %r has length %d, %s holds %d bases" % (bamFile, name, length, referenceFastaFile, fasta.off[k + 1] - fasta.off[k]))
        pileup = ctx.pileup(lengths)
        try:
            pileup.add_bam(stream, FLAG_MASK)
        except Exception:
            pileup.close()
            raise
    return names, lengths, pileup


def alignment_quality_of_sam(ctx, samFile, referenceFastaFile, n_windows=400):
    """-> (names, ref_lengths, Coverage, AlignQuality): the alignment-quality tables of the QualiMap analysis (include/nprealign.h:
    npr_pileup_coverage, npr_align_quality) over the records pileup_of_sam keeps -- samtools' flag mask, records with a reference --
    from ONE parse of the file: the pileup is built and reduced to windows, and the same arrays go through the per-record pass with
    MAPQ and the soft clips of either end.  Rows and windows are in the order of the header's @SQ lines."""
    sam = ingest.SamText(samFile)
    names, lengths = list(sam.references), np.asarray(sam.lengths, dtype=np.int64)
    fasta = ingest.FastaTable(referenceFastaFile)
    ref_off = np.zeros(len(names) + 1, dtype=np.int64)
    np.cumsum(lengths, out=ref_off[1:])
    ref_text = np.zeros(max(int(ref_off[-1]), 1), dtype=np.uint8)
    for i, (name, length) in enumerate(zip(names, lengths)):
        if name not in fasta.index:
            raise KeyError("%s: @SQ sequence %r is not in %s" % (samFile, name, referenceFastaFile))
        k = fasta.index[name]
        if int(fasta.off[k + 1] - fasta.off[k]) != int(length):
            raise ValueError("%s: @SQ sequence %r has LN %d, %s holds %d bases" % (samFile, name, length, referenceFastaFile, fasta.off[k + 1] - fasta.off[k]))
        ref_text[ref_off[i]:ref_off[i + 1]] = fasta.seq[fasta.off[k]:fasta.off[k + 1]]
    fields = sam.parse()
    n = len(fields)
    with_reference = sam.records_with_a_reference(fields, sam.span) if n else np.zeros(0, dtype=bool)
    use = with_reference & kept_by_samtools(fields[:, ingest.F_FLAG])
    ops_off, ops = sam.guides(fields)
    start = np.zeros((n, 2), dtype=np.int64)
    start[:, 0] = fields[:, ingest.F_POS]
    tid = np.where(with_reference, fields[:, ingest.F_TID], 0)
    # the clips as the parse gives them; an unselected record's may be anything: they are not looked at
    clip = np.zeros((n, 2), dtype=np.int64)
    clip[:, 0] = np.where(use, fields[:, ingest.F_QUERY_LO] - fields[:, ingest.F_SEQ_LO], 0)
    clip[:, 1] = np.where(use, fields[:, ingest.F_SEQ_HI] - fields[:, ingest.F_QUERY_HI], 0)
    mapq = np.where(use, fields[:, ingest.F_MAPQ], 0)
    pileup = ctx.pileup(lengths)
    try:
        if n:
            pileup.add_csr(sam.text, fields[:, ingest.F_QUERY_LO], fields[:, ingest.F_QUERY_HI], ops, ops_off, tid, start=start, use=use)
        coverage = pileup.coverage(ref_text, ref_off, n_windows)
    finally:
        pileup.close()
    quality = ctx.align_quality(sam.text, fields[:, ingest.F_QUERY_LO], fields[:, ingest.F_QUERY_HI], ops, ops_off, tid, mapq, clip, ref_text, ref_off,
                                start=start, use=use, n_windows=n_windows)
    return names, lengths, coverage, quality


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

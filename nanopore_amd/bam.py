"""SAM text to a coordinate-sorted BAM file and its BAI index through libnprealign.so (include/nprealign.h, "coordinate-sorted BAM";
csrc/npr_bam_host.cpp, csrc/npr_bam.hip): what the reference gets from samToBamFile, pysam.sort and pysam.index
(nanopore/metaAnalyses/customTrackAssemblyHub.py:56-62), without samtools.  The file is mapped and parsed as ingest.SamText does; the
records are ordered, encoded, framed and indexed on the device: BGZF with stored deflate blocks by default (every byte as before), or,
with compress=True, with every block compressed there (npr_sam_bam_deflate, csrc/npr_deflate.hip).  No CPU fallback.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import _sized, check, ptr
from .realign import _arr

TAIL_COLS = _lib.SAM_TAIL_COLS
(T_RNEXT, T_PNEXT, T_TLEN, T_QUAL_LO, T_QUAL_HI, T_TAGS_LO, T_TAGS_HI, T_STATUS) = range(TAIL_COLS)


def parse_tail(sam, fields, lo=0, hi=None):
    """The columns npr_sam_parse leaves aside, for lines lo .. hi of an ingest.SamText (include/nprealign.h: npr_sam_parse_tail):
    int64 [hi - lo, TAIL_COLS]."""
    hi = len(sam.span) if hi is None else hi
    n = hi - lo
    tail = np.zeros((n, TAIL_COLS), dtype=np.int64)
    if n:
        span, fields = np.ascontiguousarray(sam.span[lo:hi]), _arr(fields, np.int64)
        check(_lib.load().npr_sam_parse_tail(ptr(sam.text), ptr(span), ptr(fields), n, ptr(sam._rn), ptr(sam._rn_off), len(sam.references), ptr(tail)),
              "npr_sam_parse_tail")
    return tail


def bam_tags(text, tail):
    """The optional fields of parsed lines as BAM auxiliary bytes (npr_bam_tags): (tag_off int64 [n + 1], bytes uint8)."""
    tail = _arr(tail, np.int64)
    n = len(tail)
    off = np.zeros(n + 1, dtype=np.int64)
    out = _sized(_lib.load().npr_bam_tags, "npr_bam_tags", [ptr(text), ptr(tail), n, ptr(off)])
    return off, out


def bam_header(header, sort=True):
    """The bytes of a BAM file before its first record, from the SAM header text (npr_bam_header): (uint8 array, reference lengths)."""
    L = _lib.load()
    header = np.frombuffer(bytes(header), dtype=np.uint8)
    n_refs = C.c_int64(0)
    total = check(L.npr_bam_header(ptr(header), len(header), int(bool(sort)), None, 0, C.byref(n_refs), None, 0), "npr_bam_header")
    out, lengths = np.zeros(total, dtype=np.uint8), np.zeros(n_refs.value, dtype=np.int64)
    check(L.npr_bam_header(ptr(header), len(header), int(bool(sort)), ptr(out), total, C.byref(n_refs), ptr(lengths), len(lengths)), "npr_bam_header")
    return out, lengths


def bai_write(ref_len, run_tid, run_bin, run_beg, run_end, linear, meta, n_no_coor):
    """The BAI file's bytes from the tables npr_sam_bam returns (npr_bai_write)."""
    ref_len, run_tid, run_bin = _arr(ref_len, np.int64), _arr(run_tid, np.int32), _arr(run_bin, np.uint32)
    run_beg, run_end, linear, meta = (_arr(a, np.uint64) for a in (run_beg, run_end, linear, meta))
    args = [len(ref_len), ptr(ref_len), len(run_tid), ptr(run_tid), ptr(run_bin), ptr(run_beg), ptr(run_end), ptr(linear), ptr(meta), int(n_no_coor)]
    return _sized(_lib.load().npr_bai_write, "npr_bai_write", args)


def linear_windows(ref_len):
    """First window of every reference in the `linear` table of npr_sam_bam: int64 [n_refs + 1]."""
    off = np.zeros(len(ref_len) + 1, dtype=np.int64)
    np.cumsum(((np.asarray(ref_len, dtype=np.int64) - 1) >> 14) + 1, out=off[1:])
    return off


def sort_order(ctx, tid, pos, flag):
    """The stable coordinate order of records on the device (npr_bam_sort_order): int32 [n], the record at every place."""
    tid, pos, flag = _arr(tid, np.int32), _arr(pos, np.int64), _arr(flag, np.int32)
    if not len(tid) == len(pos) == len(flag):
        raise _lib.NprError(_lib.ERR_INVALID, "npr_bam_sort_order", "tid, pos and flag differ in number")
    order = np.zeros(len(tid), dtype=np.int32)
    check(ctx._L.npr_bam_sort_order(ctx._h, len(tid), ptr(tid), ptr(pos), ptr(flag), ptr(order)), "npr_bam_sort_order", ctx)
    return order


def bgzf_frame(ctx, data, cap=None):
    """`data` (bytes or a uint8 array) as a BGZF stream of stored blocks (bgzf_deflate: compressed ones), framed and checksummed on the device (npr_bgzf_frame): uint8 array.
    cap: the size of the output buffer handed over (default: what the stream needs)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    total = check(ctx._L.npr_bgzf_frame(ctx._h, ptr(data), len(data), None, 0), "npr_bgzf_frame", ctx)
    out = np.zeros(total if cap is None else max(int(cap), 1), dtype=np.uint8)
    check(ctx._L.npr_bgzf_frame(ctx._h, ptr(data), len(data), ptr(out), len(out) if cap is None else int(cap)), "npr_bgzf_frame", ctx)
    return out[:total]


def bgzf_deflate(ctx, data, cap=None):
    """`data` as a BGZF stream whose blocks are compressed on the device (npr_bgzf_deflate): (uint8 array, block_off int64 [blocks + 1]: the
    file offset of every block and of the end-of-file block).  cap: the size of the output buffer handed over (default: the stored length)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    bound = check(ctx._L.npr_bgzf_deflate(ctx._h, ptr(data), len(data), None, 0, None), "npr_bgzf_deflate", ctx)
    out = np.zeros(bound if cap is None else max(int(cap), 1), dtype=np.uint8)
    block_off = np.zeros((len(data) + _lib.BGZF_PAYLOAD - 1) // _lib.BGZF_PAYLOAD + 1, dtype=np.int64)
    total = check(ctx._L.npr_bgzf_deflate(ctx._h, ptr(data), len(data), ptr(out), len(out) if cap is None else int(cap), ptr(block_off)), "npr_bgzf_deflate", ctx)
    return out[:total], block_off


def deflate_last(ctx):
    """Of the last stream the context compressed (npr_deflate_last): {"a", "b", "c": the blocks emitted as dynamic Huffman over matches and
    literals, over the literals alone, and stored; "stream_bytes": the uncompressed stream's length}."""
    out = np.zeros(4, dtype=np.int64)
    check(ctx._L.npr_deflate_last(ctx._h, ptr(out)), "npr_deflate_last", ctx)
    return {"a": int(out[0]), "b": int(out[1]), "c": int(out[2]), "stream_bytes": int(out[3])}


def convert(ctx, sam, fields, tail, tag_off, tags, header, ref_len, sort=True, index=True, compress=False):
    """The device call alone (npr_sam_bam, or npr_sam_bam_deflate with compress) on a parsed ingest.SamText: (the BAM file image, the BAI
    file's bytes or None)."""
    n, n_refs = len(sam), len(ref_len)
    want_index = bool(sort and index)
    run_tid, run_bin = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32)
    run_beg, run_end = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    linear, meta = np.zeros(max(int(linear_windows(ref_len)[-1]), 1), dtype=np.uint64), np.zeros((max(n_refs, 1), 4), dtype=np.uint64)
    n_runs, n_no_coor = C.c_int64(0), C.c_int64(0)
    head = [ctx._h, ptr(sam.text), len(sam.text), ptr(sam.span), ptr(fields), ptr(tail), n, ptr(tag_off), ptr(tags), ptr(header), len(header), n_refs,
            ptr(ref_len), int(bool(sort))]
    index_args = [C.byref(n_runs), ptr(run_tid), ptr(run_bin), ptr(run_beg), ptr(run_end), ptr(linear), ptr(meta), C.byref(n_no_coor)]
    # a bound instead of a sizing call (pages nobody touches cost nothing): a record is at most twice its line plus its tag bytes
    stream = len(header) + 2 * int(sam.line_lengths().sum()) + int(tag_off[-1]) + 64 * n
    out = np.empty(stream + 31 * (stream // _lib.BGZF_PAYLOAD + 1) + 28, dtype=np.uint8)
    entry = "npr_sam_bam_deflate" if compress else "npr_sam_bam"
    total = int(check(getattr(ctx._L, entry)(*head, ptr(out), len(out), *index_args), entry, ctx))
    r = n_runs.value
    bai = bai_write(ref_len, run_tid[:r], run_bin[:r], run_beg[:r], run_end[:r], linear, meta[:n_refs], n_no_coor.value) if want_index else None
    return out[:total], bai


def sam_to_bam(ctx, samFile, bamFile, sort=True, index=True, compress=False):
    """samFile as a BAM file (npr_sam_bam): coordinate-sorted with bamFile + ".bai" beside it (sort and index), or in the file's order.
    compress: the BGZF blocks are compressed on the device (npr_sam_bam_deflate) instead of stored; the records are the same bytes.
    A line that does not parse, an RNAME the header does not name or a malformed cigar raises and leaves no file; nothing is dropped.
    -> {"records", "references", "bytes", "no_coordinate", "mapped", "unmapped"}, with compress also "stream_bytes" (the uncompressed
    stream's length)."""
    from .ingest import SamText
    sam = SamText(samFile)
    n = len(sam)
    fields = sam.parse()
    tail = parse_tail(sam, fields)
    tag_off, tags = bam_tags(sam.text, tail)
    header, ref_len = bam_header(sam.header, sort)
    out, bai = convert(ctx, sam, fields, tail, tag_off, tags, header, ref_len, sort, index, compress)
    tmp = bamFile + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            out.tofile(fh)
        os.replace(tmp, bamFile)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    if bai is not None:
        with open(bamFile + ".bai", "wb") as fh:
            bai.tofile(fh)
    flag = fields[:, 7]
    counts = {"records": n, "references": len(ref_len), "bytes": len(out), "no_coordinate": int((fields[:, 10] < 0).sum()),
              "mapped": int(((flag & 4) == 0).sum()), "unmapped": int(((flag & 4) != 0).sum())}
    if compress:
        counts["stream_bytes"] = int(deflate_last(ctx)["stream_bytes"])
    return counts

"""SAM text to a coordinate-sorted BAM file and its BAI index through libnprealign.so (include/nprealign.h, "coordinate-sorted BAM";
csrc/npr_bam_host.cpp, csrc/npr_bam.hip): what the reference gets from samToBamFile, pysam.sort and pysam.index
(nanopore/metaAnalyses/customTrackAssemblyHub.py:56-62), without samtools.  The file is mapped and parsed as ingest.SamText does; the
records are ordered, encoded, framed and indexed on the device: BGZF with stored deflate blocks by default (every byte as before), or,
with compress=True, with every block compressed there (npr_sam_bam_deflate, csrc/npr_deflate.hip).  No CPU fallback.
"""
import ctypes as C
import os
import re

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


INFLATE_STATUS = ("ok", "BTYPE 3", "a stored block's LEN is not ~NLEN", "over-subscribed code lengths", "incomplete code lengths",
                  "a repeat code with no length before it or past HLIT + HDIST", "no code for symbol 256", "a symbol or code that does not exist",
                  "a distance that reaches before the block's first byte", "output past ISIZE", "input past the deflate data's end",
                  "deflate data left after the final block", "the produced length is not ISIZE", "the CRC-32 is not the trailer's",
                  "the decoder's step bound")   # csrc/npr_inflate.h INF_*


def bgzf_scan(data):
    """The block table of a BGZF file image (npr_bgzf_scan, host code): (block_off, stream_off), int64 [blocks + 1] each: the file offset of
    every block and the stream offset of its payload; last the end-of-file block's offset and the stream's length.  A file that does not
    end with the end-of-file block, or whose blocks do not chain to it, raises."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    L, n = _lib.load(), C.c_int64(0)
    check(L.npr_bgzf_scan(ptr(data), len(data), None, None, 0, C.byref(n)), "npr_bgzf_scan")
    block_off, stream_off = np.zeros(n.value + 1, dtype=np.int64), np.zeros(n.value + 1, dtype=np.int64)
    check(L.npr_bgzf_scan(ptr(data), len(data), ptr(block_off), ptr(stream_off), n.value + 1, C.byref(n)), "npr_bgzf_scan")
    return block_off, stream_off


def bgzf_inflate(ctx, data, out=None):
    """The payloads of a BGZF file image (bytes or a uint8 array), every block inflated on the device (npr_bgzf_inflate): uint8 array.  The
    blocks may come from any writer.  A block that is refused raises NprError and nothing is written; inflate_last(ctx) says which and why.
    out: a uint8 array to write into (default: a new one)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    total = check(ctx._L.npr_bgzf_inflate(ctx._h, ptr(data), len(data), None, 0), "npr_bgzf_inflate", ctx)
    if out is None:
        out = np.empty(max(total, 1), dtype=np.uint8)
    check(ctx._L.npr_bgzf_inflate(ctx._h, ptr(data), len(data), ptr(out), len(out)), "npr_bgzf_inflate", ctx)
    return out[:total]


def inflate_last(ctx):
    """Of the last file the context inflated (npr_inflate_last): {"blocks", "failed_block" (-1: none), "status", "reason", "stream_bytes"}."""
    out = np.zeros(4, dtype=np.int64)
    check(ctx._L.npr_inflate_last(ctx._h, ptr(out)), "npr_inflate_last", ctx)
    status = int(out[2])
    return {"blocks": int(out[0]), "failed_block": int(out[1]), "status": status,
            "reason": INFLATE_STATUS[status] if 0 <= status < len(INFLATE_STATUS) else "unknown", "stream_bytes": int(out[3])}


def bam_aux_text(aux, aux_off, placeholder=None):
    """The auxiliary bytes of records as TAG:TYPE:VALUE text (npr_bam_aux_text, host code, the inverse of bam_tags): (text_off int64 [n + 1],
    text uint8, cg int64 [n, 2]: with placeholder[i] set, where the elements of record i's CG:B:I field lie and how many; -1 without one)."""
    aux, aux_off = _arr(aux, np.uint8), _arr(aux_off, np.int64)
    n = len(aux_off) - 1
    placeholder = None if placeholder is None else _arr(placeholder, np.uint8)
    text_off, cg = np.zeros(n + 1, dtype=np.int64), np.full((max(n, 1), 2), -1, dtype=np.int64)
    out = _sized(_lib.load().npr_bam_aux_text, "npr_bam_aux_text", [ptr(aux), ptr(aux_off), n, ptr(placeholder), ptr(text_off), ptr(cg)])
    return text_off, out, cg[:n]


def bam_sam(ctx, data):
    """A BAM file image as SAM text (npr_bam_sam): (uint8 array: the header text, then a line per record; the number of records)."""
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    stream = check(ctx._L.npr_bgzf_inflate(ctx._h, ptr(data), len(data), None, 0), "npr_bgzf_inflate", ctx)
    # a bound instead of a sizing call (pages nobody touches cost nothing): a stream byte becomes at most 5 text bytes (an element of a B:c array:
    # "-128,"), a 4-byte number at most 12 with its tab
    out = np.empty(6 * stream + 64, dtype=np.uint8)
    n = C.c_int64(0)
    total = int(check(ctx._L.npr_bam_sam(ctx._h, ptr(data), len(data), ptr(out), len(out), C.byref(n)), "npr_bam_sam", ctx))
    return out[:total], n.value


def bam_to_sam(ctx, bamFile, samFile):
    """bamFile as SAM text in samFile (npr_bam_sam): the blocks inflated, the records walked and the lines written on the device, the
    auxiliary fields turned to text on the host.  A file that is not BGZF, a block that does not inflate, a bad BAM magic or a malformed
    record raises and leaves no file.  -> {"records", "references", "bytes", "stream_bytes", "blocks"}."""
    data = np.fromfile(bamFile, dtype=np.uint8)
    text, n = bam_sam(ctx, data)
    last = inflate_last(ctx)
    tmp = samFile + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            text.tofile(fh)
        os.replace(tmp, samFile)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    k = 1 << 16   # the header's @SQ lines: the header comes first, and is looked for in a prefix that grows until it ends
    while True:
        head = text[:k].tobytes()
        m = re.search(rb"(?m)^[^@]", head)
        if m or k >= len(text):
            break
        k *= 4
    references = len(re.findall(rb"(?m)^@SQ\t", head[:m.start()] if m else head))
    return {"records": int(n), "references": references, "bytes": int(len(text)), "stream_bytes": last["stream_bytes"], "blocks": last["blocks"]}


def bam_references(data):
    """The reference names and lengths of a BAM file image, read on the host from as many of its first blocks as the header fills (bgzf_scan
    for where they lie, zlib for their few kilobytes): (names, lengths).  What turns a region's name into the refID an indexed query needs
    before anything is on the device; the device checks the header itself."""
    return bam_head(data)[1:]


def bam_head(data):
    """bam_references with the header text before them: (text as bytes, names, lengths)."""
    import struct
    import zlib
    data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
    block_off, _ = bgzf_scan(data)
    head, used = b"", 0

    def have(n):   # the first n bytes of the stream, when the file has them
        nonlocal head, used
        while len(head) < n and used < len(block_off) - 1:
            block = data[block_off[used]:block_off[used + 1]].tobytes()
            xlen = struct.unpack_from("<H", block, 10)[0]
            head += zlib.decompress(block[12 + xlen:-8], -15)
            used += 1
        if len(head) < n:
            raise _lib.NprError(_lib.ERR_INVALID, "bam_references", "the BAM header runs past the file")
    have(12)
    if head[:4] != b"BAM\1":
        raise _lib.NprError(_lib.ERR_INVALID, "bam_references", "no BAM magic")
    at = 8 + struct.unpack_from("<i", head, 4)[0]
    have(at + 4)
    text = head[8:at]
    n_ref = struct.unpack_from("<i", head, at)[0]
    at += 4
    names, lengths = [], np.zeros(max(n_ref, 0), dtype=np.int64)
    for k in range(n_ref):
        have(at + 4)
        l_name = struct.unpack_from("<i", head, at)[0]
        have(at + 8 + l_name)
        names.append(head[at + 4:at + 4 + l_name - 1].decode())
        lengths[k] = struct.unpack_from("<i", head, at + 4 + l_name)[0]
        at += 8 + l_name
    return text, names, lengths


def bai_chunks(bai, tid, beg, end):
    """The chunks of a BAM file a reader has to visit for [beg, end) of reference tid, 0-based and half-open, from the bytes of its BAI
    index (npr_bai_chunks, host code, which states the rule): (uint64 [n, 2] of virtual offsets (beg, end), disjoint and ascending; the
    index's n_ref)."""
    bai = np.frombuffer(bytes(bai), dtype=np.uint8) if isinstance(bai, (bytes, bytearray)) else _arr(bai, np.uint8)
    L, n_ref = _lib.load(), C.c_int64(-1)
    n = int(check(L.npr_bai_chunks(ptr(bai), len(bai), int(tid), int(beg), int(end), None, None, 0, C.byref(n_ref)), "npr_bai_chunks"))
    cb, ce = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
    check(L.npr_bai_chunks(ptr(bai), len(bai), int(tid), int(beg), int(end), ptr(cb), ptr(ce), n, C.byref(n_ref)), "npr_bai_chunks")
    return np.stack([cb[:n], ce[:n]], axis=1), int(n_ref.value)


def bam_region_to_sam(ctx, bamFile, region, samFile, index=None):
    """The records of bamFile that overlap `region` (Context.bam_open says how one is written) as SAM text in samFile, under the file's
    header: `samtools view -h bamFile region`.  index: the path of the BAI file; by default bamFile + ".bai" when that file exists --
    then only the blocks it names are inflated (npr_bam_open_region) --, else the file is opened whole and restricted on the device
    (npr_bam_stream_restrict).  A malformed file or index raises and leaves no file.
    -> {"records", "bytes", "stream_bytes", "blocks", "indexed"}: blocks and stream_bytes are what was inflated."""
    data = np.fromfile(bamFile, dtype=np.uint8)
    if index is None and os.path.exists(bamFile + ".bai"):
        index = bamFile + ".bai"
    bai = None if index is None else np.fromfile(index, dtype=np.uint8)
    with ctx.bam_open(data, index=bai, region=region) as stream:
        last = inflate_last(ctx)
        text, n = stream.sam_text(), stream.n_records
    tmp = samFile + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            text.tofile(fh)
        os.replace(tmp, samFile)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    return {"records": int(n), "bytes": int(len(text)), "stream_bytes": last["stream_bytes"], "blocks": last["blocks"], "indexed": bai is not None}


def _write_bam(out, bai, bamOut):
    """the image to bamOut through a temporary name, and the index beside it"""
    tmp = bamOut + ".tmp"
    try:
        with open(tmp, "wb") as fh:
            out.tofile(fh)
        os.replace(tmp, bamOut)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)
    if bai is not None:
        with open(bamOut + ".bai", "wb") as fh:
            bai.tofile(fh)


def bam_merge(ctx, bamIns, bamOut, sort=True, index=True, compress=False):
    """The records of the BAM files bamIns as one BAM file, made on the device without SAM text (Context.bam_merge; include/nprealign.h:
    npr_bam_streams_bam): coordinate-sorted with bamOut + ".bai" beside it (`samtools merge`; ties keep the order of bamIns), or with
    sort=False one file after the other (`samtools cat`).  The header is the first file's; all files must have its reference sequences.
    Every record's bytes pass as they stand but for its bin.  A malformed file raises and leaves no file.
    -> {"records", "references", "bytes", "stream_bytes", "files"}."""
    streams = []
    try:
        for path in bamIns:
            streams.append(ctx.bam_open(np.fromfile(path, dtype=np.uint8)))
        out, bai = ctx.bam_merge(streams, sort=sort, index=index, compress=compress)
        references = len(streams[0].references) if streams else 0
    finally:
        for s in streams:
            s.close()
    _write_bam(out, bai, bamOut)
    last = ctx.bam_merge_last()
    return {"records": last["records"], "references": references, "bytes": int(len(out)), "stream_bytes": last["stream_bytes"], "files": len(streams)}


def bam_sort(ctx, bamIn, bamOut, index=True, compress=False):
    """bamIn coordinate-sorted as bamOut, with bamOut + ".bai" beside it (index): `samtools sort` and `samtools index`, on the device without
    SAM text (bam_merge of one file)."""
    return bam_merge(ctx, [bamIn], bamOut, sort=True, index=index, compress=compress)


def bam_region_to_bam(ctx, bamFile, region, bamOut, index=None, compress=False):
    """The records of bamFile that overlap `region` as a sorted BAM file bamOut with its own index beside it: `samtools view -b bamFile
    region`.  The file is opened as bam_region_to_sam opens it (index: the BAI file's path; by default bamFile + ".bai" when it exists,
    else the file is opened whole and restricted).  -> {"records", "bytes", "stream_bytes", "blocks", "indexed"}."""
    data = np.fromfile(bamFile, dtype=np.uint8)
    if index is None and os.path.exists(bamFile + ".bai"):
        index = bamFile + ".bai"
    bai_in = None if index is None else np.fromfile(index, dtype=np.uint8)
    with ctx.bam_open(data, index=bai_in, region=region) as stream:
        last = inflate_last(ctx)
        n = stream.n_records
        out, bai = ctx.bam_merge([stream], sort=True, index=True, compress=compress)
    _write_bam(out, bai, bamOut)
    return {"records": int(n), "bytes": int(len(out)), "stream_bytes": last["stream_bytes"], "blocks": last["blocks"], "indexed": bai_in is not None}


def bam_index(ctx, bamFile, baiFile=None):
    """The BAI index of a coordinate-sorted BAM file of any writer, made on the device (Context.bam_index; npr_bam_index): `samtools index`.
    baiFile: where it goes (default bamFile + ".bai").  A file out of order raises and leaves no file.  -> {"bytes"}."""
    bai = ctx.bam_index(np.fromfile(bamFile, dtype=np.uint8))
    with open(bamFile + ".bai" if baiFile is None else baiFile, "wb") as fh:
        bai.tofile(fh)
    return {"bytes": int(len(bai))}


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

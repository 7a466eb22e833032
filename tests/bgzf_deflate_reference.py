"""A reader of BGZF files whose blocks hold any one final DEFLATE block (SAMv1 section 4.1, RFC 1951, RFC 1952), in plain Python over
zlib: what the compressed-BAM tests read the product's files with.  Imports nothing from the product.  The result has the shape of
bam_reference.bgzf_read's, so bam_decode and bai_parse work on it; voffset_by_walking and bai_query_blocks are bam_reference's
with the virtual offsets taken from the block list of a file whose blocks have any length."""
import gzip
import struct
import zlib

import bam_reference as ref

P = ref.P
EOF_BLOCK = ref.EOF_BLOCK
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])


def bgzf_read(data):
    """-> (the stream, [(file offset of a block, stream offset of its first byte, payload bytes)]).  Every block: the header, BSIZE, one final
    DEFLATE block that a FRESH raw inflater (no history: a match that reaches before the block fails) ends exactly at the trailer, CRC-32
    and ISIZE; only the last block is short; the end-of-file block; gzip.decompress of the whole."""
    data = bytes(data)
    assert len(data) >= 28 and data[-28:] == EOF_BLOCK, "no end-of-file block"
    at, out, blocks, first = 0, [], [], 0
    while at < len(data) - 28:
        assert at + 18 <= len(data) - 28 and data[at:at + 16] == HEAD, "block header at %d" % at
        size = struct.unpack("<H", data[at + 16:at + 18])[0] + 1
        assert size >= 18 + 1 + 8 and at + size <= len(data) - 28, "BSIZE of the block at %d" % at
        body = data[at + 18:at + size - 8]
        assert body[0] & 1 == 1, "BFINAL of the block at %d" % at
        assert (body[0] >> 1) & 3 in (0, 1, 2), "BTYPE of the block at %d" % at
        z = zlib.decompressobj(-15)
        payload = z.decompress(body)
        assert z.eof and z.unused_data == b"" and z.unconsumed_tail == b"", "the deflate data of the block at %d does not end at its trailer" % at
        crc, isize = struct.unpack("<II", data[at + size - 8:at + size])
        assert isize == len(payload) and 0 < isize <= P and crc == zlib.crc32(payload), "CRC or ISIZE of the block at %d" % at
        blocks.append((at, first, isize))
        out.append(payload)
        first += isize
        at += size
    assert at == len(data) - 28
    assert all(b[2] == P for b in blocks[:-1]), "only the last block may be short"
    stream = b"".join(out)
    assert gzip.decompress(data) == stream
    return stream, blocks


def block_types(data):
    """BTYPE of every block before the end-of-file block."""
    at, out = 0, []
    while at < len(data) - 28:
        out.append((data[at + 18] >> 1) & 3)
        at += struct.unpack("<H", data[at + 16:at + 18])[0] + 1
    return out


def voffset_by_walking(blocks, u, stream_len, file_len):
    """bam_reference.voffset_by_walking for blocks of any length: the end of the stream on a full last block is where the next block would
    begin, the end-of-file block's offset file_len - 28."""
    for at, first, ln in blocks:
        if first <= u < first + ln:
            return at << 16 | (u - first)
    assert u == stream_len
    if not blocks:
        return 0
    at, first, ln = blocks[-1]
    return at << 16 | ln if ln < P else (file_len - 28) << 16


def voffset_to_stream(blocks, v, stream_len, file_len):
    """The stream offset a virtual offset of this file points at."""
    at, within = v >> 16, v & 0xffff
    for file_at, first, ln in blocks:
        if file_at == at:
            assert within <= ln
            return first + within
    assert within == 0 and at == file_len - 28, "a virtual offset at no block"
    return stream_len


def bai_query_blocks(index, records, blocks, stream_len, file_len, tid, beg, end):
    """bam_reference.bai_query for a file whose blocks lie at `blocks`."""
    bins, linear = index[tid]
    low = 0
    if linear:
        w = beg >> 14
        low = linear[w] if w < len(linear) else ref.NONE
    chunks = [c for b in ref.reg2bins(beg, end) if b in bins for c in bins[b] if c[1] > low]
    found = []
    for i, r in enumerate(records):
        v0 = voffset_by_walking(blocks, r["u0"], stream_len, file_len)
        if r["tid"] == tid and any(c[0] <= v0 < c[1] for c in chunks):
            rb = max(r["pos"], 0)
            if rb < end and max(r["end"], rb + 1) > beg:
                found.append(i)
    return found

"""The rules of npr_bam_streams_bam and npr_bam_index (include/nprealign.h, "BAM streams to BAM files") restated in plain Python on the
helpers the other BAM tests trust: bam_reference.bam_decode(any_writer=True) for a record's u0, u1 and end, bam_reference.stable_order and
record_bin, bam_region_cases.spec_index and bgzf_blocks.  Gives the expected output stream, its stored framing and the expected BAI bytes
for a list of streams, a sort flag and a block list.  Imports nothing from the product."""
import struct
import zlib

import bam_reference as ref
import bam_region_cases as rc


def measured(stream):
    """-> (refs, [record dict of bam_decode with `raw` (its bytes, block_size included), `size` and the measured `bin`])"""
    _, refs, records = ref.bam_decode(stream, any_writer=True)
    for r in records:
        r["raw"], r["size"], r["bin"] = stream[r["u0"]:r["u1"]], r["u1"] - r["u0"], ref.record_bin(r)
    return refs, records


def with_bin(raw, bin_):
    return raw[:14] + struct.pack("<H", bin_) + raw[16:]


def merged(streams, sort, header):
    """The output stream: `header`, then the records of the streams concatenated in argument order -- stably sorted by (tid, pos, FLAG)
    when `sort` -- each as it stands but for its two bin bytes.  -> (the stream, the concatenation index of the record at every place)"""
    records = [r for s in streams for r in measured(s)[1]]
    order = ref.stable_order([r["tid"] for r in records], [r["pos"] for r in records], [r["flag"] for r in records]) if sort else list(range(len(records)))
    return header + b"".join(with_bin(records[i]["raw"], records[i]["bin"]) for i in order), order


def stored_frame(stream):
    """the stream in blocks of 65 280 bytes, each one final stored deflate block, and the end-of-file block: the layout bam_reference.bgzf_read checks"""
    out = []
    for at in range(0, len(stream), ref.P):
        p = stream[at:at + ref.P]
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", len(p) + 30) + b"\x01" +
                   struct.pack("<HH", len(p), ~len(p) & 0xffff) + p + struct.pack("<II", zlib.crc32(p), len(p)))
    return b"".join(out) + ref.EOF_BLOCK


def index_of(stream, blocks):
    """The BAI bytes of a sorted stream that lies in `blocks` ([(file offset, stream offset, ISIZE)]): spec_index over its decoded records."""
    refs, records = measured(stream)
    return rc.spec_index(records, [ln for _, ln in refs], blocks, len(stream))


def in_coordinate_order(records):
    keys = [((1 << 32) if r["tid"] < 0 else r["tid"], r["pos"]) for r in records]
    return all(a <= b for a, b in zip(keys, keys[1:]))

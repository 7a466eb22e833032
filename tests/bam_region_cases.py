"""What the region-query tests share (tests/test_bai_chunks_host.py, tests/test_gpu_bam_region.py; include/nprealign.h, "region queries"):
the records, as SAM text for the device's writer and as a BAM stream from the encoder of tests/bam_pileup_reference.py; a BGZF block walker
and an index builder by the specification's rules for the file of any writer; the rule of npr_bai_chunks restated on bam_reference.bai_parse
and reg2bins; the blocks a query has to inflate; the regions.  Imports nothing from the product.
  Three references of 300 000, 40 000 and 5 000 bases, the last without a record.  About 400 records of 300 to 600 bases (the stream spans
  more than four blocks of 65 280 bytes and records straddle their boundaries), among them: records made long with an N run (50M19900N50M,
  and one of more than 2^17 reference bases), so that bins of three levels and the linear index's backfill are in play; records that start
  or end exactly at 16 383 / 16 384; a record with FLAG 4 and a position (its interval is one base, whatever its cigar says); records of
  refID -1 at the end; one record of 65 537 operations (1M1I x 32 768, then 20000N), which a BAM file stores under the placeholder
  <l_seq>S<n>N with its operations in a CG:B:I field.  No record begins at or beyond 280 000 of the first reference."""
import struct

import numpy as np

import bam_pileup_reference as bp
import bam_reference as ref

REFS = [("chrA", 300000), ("chrB", 40000), ("chrC", 5000)]
HEADER_TEXT = "@HD\tVN:1.4\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS)
LONG_OPS = "1M1I" * 32768 + "20000N"
_RECORDS = None


def records():
    """-> [dict(name, flag, tid, pos, cigar, seq)] in the order of the SAM file (shuffled); built once."""
    global _RECORDS
    if _RECORDS is not None:
        return _RECORDS
    rng = np.random.default_rng(41)
    out = []

    def add(name, flag, tid, pos, cigar):
        l_seq = bp.consumed(bp.cigar_words(cigar), bp.READ_OPS) if cigar != "*" else 40
        out.append(dict(name=name, flag=flag, tid=tid, pos=pos, cigar=cigar, seq="".join("ACGT"[c] for c in rng.integers(0, 4, l_seq))))

    for k in range(370):
        a, b, c = (int(v) for v in rng.integers(90, 190, 3))
        cigar = "%dM%dI%dM%dD%dM" % (a, rng.integers(1, 9), b, rng.integers(1, 9), c) if k % 3 else "%dS%dM%dM" % (rng.integers(1, 20), a + b, c)
        add("a%d" % k, 16 * (k & 1), 0, int(rng.integers(0, 279000)), cigar)
    for k in range(20):
        add("b%d" % k, 0, 1, int(rng.integers(0, 39000)), "%dM2D%dM" % (rng.integers(150, 300), rng.integers(150, 300)))
    for k, pos in enumerate((1000, 15000, 16000, 100000, 120000, 262100)):
        add("n%d" % k, 0, 0, pos, "50M19900N50M")
    add("far", 0, 0, 5000, "150M140000N150M")                      # more than 2^17 reference bases: a bin of 2^20
    add("ends_16383", 0, 0, 16383 - 300, "300M"), add("ends_16384", 16, 0, 16384 - 300, "300M")
    add("starts_16383", 0, 0, 16383, "300M"), add("starts_16384", 16, 0, 16384, "300M")
    add("ends_b_16384", 0, 1, 16384 - 310, "310M"), add("starts_b_16384", 0, 1, 16384, "310M")
    add("unmapped_placed", 4, 0, 20000, "300M")                      # FLAG 4 with a position: the interval is [20000, 20001)
    add("long", 0, 0, 200000, LONG_OPS)
    for k in range(3):
        add("u%d" % k, 4, -1, -1, "*")
    order = rng.permutation(len(out))
    _RECORDS = [out[i] for i in order]
    return _RECORDS


def sam_text():
    lines = ["\t".join([r["name"], str(r["flag"]), REFS[r["tid"]][0] if r["tid"] >= 0 else "*", str(r["pos"] + 1), "30" if r["tid"] >= 0 else "0", r["cigar"], "*", "0", "0",
                        r["seq"], "*"]) for r in records()]
    return HEADER_TEXT.replace("SO:coordinate", "SO:unsorted") + "\n".join(lines) + "\n"


def sorted_stream():
    """The coordinate-sorted BAM stream of the records, by the Python encoder (no qualities, bin 0): what the host tests index."""
    recs = records()
    order = sorted(range(len(recs)), key=lambda i: ref.sort_key(recs[i]["tid"], recs[i]["pos"], recs[i]["flag"], len(REFS)))
    out = [bp.header(REFS, text=HEADER_TEXT)]
    for i in order:
        r = recs[i]
        words = bp.cigar_words(r["cigar"]) if r["cigar"] != "*" else []
        nib = [1 << "ACGT".index(c) for c in r["seq"]]
        out.append((bp.cg_record if len(words) > 65535 else bp.record)(r["name"], r["flag"], r["tid"], r["pos"], words, nib))
    return b"".join(out)


# ---------------------------------------------------------------- files of any writer
def bgzf_blocks(data):
    """-> [(file offset, stream offset, ISIZE)] of every block before the end-of-file block, by the BSIZE chain (SAMv1 section 4.1)."""
    data = bytes(data)
    assert data[-28:] == ref.EOF_BLOCK
    at, u, out = 0, 0, []
    while at < len(data) - 28:
        assert data[at:at + 4] == b"\x1f\x8b\x08\x04"
        xlen = struct.unpack_from("<H", data, at + 10)[0]
        x, bsize = at + 12, None
        while x < at + 12 + xlen:
            slen = struct.unpack_from("<H", data, x + 2)[0]
            if data[x:x + 2] == b"BC":
                bsize = struct.unpack_from("<H", data, x + 4)[0]
            x += 4 + slen
        isize = struct.unpack_from("<I", data, at + bsize + 1 - 4)[0]
        out.append((at, u, isize))
        at, u = at + bsize + 1, u + isize
    assert at == len(data) - 28
    return out


def stored_blocks(stream_len):
    """the blocks of this project's stored writer for a stream of that length: full ones of P bytes with 31 bytes around each"""
    return [(k * (ref.P + 31), k * ref.P, min(ref.P, stream_len - k * ref.P)) for k in range((stream_len + ref.P - 1) // ref.P)]


def spec_index(decoded, ref_len, blocks, stream_len):
    """The BAI file of a sorted file from its decoded records (bam_reference.bam_decode) and its blocks, by the rules of SAMv1 section 5 as
    bam_reference.expected_index states them, with the virtual offsets of bam_reference.voffset_by_walking: the bytes."""
    def vo(u):
        return ref.voffset_by_walking(blocks, u, stream_len)
    n_refs = len(ref_len)
    bins, linear, meta, no_coor, prev = [dict() for _ in range(n_refs)], [[ref.NONE] * (((ln - 1) >> 14) + 1) for ln in ref_len], [None] * n_refs, 0, None
    for r in decoded:
        v0, v1 = vo(r["u0"]), vo(r["u1"])
        key = (r["tid"], ref.record_bin(r))
        if r["tid"] >= 0:
            chunks = bins[r["tid"]].setdefault(key[1], [])
            if key == prev:
                chunks[-1] = (chunks[-1][0], v1)
            else:
                chunks.append((v0, v1))
            m = meta[r["tid"]] or [v0, v1, 0, 0]
            m[0], m[1] = min(m[0], v0), max(m[1], v1)
            m[3 if r["flag"] & 4 else 2] += 1
            meta[r["tid"]] = m
            beg = max(r["pos"], 0)
            end = max(r["end"], beg + 1)
            lin = linear[r["tid"]]
            for w in range(min(beg >> 14, len(lin) - 1), min((end - 1) >> 14, len(lin) - 1) + 1):
                lin[w] = min(lin[w], v0)
        else:
            no_coor += 1
        prev = key
    for lin in linear:
        while lin and lin[-1] == ref.NONE:
            lin.pop()
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] == ref.NONE:
                lin[w] = lin[w + 1]
    return ref.bai_bytes(bins, linear, meta, no_coor)


# ---------------------------------------------------------------- the rules restated
def chunks_rule(bai, tid, beg, end):
    """The chunks of [beg, end) of reference tid: the bins of reg2bins (never 37450), the lower bound ioffset[min(beg >> 14, n_intv - 1)]
    (0 without a window), chunks with end <= low dropped, the rest sorted by beg and merged while beg <= the running end."""
    index, _ = ref.bai_parse(bytes(bai))
    bins, linear = index[tid]
    low = linear[min(beg >> 14, len(linear) - 1)] if linear else 0
    chunks = sorted(c for b in ref.reg2bins(beg, end) if b in bins and b != 37450 for c in bins[b] if c[1] > low)
    out = []
    for c in chunks:
        if out and c[0] <= out[-1][1]:
            out[-1] = (out[-1][0], max(out[-1][1], c[1]))
        else:
            out.append(c)
    return out


def header_end(stream):
    return bp.header_end(stream)


def blocks_rule(blocks, chunks, head_end):
    """The indices of the blocks a query inflates: those that begin before the header's end, and per chunk [vb, ve) those whose file offset
    lies in [vb >> 16, ve >> 16], the last one only when ve & 0xffff > 0."""
    need = {k for k, (at, u, isize) in enumerate(blocks) if u < head_end}
    for vb, ve in chunks:
        for k, (at, u, isize) in enumerate(blocks):
            if vb >> 16 <= at < ve >> 16 or (at == ve >> 16 and ve & 0xffff > 0):
                need.add(k)
    return sorted(need)


def query_by_walking(bai, decoded, blocks, stream_len, tid, beg, end):
    """bam_reference.bai_query for the file of any writer: the records whose virtual offset lies in a chunk of chunks_rule, filtered by overlap."""
    chunks = chunks_rule(bai, tid, beg, end)
    found = []
    for i, r in enumerate(decoded):
        if r["tid"] != tid:
            continue
        v0 = ref.voffset_by_walking(blocks, r["u0"], stream_len)
        rb = max(r["pos"], 0)
        if any(c[0] <= v0 < c[1] for c in chunks) and rb < end and max(r["end"], rb + 1) > beg:
            found.append(i)
    return found


# ---------------------------------------------------------------- regions
EDGES = (16383, 16384, 16385, 32767, 32768, 131071, 131072, 131073, 147455, 147456, 262143, 262144)


def gpu_regions():
    """about a dozen (tid, beg, end): single positions on both sides of a window and a bin boundary, a whole reference, a region past the
    last record, one in the empty reference, ones that only an N run or the long record's CG operations reach"""
    return [(0, 16383, 16384), (0, 16384, 16385), (0, 131071, 131073), (0, 0, 300000), (0, 290000, 300000), (2, 0, 5000), (2, 100, 200),
            (0, 100000, 103000), (0, 90000, 90010), (0, 210000, 210005), (0, 240000, 240010), (1, 1000, 30000), (1, 16384, 16385), (0, 20000, 20001)]


def host_regions():
    """a few hundred (tid, beg, end)"""
    rng = np.random.default_rng(43)
    out = list(gpu_regions())
    for e in EDGES:
        out += [(0, e, e + 1), (0, e - 1, e), (0, e - 1, e + 1), (0, max(e - 5000, 0), e), (0, e, min(e + 5000, 300000))]
    out += [(0, 0, 1), (0, 299999, 300000), (0, 280700, 300000), (1, 0, 40000), (1, 39999, 40000), (1, 16383, 16384), (0, 0, 1 << 29), (1, 300000, 1 << 29)]
    for _ in range(200):
        beg = int(rng.integers(0, 300000))
        out.append((0, beg, min(300000, beg + int(rng.choice([1, 10, 500, 3000, 20000, 150000])))))
    for _ in range(30):
        beg = int(rng.integers(0, 40000))
        out.append((1, beg, min(40000, beg + int(rng.choice([1, 100, 5000])))))
    return out


def rebgzf(stream, member=4001, level=6):
    """the stream as another writer's file: members of about 4 KB of payload, each compressed by zlib"""
    return bp.bgzf(stream, member=member, level=level)

"""BGZF, BAM, BAI and .2bit as the specifications state them (SAMv1 sections 4, 4.1 and 5; UCSC's twoBit description), in plain Python
and numpy: the readers and the restated index rules the BAM tests compare the product against.  Imports nothing from the product."""
import bisect
import gzip
import struct
import zlib

import numpy as np

P = 65280                      # payload of a full block
EOF_BLOCK = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
OPS = "MIDNSHP=X"
BASES = "=ACMGRSVTWYHKDBN"
NONE = (1 << 64) - 1


# ---------------------------------------------------------------- BGZF
def bgzf_read(data):
    """-> (the stream, [(file offset of a block, stream offset of its first byte, payload bytes)]); every byte of every block is checked
    against the stored-deflate layout."""
    data = bytes(data)
    assert len(data) >= 28 and data[-28:] == EOF_BLOCK, "no end-of-file block"
    at, out, blocks = 0, [], []
    while at < len(data) - 28:
        head = data[at:at + 18]
        assert head[:16] == bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]), "block header at %d" % at
        bsize = struct.unpack("<H", head[16:18])[0]
        assert data[at + 18] == 1, "not one final stored block"
        ln, nln = struct.unpack("<HH", data[at + 19:at + 23])
        assert ln ^ nln == 0xffff and bsize == ln + 30 and 0 < ln <= P
        payload = data[at + 23:at + 23 + ln]
        crc, isize = struct.unpack("<II", data[at + 23 + ln:at + 31 + ln])
        assert isize == ln and crc == zlib.crc32(payload), "CRC or ISIZE of the block at %d" % at
        blocks.append((at, sum(len(p) for p in out), ln))
        out.append(payload)
        at += bsize + 1
    assert at == len(data) - 28
    assert all(b[2] == P for b in blocks[:-1]), "only the last block may be short"
    stream = b"".join(out)
    assert gzip.decompress(data) == stream
    return stream, blocks


def voffset(u):
    return ((u // P) * (P + 31)) << 16 | (u % P)


def voffset_by_walking(blocks, u, stream_len):
    """The virtual offset of stream byte u from the block list.  u == stream_len (the end of the last record) lies one past the payload
    of a short last block -- where a reader stands after the block's last byte, and where the block would grow --, and where the next
    block would begin when the last block is full."""
    for at, first, ln in blocks:
        if first <= u < first + ln:
            return at << 16 | (u - first)
    assert u == stream_len
    if not blocks:
        return 0
    at, first, ln = blocks[-1]
    return at << 16 | ln if ln < P else (at + P + 31) << 16


# ---------------------------------------------------------------- BAM
def reg2bin(beg, end):
    end -= 1
    if beg >> 14 == end >> 14:
        return ((1 << 15) - 1) // 7 + (beg >> 14)
    if beg >> 17 == end >> 17:
        return ((1 << 12) - 1) // 7 + (beg >> 17)
    if beg >> 20 == end >> 20:
        return ((1 << 9) - 1) // 7 + (beg >> 20)
    if beg >> 23 == end >> 23:
        return ((1 << 6) - 1) // 7 + (beg >> 23)
    if beg >> 26 == end >> 26:
        return ((1 << 3) - 1) // 7 + (beg >> 26)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, first in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out.extend(range(first + (beg >> shift), first + (end >> shift) + 1))
    return out


def _fmt_float(bits):
    return "%g" % struct.unpack("<f", bits)[0]


def _aux_text(b):
    out, at = [], 0
    while at < len(b):
        tag, t = b[at:at + 2].decode(), chr(b[at + 2])
        at += 3
        if t == "A":
            out.append("%s:A:%s" % (tag, chr(b[at])))
            at += 1
        elif t in "cCsSiI":
            fmt = {"c": "<b", "C": "<B", "s": "<h", "S": "<H", "i": "<i", "I": "<I"}[t]
            out.append("%s:i:%d" % (tag, struct.unpack_from(fmt, b, at)[0]))
            at += struct.calcsize(fmt)
        elif t == "f":
            out.append("%s:f:%s" % (tag, _fmt_float(b[at:at + 4])))
            at += 4
        elif t in "ZH":
            end = b.index(b"\0", at)
            out.append("%s:%s:%s" % (tag, t, b[at:end].decode()))
            at = end + 1
        elif t == "B":
            sub, count = chr(b[at]), struct.unpack_from("<I", b, at + 1)[0]
            at += 5
            fmt = {"c": "b", "C": "B", "s": "h", "S": "H", "i": "i", "I": "I", "f": "f"}[sub]
            vals = struct.unpack_from("<%d%s" % (count, fmt), b, at)
            at += count * struct.calcsize(fmt)
            out.append("%s:B:%s" % (tag, ",".join([sub] + [("%g" % v) if sub == "f" else str(v) for v in vals])))
        else:
            raise AssertionError("aux type %r" % t)
    return out


def bam_decode(stream, any_writer=False):
    """-> (header text, [(name, length)], [record dict]); a record has the SAM columns as text (`line`, with a CG tag folded back into
    CIGAR), and tid, pos, end, flag, bin, n_cigar_op, u0, u1 (its bytes in the stream).
    Two assertions hold this project's writer to more than the specification asks: the unused low nibble of an odd l_seq is 0 (section
    4.2.3 only recommends it: "the bottom 4 bits of the last byte are undefined"), and a CG tag is the record's last (section 4.2.2 says
    the tag "CG:B:I" holds the real cigar, not where it stands).  any_writer=True lifts both and keeps the specification's rule: the
    nibble is ignored, and the FIRST CG:B:I field is folded wherever it stands among the other tags -- of a record whose stored cigar is
    <l_seq>S<n>N; beside any other stored cigar a CG field is printed as the tag it is, where the default asserts.  (POS is pos + 1 for every pos,
    so pos -1 prints 0 on a real refID too: section 4.2, "0-based leftmost coordinate", -1 + 1 = SAM's 0 for "unavailable".)"""
    assert stream[:4] == b"BAM\1"
    l_text = struct.unpack_from("<i", stream, 4)[0]
    text = stream[8:8 + l_text].decode()
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    refs = []
    for _ in range(n_ref):
        l_name = struct.unpack_from("<i", stream, at)[0]
        name = stream[at + 4:at + 4 + l_name]
        assert name[-1:] == b"\0"
        refs.append((name[:-1].decode(), struct.unpack_from("<i", stream, at + 4 + l_name)[0]))
        at += 8 + l_name
    records = []
    while at < len(stream):
        u0 = at
        size, tid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", stream, at)
        body = stream[at + 36:at + 4 + size]
        at += 4 + size
        name = body[:l_name]
        assert name[-1:] == b"\0" and b"\0" not in name[:-1]
        q = l_name
        cig = struct.unpack_from("<%dI" % n_cig, body, q)
        q += 4 * n_cig
        packed = np.frombuffer(body[q:q + (l_seq + 1) // 2], dtype=np.uint8)
        nib = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)
        if l_seq & 1 and not any_writer:
            assert nib[-1] == 0
        seq = "".join(BASES[v] for v in nib[:l_seq]) or "*"
        q += (l_seq + 1) // 2
        qual = body[q:q + l_seq]
        q += l_seq
        qual = "*" if (l_seq == 0 or qual == b"\xff" * l_seq) else bytes(v + 33 for v in qual).decode()
        aux = _aux_text(body[q:])
        stored = list(cig)
        cg = [a for a in aux if a.startswith("CG:B:I")]
        if cg and any_writer and not (n_cig == 2 and stored[0] == (l_seq << 4 | 4) and stored[1] & 15 == 3):
            cg = []   # (section 4.2.2: CG holds the cigar only of a record whose stored cigar is kSmN; elsewhere it is a tag like any other)
        if cg:
            real = [int(v) for v in cg[0].split(",")[1:]]
            consumed = sum(v >> 4 for v in real if (v & 15) in (0, 2, 3, 7, 8))
            assert n_cig == 2 and stored == [l_seq << 4 | 4, consumed << 4 | 3], "the placeholder of a long cigar"
            assert any_writer or aux[-1] == cg[0], "CG comes after the record's other tags"
            at_cg = aux.index(cg[0])
            cig, aux = real, aux[:at_cg] + aux[at_cg + 1:]
        cigar = "".join("%d%s" % (v >> 4, OPS[v & 15]) for v in cig) or "*"
        consumed = sum(v >> 4 for v in cig if (v & 15) in (0, 2, 3, 7, 8))
        end = pos + 1 if (consumed == 0 or flag & 4) else pos + consumed
        rname = refs[tid][0] if tid >= 0 else "*"
        rnext = "*" if ntid < 0 else ("=" if ntid == tid else refs[ntid][0])
        line = "\t".join([name[:-1].decode(), str(flag), rname, str(pos + 1), str(mapq), cigar, rnext, str(npos + 1), str(tlen), seq, qual] + aux)
        records.append(dict(line=line, tid=tid, pos=pos, end=end, flag=flag, bin=bin_, n_cigar_op=n_cig, n_ops=len(cig), u0=u0, u1=at))
    assert at == len(stream)
    return text, refs, records


def sort_key(tid, pos, flag, n_refs):
    return (n_refs if tid < 0 else tid, pos + 1, (flag >> 4) & 1)


def stable_order(tid, pos, flag):
    n_refs = max([t for t in tid] + [-1]) + 1
    return sorted(range(len(tid)), key=lambda i: sort_key(int(tid[i]), int(pos[i]), int(flag[i]), n_refs))


def record_bin(r):
    if r["tid"] < 0:
        return 4680
    beg = max(r["pos"], 0)
    return reg2bin(beg, max(r["end"], beg + 1))


# ---------------------------------------------------------------- BAI
def expected_index(records, ref_len):
    """The index tables from the decoded records of a sorted file, by the rules of the header: (bins per reference: {bin: [(beg, end)]},
    linear per reference, meta per reference or None, n_no_coor)."""
    n_refs = len(ref_len)
    bins = [dict() for _ in range(n_refs)]
    linear = [[NONE] * (((ln - 1) >> 14) + 1) for ln in ref_len]
    meta = [None] * n_refs
    no_coor = 0
    prev = None
    for r in records:
        v0, v1 = voffset(r["u0"]), voffset(r["u1"])
        key = (r["tid"], record_bin(r))
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
    for k in range(n_refs):
        lin = linear[k]
        while lin and lin[-1] == NONE:
            lin.pop()
        for w in range(len(lin) - 2, -1, -1):
            if lin[w] == NONE:
                lin[w] = lin[w + 1]
    return bins, linear, meta, no_coor


def bai_bytes(bins, linear, meta, no_coor):
    out = [b"BAI\1", struct.pack("<i", len(bins))]
    for k in range(len(bins)):
        out.append(struct.pack("<i", len(bins[k]) + (1 if meta[k] else 0)))
        for b in sorted(bins[k]):
            out.append(struct.pack("<Ii", b, len(bins[k][b])))
            out.extend(struct.pack("<QQ", *c) for c in bins[k][b])
        if meta[k]:
            out.append(struct.pack("<IiQQQQ", 37450, 2, *meta[k]))
        out.append(struct.pack("<i", len(linear[k])))
        out.extend(struct.pack("<Q", v) for v in linear[k])
    out.append(struct.pack("<Q", no_coor))
    return b"".join(out)


def bai_parse(data):
    """-> (per reference ({bin: [(beg, end)]}, [ioffset]), n_no_coor); the pseudo-bin stays in the dict under 37450."""
    assert data[:4] == b"BAI\1"
    n_ref = struct.unpack_from("<i", data, 4)[0]
    at, refs = 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<i", data, at)[0]
        at += 4
        bins = {}
        for _ in range(n_bin):
            b, n_chunk = struct.unpack_from("<Ii", data, at)
            at += 8
            assert b not in bins
            bins[b] = [struct.unpack_from("<QQ", data, at + 16 * c) for c in range(n_chunk)]
            at += 16 * n_chunk
        n_intv = struct.unpack_from("<i", data, at)[0]
        at += 4
        refs.append((bins, list(struct.unpack_from("<%dQ" % n_intv, data, at))))
        at += 8 * n_intv
    no_coor = struct.unpack_from("<Q", data, at)[0] if at < len(data) else 0
    assert at + 8 == len(data)
    return refs, no_coor


def bai_query(index, records, tid, beg, end):
    """The records overlapping [beg, end) of reference tid that a reader finds THROUGH the index: the chunks of reg2bins, cut by the
    linear index's lower bound, then every record whose virtual offset lies in a chunk, filtered by overlap (a reader's last step)."""
    bins, linear = index[tid]
    low = 0
    if linear:
        w = beg >> 14
        low = linear[w] if w < len(linear) else NONE   # beyond the last window that has a record nothing can overlap
    chunks = [c for b in reg2bins(beg, end) if b in bins for c in bins[b] if c[1] > low]
    found = []
    for i, r in enumerate(records):
        v0 = voffset(r["u0"])
        if r["tid"] == tid and any(c[0] <= v0 < c[1] for c in chunks):
            rb = max(r["pos"], 0)
            if rb < end and max(r["end"], rb + 1) > beg:
                found.append(i)
    return found


def records_of_tid(records):
    """-> {tid: [place of every record of that tid, ascending]}: what bai_query_tid scans instead of the whole file"""
    out = {}
    for i, r in enumerate(records):
        out.setdefault(r["tid"], []).append(i)
    return out


def bai_query_tid(index, records, of_tid, tid, beg, end, vo=voffset):
    """bai_query for a file of many records and references: only the records of `tid` are looked at (of_tid = records_of_tid(records)),
    and a record's chunk is found by bisection -- the chunks of one reference are disjoint, every record lying in one run of one bin.
    vo: stream offset -> virtual offset (the closed form of the stored writer by default)."""
    bins, linear = index[tid]
    low = 0
    if linear:
        w = beg >> 14
        low = linear[w] if w < len(linear) else NONE
    chunks = sorted(c for b in reg2bins(beg, end) if b in bins for c in bins[b] if c[1] > low)
    assert all(a[1] <= b[0] for a, b in zip(chunks, chunks[1:])), "chunks of one reference overlap"
    begs = [c[0] for c in chunks]
    found = []
    for i in of_tid.get(tid, []):
        r = records[i]
        v0 = vo(r["u0"])
        k = bisect.bisect_right(begs, v0) - 1
        if k >= 0 and v0 < chunks[k][1]:
            rb = max(r["pos"], 0)
            if rb < end and max(r["end"], rb + 1) > beg:
                found.append(i)
    return found


def brute_overlaps(records, tid, beg, end):
    return [i for i, r in enumerate(records) if r["tid"] == tid and max(r["pos"], 0) < end and max(r["end"], max(r["pos"], 0) + 1) > beg]


# ---------------------------------------------------------------- 2bit
def twobit_decode(data):
    """-> [(name, sequence)] with N blocks and lower-case mask blocks applied."""
    sig, version, count, reserved = struct.unpack_from("<IIII", data, 0)
    assert sig == 0x1A412743 and version == 0 and reserved == 0
    at, index = 16, []
    for _ in range(count):
        ln = data[at]
        index.append((data[at + 1:at + 1 + ln].decode(), struct.unpack_from("<I", data, at + 1 + ln)[0]))
        at += 5 + ln
    out = []
    for k, (name, off) in enumerate(index):
        assert off == at, "records follow the index back to back"
        size, n_n = struct.unpack_from("<II", data, at)
        at += 8
        n_starts = struct.unpack_from("<%dI" % n_n, data, at)
        n_sizes = struct.unpack_from("<%dI" % n_n, data, at + 4 * n_n)
        at += 8 * n_n
        n_m = struct.unpack_from("<I", data, at)[0]
        at += 4
        m_starts = struct.unpack_from("<%dI" % n_m, data, at)
        m_sizes = struct.unpack_from("<%dI" % n_m, data, at + 4 * n_m)
        at += 8 * n_m
        assert struct.unpack_from("<I", data, at)[0] == 0
        at += 4
        packed = np.frombuffer(data[at:at + (size + 3) // 4], dtype=np.uint8)
        at += (size + 3) // 4
        two = np.stack([packed >> 6, (packed >> 4) & 3, (packed >> 2) & 3, packed & 3], axis=1).reshape(-1)
        assert not two[size:].any(), "the last byte is filled with T"
        seq = np.frombuffer(b"TCAG", dtype=np.uint8)[two[:size]].copy()
        for s, z in zip(n_starts, n_sizes):
            assert z > 0 and not two[s:s + z].any()
            seq[s:s + z] = ord("N")
        for s, z in zip(m_starts, m_sizes):
            assert z > 0
            seq[s:s + z] |= 0x20
        out.append((name, seq.tobytes().decode()))
    assert at == len(data)
    return out

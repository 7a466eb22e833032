"""The rules of npr_pileup_add_bam (include/nprealign.h) restated in plain Python / numpy, one record, one cigar run at a time, on the
stream tests/bam_reference.py decodes (bam_decode reads the header here; the records are walked again because the rules need the raw
cigar words and auxiliary bytes, malformed ones included, which bam_decode turns to text or refuses).  With it a minimal BAM record and
BGZF encoder for the constructed cases (tests/bam_pileup_cases.py): Python's zlib compresses the blocks, so the files are another
writer's.  Imports nothing from the product."""
import struct
import zlib

import numpy as np

import bam_reference as ref

SKIP, ADD, REFUSED = 0, 1, 2
WHY = ("none", "parts", "aux", "op", "pos", "ref", "read")
FLAG_MASK = 0x4 | 0x100 | 0x200 | 0x400
REF_OPS, READ_OPS, COLUMN_OPS = (0, 2, 3, 7, 8), (0, 1, 4, 7, 8), (0, 7, 8)
WIDTH = {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}


# ---------------------------------------------------------------- the encoder
def cigar_words(text):
    """'5M2I' -> [5 << 4 | 0, 2 << 4 | 1]"""
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(int(n) << 4 | ref.OPS.index(ch))
            n = ""
    assert n == ""
    return out


def consumed(words, ops):
    return sum(w >> 4 for w in words if (w & 15) in ops)


def pack_seq(nibbles):
    nib = list(nibbles) + [0] * (len(nibbles) & 1)
    return bytes(nib[k] << 4 | nib[k + 1] for k in range(0, len(nib), 2))


def record(name, flag, tid, pos, words, nibbles, aux=b"", l_seq=None, mapq=30, bin=0, next_tid=-1, next_pos=-1, tlen=0, qual=None):
    """One BAM record.  l_seq: what the record says (default: the nibbles given); qual: the quality bytes as they are stored (default: 0xFF per
    nibble given, "no qualities").  With an odd l_seq and one nibble more given, that nibble lands in the unused low half of the last byte."""
    name = name.encode() + b"\0"
    l_seq = len(nibbles) if l_seq is None else l_seq
    qual = b"\xff" * len(nibbles) if qual is None else bytes(qual)
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(name), mapq, bin, len(words), flag, l_seq, next_tid, next_pos, tlen) + name
    body += struct.pack("<%dI" % len(words), *words) + pack_seq(nibbles) + qual + aux
    return struct.pack("<i", len(body)) + body


def cg_record(name, flag, tid, pos, words, nibbles, aux_before=b"", aux_after=b"", with_cg=True, **kw):
    """The record of a long cigar: <l_seq>S<n>N stored, the operations in a CG:B:I field between the other auxiliary bytes.  kw: record()'s."""
    stored = [len(nibbles) << 4 | 4, consumed(words, REF_OPS) << 4 | 3]
    cg = b"CGBI" + struct.pack("<I%dI" % len(words), len(words), *words) if with_cg else b""
    return record(name, flag, tid, pos, stored, nibbles, aux=aux_before + cg + aux_after, **kw)


def header(refs, text=None):
    text = ("@HD\tVN:1.6\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs) if text is None else text).encode()
    out = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
    for name, ln in refs:
        out += struct.pack("<i", len(name) + 1) + name.encode() + b"\0" + struct.pack("<i", ln)
    return out


def bgzf(stream, member=65280, level=6):
    """The stream as BGZF members of `member` payload bytes, each compressed by zlib (raw deflate) at `level`, and the end-of-file block."""
    out = []
    for at in range(0, len(stream), member):
        payload = stream[at:at + member]
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        data = z.compress(payload) + z.flush()
        assert len(data) + 26 <= 65536
        out.append(bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0]) + struct.pack("<H", len(data) + 25) + data +
                   struct.pack("<II", zlib.crc32(payload), len(payload)))
    return b"".join(out) + ref.EOF_BLOCK


# ---------------------------------------------------------------- the rules
def header_end(stream):
    l_text = struct.unpack_from("<i", stream, 4)[0]
    at = 8 + l_text
    n_ref = struct.unpack_from("<i", stream, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 8 + struct.unpack_from("<i", stream, at)[0]
    return at


def split(stream):
    """-> ([(name, length)], [the bytes of every record, block_size included])"""
    end = header_end(stream)
    _, refs, none = ref.bam_decode(stream[:end])
    assert none == []
    records, at = [], end
    while at < len(stream):
        size = struct.unpack_from("<i", stream, at)[0]
        assert size >= 33 and at + 4 + size <= len(stream)
        records.append(stream[at:at + 4 + size])
        at += 4 + size
    return refs, records


def aux_walk(b):
    """The auxiliary bytes of a record -> (well-formed, the words of the first CG:B:I field or None)"""
    at, cg = 0, None
    while at < len(b):
        if len(b) - at < 3:
            return False, None
        tag, t = b[at:at + 2], chr(b[at + 2])
        at += 3
        if t == "A":
            need = 1
        elif t in WIDTH:
            need = WIDTH[t]
        elif t in "ZH":
            nul = b.find(b"\0", at)
            if nul < 0:
                return False, None
            need = nul + 1 - at
        elif t == "B":
            if len(b) - at < 5 or chr(b[at]) not in WIDTH:
                return False, None
            sub, count = chr(b[at]), struct.unpack_from("<I", b, at + 1)[0]
            need = 5 + WIDTH[sub] * count
            if need <= len(b) - at and cg is None and tag == b"CG" and sub == "I":
                cg = list(struct.unpack_from("<%dI" % count, b, at + 5))
        else:
            return False, None
        if need > len(b) - at:
            return False, None
        at += need
    return True, cg


def check(rec, ref_len, flag_mask=FLAG_MASK):
    """One record (its bytes, block_size included) -> dict(verdict, why, from_cg, words, ref_sum, read_sum, tid, pos, nibbles)."""
    size, tid, pos, l_name, mapq, bin_, n_cig, flag, l_seq, ntid, npos, tlen = struct.unpack_from("<iiiBBHHHiiii", rec, 0)
    out = dict(verdict=REFUSED, why="parts", from_cg=0, words=[], ref_sum=0, read_sum=0, tid=tid, pos=pos, nibbles=None)
    if size < 32 or 4 + size > len(rec) or l_name < 1 or l_seq < 0 or 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq > size or tid >= len(ref_len):
        return out
    out.update(verdict=SKIP, why="none")
    if tid < 0 or flag & flag_mask or l_seq <= 0 or n_cig == 0:
        return out
    at = 36 + l_name
    words = list(struct.unpack_from("<%dI" % n_cig, rec, at))
    at += 4 * n_cig
    packed = np.frombuffer(rec[at:at + (l_seq + 1) // 2], dtype=np.uint8)
    out["nibbles"] = np.stack([packed >> 4, packed & 15], axis=1).reshape(-1)[:l_seq]
    at += (l_seq + 1) // 2 + l_seq
    if n_cig == 2 and words[0] == (l_seq << 4 | 4) and words[1] & 15 == 3:
        fine, cg = aux_walk(rec[at:4 + size])
        if not fine:
            out.update(verdict=REFUSED, why="aux")
            return out
        if cg is not None:
            words = cg
            out["from_cg"] = 1
    out["words"] = words
    if not words:
        return out
    out["ref_sum"], out["read_sum"] = consumed(words, REF_OPS), consumed(words, READ_OPS)
    out["verdict"] = REFUSED
    if any(w & 15 > 8 for w in words):
        out["why"] = "op"
    elif pos < 0:
        out["why"] = "pos"
    elif pos + out["ref_sum"] > ref_len[tid]:
        out["why"] = "ref"
    elif out["read_sum"] != l_seq:
        out["why"] = "read"
    else:
        out["verdict"] = ADD
    return out


CODE = np.full(16, 4, dtype=np.int64)
CODE[[1, 2, 4, 8]] = [0, 1, 2, 3]


def add(table, base, v):
    """The columns of one record with the verdict ADD into table[T, 8]; base: the first row of its reference sequence."""
    x, y, last_col, ins_since, started = v["pos"], 0, None, False, False
    for w in v["words"]:
        ln, op = w >> 4, w & 15
        if ln == 0:
            continue
        if op in COLUMN_OPS or op == 2:
            if not started:
                table[base + x, 7] += 1
                started = True
            if op == 2:
                table[base + x:base + x + ln, 5] += 1
            else:
                np.add.at(table, (base + x + np.arange(ln), CODE[v["nibbles"][y:y + ln]]), 1)
                y += ln
            x += ln
            last_col, ins_since = x - 1, False
        elif op == 1:
            if last_col is not None and not ins_since:
                table[base + last_col, 6] += 1
            ins_since = True
            y += ln
        elif op == 3:
            x += ln
        elif op == 4:
            y += ln


def pileup(stream, flag_mask=FLAG_MASK, table=None):
    """-> (table int32 [sum l_ref, 8], {"records", "selected", "added", "refused"}, [check() of every record])"""
    refs, records = split(stream)
    ref_len = [ln for _, ln in refs]
    base = np.concatenate([[0], np.cumsum(ref_len)]).astype(np.int64)
    table = np.zeros((int(base[-1]), 8), dtype=np.int32) if table is None else table
    verdicts = [check(r, ref_len, flag_mask) for r in records]
    for v in verdicts:
        if v["verdict"] == ADD:
            add(table, int(base[v["tid"]]), v)
    n_add, n_ref = sum(v["verdict"] == ADD for v in verdicts), sum(v["verdict"] == REFUSED for v in verdicts)
    return table, dict(records=len(records), selected=n_add + n_ref, added=n_add, refused=n_ref), verdicts

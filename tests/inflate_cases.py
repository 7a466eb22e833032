"""The cases of the inflate tests (tests/test_inflate_host.py on the host, tests/test_gpu_bgzf_inflate.py on the device): payloads, the ways
zlib compresses them, deflate data written bit by bit that must be refused -- one case for every refusal csrc/npr_inflate.h lists --, and
BGZF blocks around either.  Imports nothing from the product."""
import struct
import zlib

import numpy as np

import bgzf_deflate_reference as dref

STATUS = ("OK", "BTYPE", "STORED_LEN", "OVERSUBSCRIBED", "INCOMPLETE", "REPEAT", "NO_EOB", "SYMBOL", "DISTANCE", "OUTPUT", "INPUT", "TRAILING",
          "ISIZE", "CRC", "BOUND")
MAX_BODY = 65536 - 26   # deflate bytes a BGZF block can hold: BSIZE is a uint16


def payloads():
    from test_gpu_bgzf_deflate import _bam_like
    rng = np.random.default_rng(1951)
    out = {"zeros %d" % n: bytes(n) for n in (0, 1, 2, 257, 258, 259, 65279, 65280, 65536)}
    out["one byte"] = b"\xa7" * 65536
    out["four values"] = (rng.integers(0, 4, 65536).astype(np.uint8) * 17).tobytes()
    out["random"] = rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()
    half = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    out["distance 32768"] = half + half
    out["bam-like"] = _bam_like(65536).tobytes()
    return out


def _deflate(payload, level=6, mem=9, strategy=zlib.Z_DEFAULT_STRATEGY, sync_at=None):
    z = zlib.compressobj(level, zlib.DEFLATED, -15, mem, strategy)
    if sync_at is None:
        return z.compress(payload) + z.flush()
    return z.compress(payload[:sync_at]) + z.flush(zlib.Z_SYNC_FLUSH) + z.compress(payload[sync_at:]) + z.flush()


WAYS = {
    "level 0": lambda p: _deflate(p, 0), "level 1": lambda p: _deflate(p, 1), "level 6": lambda p: _deflate(p, 6), "level 9": lambda p: _deflate(p, 9),
    "fixed": lambda p: _deflate(p, strategy=zlib.Z_FIXED), "huffman only": lambda p: _deflate(p, strategy=zlib.Z_HUFFMAN_ONLY),
    "rle": lambda p: _deflate(p, strategy=zlib.Z_RLE),
    "memLevel 1": lambda p: _deflate(p, mem=1),                      # many deflate blocks, switching at arbitrary bit positions
    "sync flush": lambda p: _deflate(p, sync_at=len(p) // 2 + 1),    # an empty stored block after an unaligned position
}


class Bits(object):
    """Deflate's bit order: everything from the least significant bit, a Huffman code from its most significant."""

    def __init__(self):
        self.bits = []

    def put(self, value, n):
        self.bits += [(value >> k) & 1 for k in range(n)]
        return self

    def code(self, value, n):
        self.bits += [(value >> k) & 1 for k in range(n - 1, -1, -1)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def bytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(v << k for k, v in enumerate(b[at:at + 8])) for at in range(0, len(b), 8))


def canonical(lens):
    """{symbol: (code, length)} of RFC 1951 3.2.2."""
    code, out = 0, {}
    for n in range(1, 16):
        for s in sorted(k for k, v in lens.items() if v == n):
            out[s] = (code, n)
            code += 1
        code <<= 1
    return out


CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
# a complete code-length code: the lengths 0 .. 4 one by one and the three repeat symbols, 3 bits each
CL_LENS = {0: 3, 1: 3, 2: 3, 3: 3, 4: 3, 16: 3, 17: 3, 18: 3}


def dynamic(final, hlit, hdist, cl_lens, sent):
    """The header of a dynamic block: `sent` = the code-length symbols as (symbol,) or (16 | 17 | 18, extra value)."""
    w = Bits().put(final, 1).put(2, 2).put(hlit - 257, 5).put(hdist - 1, 5).put(19 - 4, 4)
    for s in CL_ORDER:
        w.put(cl_lens.get(s, 0), 3)
    cl = canonical(cl_lens)
    for item in sent:
        w.code(*cl[item[0]])
        if item[0] >= 16:
            w.put(item[1], {16: 2, 17: 3, 18: 7}[item[0]])
    return w


def _lengths(ll, d, hlit, hdist):
    """ll and d ({symbol: length}) one by one, zeros in runs of symbol 18 / 17 where they are long enough."""
    seq = [ll.get(s, 0) for s in range(hlit)] + [d.get(s, 0) for s in range(hdist)]
    sent, at = [], 0
    while at < len(seq):
        run = 0
        while at + run < len(seq) and seq[at + run] == 0:
            run += 1
        if run >= 11:
            run = min(run, 138)
            sent.append((18, run - 11))
        elif run >= 3:
            sent.append((17, run - 3))
        else:
            run = 1
            sent.append((seq[at],))
        at += run
    return sent


def dynamic_block(ll, d, symbols, final=1, hlit=None, hdist=None):
    """A whole dynamic block: the codes ll and d, then `symbols` = ("l", literal/length symbol) | ("d", distance symbol) | ("x", value, bits)."""
    hlit = max(257, max(ll) + 1) if hlit is None else hlit
    hdist = max(1, max(d) + 1 if d else 1) if hdist is None else hdist
    w = dynamic(final, hlit, hdist, CL_LENS, _lengths(ll, d, hlit, hdist))
    cl, cd = canonical(ll), canonical(d)
    for item in symbols:
        if item[0] == "l":
            w.code(*cl[item[1]])
        elif item[0] == "d":
            w.code(*cd[item[1]])
        else:
            w.put(item[1], item[2])
    return w


def fixed_code(sym):
    if sym < 144:
        return 0x30 + sym, 8
    if sym < 256:
        return 0x190 + sym - 144, 9
    if sym < 280:
        return sym - 256, 7
    return 0xc0 + sym - 280, 8


def handmade():
    """Deflate data zlib never writes and accepts: name -> (body, payload)."""
    out = {}
    # one distance code of one bit (an incomplete code zlib's inflate_table lets pass): 'a', a match of 3 at distance 1, the end
    out["one distance code"] = (dynamic_block({97: 1, 256: 2, 257: 2}, {0: 1}, [("l", 97), ("l", 257), ("d", 0), ("l", 256)]).bytes(), b"aaaa")
    # no distance code at all, and none needed
    out["no distance code"] = (dynamic_block({97: 1, 256: 1}, {}, [("l", 97), ("l", 97), ("l", 256)]).bytes(), b"aa")
    # one literal/length code of one bit: the end of block alone
    out["one length code"] = (dynamic_block({256: 1}, {}, [("l", 256)]).bytes(), b"")
    # lengths sent with symbol 16 across the border of the two alphabets: literal 255, then symbol 256 and distances 0 and 1 as its repeats
    w = dynamic(1, 257, 2, CL_LENS, [(18, 127), (18, 117 - 11), (1,), (16, 0)])
    c = canonical({255: 1, 256: 1})
    w.code(*c[255]).code(*c[256])
    out["repeat across alphabets"] = (w.bytes(), b"\xff")
    # a match that overlaps its own output, of the largest length, in a fixed block; then a non-final empty fixed block before it
    w = Bits().put(0, 1).put(1, 2).code(*fixed_code(256)).put(1, 1).put(1, 2).code(*fixed_code(120)).code(*fixed_code(285)).code(0, 5).code(*fixed_code(256))
    out["fixed, length 258"] = (w.bytes(), b"x" * 259)
    # the farthest distance, 32 768 (zlib's own matches end 262 short of it): 32 768 random literals, then the same bytes as matches
    half = np.random.default_rng(32768).integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = Bits().put(1, 1).put(1, 2)
    for c in half:
        w.code(*fixed_code(c))
    for length in [258] * 126 + [130, 130]:
        sym, extra, bits = length_symbol(length)
        w.code(*fixed_code(sym)).put(extra, bits).code(29, 5).put(8191, 13)
    out["distance 32768 by hand"] = (w.code(*fixed_code(256)).bytes(), half + half)
    return out


def length_symbol(length):
    """(symbol, extra value, extra bits) of a match length 3 .. 258 (RFC 1951 3.2.5)."""
    if length == 258:
        return 285, 0, 0
    if length < 11:
        return 254 + length, 0, 0
    bits = (length - 3).bit_length() - 3
    return 261 + 4 * bits + (((length - 3) >> bits) & 3), (length - 3) & ((1 << bits) - 1), bits


def refusals():
    """name -> (body, isize, crc, the status expected).  Each is checked against zlib by the host test before anything of ours sees it."""
    good = _deflate(b"0123456789" * 3)
    crc = zlib.crc32(b"0123456789" * 3)
    out = {}
    out["BTYPE 3"] = (Bits().put(1, 1).put(3, 2).align().put(0, 32).bytes(), 0, 0, "BTYPE")
    out["LEN != ~NLEN"] = (Bits().put(1, 1).put(0, 2).align().put(3, 16).put(0xfffd, 16).bytes() + b"abc", 3, zlib.crc32(b"abc"), "STORED_LEN")
    # four code-length codes of one bit
    w = Bits().put(1, 1).put(2, 2).put(0, 5).put(0, 5).put(0, 4)
    for _ in range(4):
        w.put(1, 3)
    out["over-subscribed"] = (w.put(0, 64).bytes(), 0, 0, "OVERSUBSCRIBED")
    out["over-subscribed literals"] = (dynamic_block({0: 1, 1: 1, 256: 1}, {}, []).put(0, 64).bytes(), 0, 0, "OVERSUBSCRIBED")
    out["incomplete literals"] = (dynamic_block({0: 2, 256: 2}, {}, [("l", 256)]).bytes(), 0, 0, "INCOMPLETE")
    out["incomplete distances"] = (dynamic_block({0: 1, 256: 1}, {0: 2, 1: 2}, [("l", 256)]).bytes(), 0, 0, "INCOMPLETE")
    out["incomplete code-length code"] = (dynamic(1, 257, 1, {0: 1}, []).put(0, 400).bytes(), 0, 0, "INCOMPLETE")
    out["repeat with no length before"] = (dynamic(1, 257, 1, CL_LENS, [(16, 0)]).put(0, 64).bytes(), 0, 0, "REPEAT")
    out["repeat past HLIT + HDIST"] = (dynamic(1, 257, 1, CL_LENS, [(18, 127), (18, 118 - 11), (17, 0)]).put(0, 64).bytes(), 0, 0, "REPEAT")
    out["no symbol 256"] = (dynamic_block({0: 1, 1: 1}, {}, []).put(0, 64).bytes(), 0, 0, "NO_EOB")
    out["literal/length symbol 286"] = (Bits().put(1, 1).put(1, 2).code(*fixed_code(97)).code(*fixed_code(286)).code(0, 5).code(*fixed_code(256)).bytes(), 4, 0, "SYMBOL")
    out["distance symbol 30"] = (Bits().put(1, 1).put(1, 2).code(*fixed_code(97)).code(*fixed_code(257)).code(30, 5).code(*fixed_code(256)).bytes(), 4, 0, "SYMBOL")
    out["HLIT 287"] = (Bits().put(1, 1).put(2, 2).put(30, 5).put(0, 5).put(15, 4).put(0, 400).bytes(), 0, 0, "SYMBOL")
    out["bits that are no code"] = (dynamic_block({256: 1}, {}, []).put(1, 1).put(0, 32).bytes(), 0, 0, "SYMBOL")
    out["a match without a distance code"] = (dynamic_block({97: 2, 256: 2, 257: 1}, {}, [("l", 97), ("l", 257)]).put(0, 16).bytes(), 4, 0, "SYMBOL")
    out["distance before the first byte"] = (Bits().put(1, 1).put(1, 2).code(*fixed_code(257)).code(0, 5).code(*fixed_code(256)).bytes(), 3, zlib.crc32(b"aaa"), "DISTANCE")
    out["distance one too far"] = (Bits().put(1, 1).put(1, 2).code(*fixed_code(97)).code(*fixed_code(257)).code(1, 5).code(*fixed_code(256)).bytes(), 4, 0, "DISTANCE")
    out["output past ISIZE"] = (good, 29, crc, "OUTPUT")
    out["a match past ISIZE"] = (_deflate(bytes(300)), 299, zlib.crc32(bytes(299)), "OUTPUT")
    out["a stored block past ISIZE"] = (_deflate(b"abcdef", 0), 5, 0, "OUTPUT")
    out["input past n"] = (good[:-3], 30, crc, "INPUT")
    out["a stored block past n"] = (_deflate(b"abcdef", 0)[:-1], 6, zlib.crc32(b"abcdef"), "INPUT")
    out["no input"] = (b"", 0, 0, "INPUT")
    out["trailing bytes"] = (good + b"\0", 30, crc, "TRAILING")
    out["produced != ISIZE"] = (good, 31, crc, "ISIZE")
    out["CRC"] = (good, 30, crc ^ 1, "CRC")
    return out


def zlib_accepts(body, isize, crc):
    """Whether a fresh raw inflater ends exactly on `body` with isize bytes of that CRC-32."""
    z = zlib.decompressobj(-15)
    try:
        got = z.decompress(body)
    except zlib.error:
        return False
    return z.eof and z.unused_data == b"" and len(got) == isize and zlib.crc32(got) == crc


def block(body, isize, crc, extra=b""):
    """One BGZF block around deflate data; `extra`: subfields put before BC."""
    xlen = 6 + len(extra)
    head = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff]) + struct.pack("<H", xlen) + extra + b"BC" + struct.pack("<HH", 2, 12 + xlen + len(body) + 8 - 1)
    return head + body + struct.pack("<II", crc & 0xffffffff, isize)


def accepted():
    """[(name, body, payload)]: every payload every way, and the hand-made ones."""
    out = [("%s, %s" % (kind, way), fn(p), p) for kind, p in payloads().items() for way, fn in WAYS.items()]
    return out + [(name, body, p) for name, (body, p) in handmade().items()]


EOF_BLOCK = dref.EOF_BLOCK

"""npr_bgzf_scan (csrc/npr_bam_host.cpp), the host side of the BGZF reader: the block table of good files against the Python reader's,
and the files it must refuse -- a cut file, a missing end-of-file block, a BSIZE off by one -- and accept: a BC subfield that stands
second among the extra subfields, blocks of ISIZE 0.  No GPU."""
import ctypes as C
import gzip
import struct
import zlib

import numpy as np
import pytest

import bgzf_deflate_reference as dref
import inflate_cases as cases
from nanopore_amd import _lib, bam


def _file(parts, level=6, extra=b""):
    return b"".join(cases.block(cases.WAYS["level %d" % level](p), len(p), zlib.crc32(p), extra) for p in parts) + cases.EOF_BLOCK


def _parts(n):
    rng = np.random.default_rng(n)
    stream = (rng.integers(0, 4, n).astype(np.uint8) * 17).tobytes()
    return [stream[at:at + dref.P] for at in range(0, n, dref.P)]


@pytest.mark.parametrize("n", (0, 1, 65280, 65281, 3 * 65280 + 17))
def test_the_block_table_is_the_python_readers(n):
    parts = _parts(n)
    data = _file(parts)
    stream, blocks = dref.bgzf_read(data)
    block_off, stream_off = bam.bgzf_scan(data)
    assert block_off.tolist() == [b[0] for b in blocks] + [len(data) - 28]
    assert stream_off.tolist() == [b[1] for b in blocks] + [len(stream)]
    # the count alone, the capacity, and no write past it
    L, count = _lib.load(), C.c_int64(-1)
    arr = np.frombuffer(data, np.uint8)
    assert L.npr_bgzf_scan(_lib.ptr(arr), len(arr), None, None, 0, C.byref(count)) == n and count.value == len(parts)
    short = np.full(len(parts) + 2, -7, np.int64)
    assert L.npr_bgzf_scan(_lib.ptr(arr), len(arr), _lib.ptr(short), None, len(parts), C.byref(count)) == _lib.ERR_CAPACITY
    assert (short[len(parts):] == -7).all()
    assert L.npr_bgzf_scan(_lib.ptr(arr), len(arr), _lib.ptr(short), None, len(parts) + 1, C.byref(count)) == n
    assert short[:-1].tolist() == block_off.tolist() and short[-1] == -7


def test_blocks_of_isize_0_and_a_bc_subfield_that_is_not_first():
    parts = [b"first", b"", b"third", b""]
    other = b"XY" + struct.pack("<H", 3) + b"abc"
    data = _file(parts, extra=other)
    assert data[12:14] == b"XY" and data[19:21] == b"BC"
    block_off, stream_off = bam.bgzf_scan(data)
    assert len(block_off) == 5 and stream_off.tolist() == [0, 5, 5, 10, 10]
    assert gzip.decompress(data) == b"firstthird"   # (a gzip reader takes the members as they are)
    # the end-of-file block in the middle is a block like any other
    data = _file([b"first"]) + _file([b"second"])
    block_off, stream_off = bam.bgzf_scan(data)
    assert len(block_off) == 4 and stream_off.tolist() == [0, 5, 5, 11]


def _tags_bytes(lines):
    """npr_bam_tags on SAM lines with 11 empty-ish mandatory columns: (tag_off, bytes)."""
    text = "".join("r\t0\t*\t0\t0\t*\t*\t0\t0\t*\t*" + ("\t" + t if t else "") + "\n" for t in lines).encode()
    arr = np.frombuffer(text, np.uint8)
    tail = np.zeros((len(lines), 8), np.int64)
    at = 0
    for i, t in enumerate(lines):
        end = text.index(b"\n", at)
        tail[i, 5], tail[i, 6], tail[i, 7] = (end - len(t) if t else end), end, 0
        at = end + 1
    return bam.bam_tags(arr, tail)


def test_aux_text_inverts_bam_tags():
    import bam_reference as ref
    from test_gpu_bam import TAGS
    lines = [TAGS, "", "RG:Z:g", "Xq:i:255\tXr:i:256\tXs:i:65536\tXt:i:-1\tXu:i:-129\tXv:i:-32769\tXw:i:4294967295", "Xf:f:1e+10\tXg:f:3.14159\tXh:f:-1e-05"]
    tag_off, raw = _tags_bytes(lines)
    text_off, text, cg = bam.bam_aux_text(raw, tag_off)
    assert (cg == -1).all()
    for i, t in enumerate(lines):
        got = text[text_off[i]:text_off[i + 1]].tobytes().decode()
        assert got == "\t".join(ref._aux_text(raw[tag_off[i]:tag_off[i + 1]].tobytes())), i   # the specification's reader
        if i != 4:
            assert got == t, i   # the text itself: every integer type prints as i, these floats as %g prints them
    assert text[text_off[4]:text_off[5]].tobytes() == b"Xf:f:1e+10\tXg:f:3.14159\tXh:f:-1e-05"
    # every integer type was met
    assert {chr(raw[tag_off[3] + 2 + k]) for k in (0,)} == {"C"} and set(b"CSIcsi") <= set(raw[tag_off[3]:tag_off[4]].tobytes())


def test_aux_text_folds_a_cg_field_only_under_a_placeholder():
    ops = [5 << 4 | 4, 7 << 4 | 0, 3 << 4 | 8]
    cgf = b"CGBI" + struct.pack("<I3I", 3, *ops)
    raw = np.frombuffer(b"NMC\x03" + cgf + b"XaAq" + b"NMC\x03" + cgf, np.uint8)
    off = np.array([0, 4 + len(cgf) + 4, len(raw)], np.int64)
    text_off, text, cg = bam.bam_aux_text(raw, off, placeholder=np.array([1, 0], np.uint8))
    assert text[:text_off[1]].tobytes() == b"NM:i:3\tXa:A:q" and cg[0].tolist() == [4 + 8, 3]
    assert text[text_off[1]:].tobytes() == b"NM:i:3\tCG:B:I,%d,%d,%d" % tuple(ops) and cg[1].tolist() == [-1, -1]
    bad = np.frombuffer(b"CGBI" + struct.pack("<II", 1, 9), np.uint8)   # an operation above 8
    with pytest.raises(_lib.NprError):
        bam.bam_aux_text(bad, np.array([0, len(bad)], np.int64), placeholder=np.array([1], np.uint8))


@pytest.mark.parametrize("raw", (b"NM", b"NMq\x01", b"XzZno nul", b"XhH1A", b"XbBc\x03\x00\x00\x00\x01\x02", b"XbBq\x00\x00\x00\x00", b"XbBc\x01\x00",
                                 b"NMi\x01\x02\x03", b"Xff\x00\x00", b"XaA", b"NMC\x03X"))
def test_aux_text_refuses_malformed_bytes(raw):
    arr = np.frombuffer(b"NMC\x03" + raw, np.uint8)
    with pytest.raises(_lib.NprError) as e:
        bam.bam_aux_text(arr, np.array([0, 4, len(arr)], np.int64))
    assert e.value.code == _lib.ERR_INVALID
    good = bam.bam_aux_text(arr[:4], np.array([0, 4], np.int64))
    assert good[1].tobytes() == b"NM:i:3"


def test_files_that_are_refused():
    good = _file(_parts(70000))
    assert len(bam.bgzf_scan(good)[0]) == 3
    first = struct.unpack("<H", good[16:18])[0] + 1

    def refused(data):
        with pytest.raises(_lib.NprError) as e:
            bam.bgzf_scan(data)
        return e.value.code == _lib.ERR_INVALID

    assert refused(good[:-28])                                   # no end-of-file block
    assert refused(good[:-1]) and refused(good[:100]) and refused(b"")   # cut
    assert refused(good[:first - 7] + good[first:])              # a block cut short: the chain misses the end-of-file block
    for delta in (-1, 1):                                        # BSIZE off by one
        bad = bytearray(good)
        bad[16:18] = struct.pack("<H", first - 1 + delta)
        assert refused(bytes(bad))
    bad = bytearray(good)
    bad[3] = 0                                                   # FLG without FEXTRA
    assert refused(bytes(bad))
    bad = bytearray(good)
    bad[12:14] = b"BX"                                           # no BC subfield
    assert refused(bytes(bad))
    bad = bytearray(good)
    bad[14:16] = struct.pack("<H", 3)                            # BC of a length that is not 2
    assert refused(bytes(bad))
    bad = bytearray(good)
    bad[first - 4:first] = struct.pack("<I", 65537)              # ISIZE above 65 536
    assert refused(bytes(bad))
    bad = bytearray(good)
    bad[10:12] = struct.pack("<H", 60000)                        # an extra field longer than the block
    assert refused(bytes(bad))

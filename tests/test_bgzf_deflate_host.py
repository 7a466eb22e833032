"""The compressed-BGZF reader of the tests (tests/bgzf_deflate_reference.py) on blocks made with zlib in Python -- it accepts them and
rejects four corruptions --, and the two entry points of the compressed writer in the library's export table.  No GPU."""
import struct
import zlib

import numpy as np
import pytest

import bgzf_deflate_reference as dref


def _block(payload, level=6, body=None):
    if body is None:
        z = zlib.compressobj(level, zlib.DEFLATED, -15, 9)   # (memLevel 9: the payloads here stay one deflate block)
        body = z.compress(payload) + z.flush()
    return dref.HEAD + struct.pack("<H", 18 + len(body) + 8 - 1) + body + struct.pack("<II", zlib.crc32(payload), len(payload))


def _file(stream, level=6):
    return b"".join(_block(stream[at:at + dref.P], level) for at in range(0, len(stream), dref.P)) + dref.EOF_BLOCK


def _stream(n):
    rng = np.random.default_rng(n)
    return (rng.integers(0, 4, n).astype(np.uint8) * 17).tobytes()


@pytest.mark.parametrize("n", (0, 1, 65279, 65280, 65281, 2 * 65280 + 17))
@pytest.mark.parametrize("level", (1, 6, 9))
def test_reader_accepts_blocks_made_with_zlib(n, level):
    stream = _stream(n)
    data = _file(stream, level)
    got, blocks = dref.bgzf_read(data)
    assert got == stream and len(blocks) == (n + dref.P - 1) // dref.P
    at = 0
    for k, (file_at, first, ln) in enumerate(blocks):
        assert file_at == at and first == k * dref.P
        at += struct.unpack("<H", data[at + 16:at + 18])[0] + 1
    for u in sorted({0, 1, dref.P - 1, dref.P, n - 1, n} & set(range(n + 1))):
        v = dref.voffset_by_walking(blocks, u, n, len(data))
        assert dref.voffset_to_stream(blocks, v, n, len(data)) == u
    if n and n % dref.P == 0:
        assert dref.voffset_by_walking(blocks, n, n, len(data)) == (len(data) - 28) << 16


def test_reader_rejects_corruptions():
    stream = _stream(70000)
    good = _file(stream)
    assert dref.bgzf_read(good)[0] == stream
    first = struct.unpack("<H", good[16:18])[0] + 1
    flipped = bytearray(good)
    flipped[first - 8] ^= 1                                   # the CRC of the first block
    with pytest.raises(AssertionError):
        dref.bgzf_read(bytes(flipped))
    bsize = bytearray(good)
    bsize[16:18] = struct.pack("<H", first - 2)               # BSIZE one too small
    with pytest.raises((AssertionError, zlib.error)):
        dref.bgzf_read(bytes(bsize))
    cut = _block(stream[:dref.P])
    cut = cut[:18] + cut[18:-8][:-3] + cut[-8:]               # deflate data cut short, BSIZE left as it was
    with pytest.raises((AssertionError, zlib.error)):
        dref.bgzf_read(cut + dref.EOF_BLOCK)
    cut = dref.HEAD + struct.pack("<H", len(cut) - 1) + cut[18:]   # ... and with a BSIZE that fits
    with pytest.raises((AssertionError, zlib.error)):
        dref.bgzf_read(cut + dref.EOF_BLOCK)
    # a fixed-Huffman block whose first token is a match of length 3 at distance 1: BFINAL 1, BTYPE 01, length code 257 (7 bits 0000001),
    # distance code 0 (5 bits 00000), end of block (7 bits 0000000); Huffman codes go in from their most significant bit
    bits = [1, 1, 0] + [0, 0, 0, 0, 0, 0, 1] + [0] * 5 + [0] * 7
    body = bytes(sum(b << k for k, b in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))
    with pytest.raises((AssertionError, zlib.error)):
        dref.bgzf_read(_block(b"aaa", body=body) + dref.EOF_BLOCK)
    # (the same tokens after a literal are a valid block: the rejection above is the match before the block's first byte)
    lit = [int(c) for c in format(0x30 + ord("a"), "08b")]
    bits = [1, 1, 0] + lit + [0, 0, 0, 0, 0, 0, 1] + [0] * 5 + [0] * 7
    body = bytes(sum(b << k for k, b in enumerate(bits[at:at + 8])) for at in range(0, len(bits), 8))
    assert dref.bgzf_read(_block(b"aaaa", body=body) + dref.EOF_BLOCK)[0] == b"aaaa"


def test_the_library_exports_the_compressed_writer():
    from nanopore_amd import _lib
    assert "npr_bgzf_deflate" in _lib.EXPORTS and "npr_sam_bam_deflate" in _lib.EXPORTS
    L = _lib.load()
    data = np.zeros(8, dtype=np.uint8)
    assert L.npr_bgzf_deflate(None, _lib.ptr(data), 8, None, 0, None) == _lib.ERR_INVALID
    args = [None, None, 0, None, None, None, 0, None, None, None, 0, 0, None, 0, None, 0, None] + [None] * 6 + [None]
    assert L.npr_sam_bam_deflate(*args) == _lib.ERR_INVALID

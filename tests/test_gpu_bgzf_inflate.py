"""npr_bgzf_inflate (csrc/npr_inflate.hip: one workgroup inflates one BGZF block with the decoder of csrc/npr_inflate.h) against zlib: the
accepted cases of tests/inflate_cases.py as the blocks of BGZF files, the device's own writers read back, blocks of random lengths, and every
refusal placed in block 1 of a three-block file.  The refusals are refusals of input, bounded by construction: tests/test_inflate_host.py
runs the same decoder on the same cases under AddressSanitizer."""
import zlib

import numpy as np
import pytest

import inflate_cases as cases

pytestmark = pytest.mark.gpu

P = 65280


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


def _file(items):
    """[(body, payload)] as one BGZF file."""
    return b"".join(cases.block(body, len(p), zlib.crc32(p)) for body, p in items) + cases.EOF_BLOCK


def test_every_accepted_case_gives_its_payload_back(ctx):
    from nanopore_amd import bam
    # (deflate data of more than 65 510 bytes -- 65 536 bytes that zlib stores or hardly shortens -- fits no BGZF block: BSIZE is a uint16.
    # Those cases, 14 of 132, are the host test's alone.)
    items = [(name, body, p) for name, body, p in cases.accepted() if len(body) <= cases.MAX_BODY]
    assert len(items) == 14 * 9 + 6 - 14 and {(body[0] >> 1) & 3 for _, body, _ in items} == {0, 1, 2}
    assert "distance 32768 by hand" in [name for name, _, _ in items]
    data = _file([(body, p) for _, body, p in items])
    want = b"".join(p for _, _, p in items)
    got = bam.bgzf_inflate(ctx, data)
    last = bam.inflate_last(ctx)
    assert last == {"blocks": len(items), "failed_block": -1, "status": 0, "reason": "ok", "stream_bytes": len(want)}
    if got.tobytes() != want:   # which case
        at = 0
        for name, _, p in items:
            assert got[at:at + len(p)].tobytes() == p, name
            at += len(p)
    assert got.tobytes() == want
    # one block at a time, a block of 65 536 bytes among them: the CRC beyond the writers' payload length, a stream offset that is not a multiple of four
    for name in ("zeros 65536, level 6", "bam-like, level 9", "one distance code", "zeros 1, level 0"):
        body, p = next((b, q) for n, b, q in items if n == name)
        data = _file([(cases.WAYS["level 6"](b"abc"), b"abc"), (body, p)])
        assert bam.bgzf_inflate(ctx, data).tobytes() == b"abc" + p, name


@pytest.mark.parametrize("n", (0, 1, P - 1, P, P + 1, 2 * P + 17))
def test_the_device_writers_read_back(ctx, n):
    from nanopore_amd import bam
    rng = np.random.default_rng(n)
    for kind, x in (("16 values", (rng.integers(0, 16, n) * 17).astype(np.uint8)), ("random", rng.integers(0, 256, n).astype(np.uint8)),
                    ("bam-like", np.frombuffer(cases.payloads()["bam-like"] * 3, np.uint8)[:n])):
        deflated, _ = bam.bgzf_deflate(ctx, x)
        assert bam.bgzf_inflate(ctx, deflated).tobytes() == x.tobytes(), kind
        assert bam.inflate_last(ctx)["blocks"] == (n + P - 1) // P
        assert bam.bgzf_inflate(ctx, bam.bgzf_frame(ctx, x)).tobytes() == x.tobytes(), kind


def test_blocks_of_random_lengths_and_an_empty_one(ctx):
    from nanopore_amd import bam
    rng = np.random.default_rng(4)
    lengths = [int(v) for v in rng.integers(1, 65281, 40)]
    lengths[20] = 0
    acgt = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], np.uint8)
    parts = [acgt[rng.integers(0, 16, n)].tobytes() if k % 3 else bytes(rng.integers(0, 256, n, dtype=np.uint8)) for k, n in enumerate(lengths)]
    ways = list(cases.WAYS.values())
    data = _file([(ways[k % len(ways)](p), p) for k, p in enumerate(parts)])
    block_off, stream_off = bam.bgzf_scan(data)
    assert len(block_off) == 41 and np.diff(stream_off).tolist() == lengths and block_off[-1] == len(data) - 28
    assert bam.bgzf_inflate(ctx, data).tobytes() == b"".join(parts)
    # more blocks than workgroups: a workgroup uses its LDS again
    small = [(cases.WAYS["level 1"](bytes([k & 0xff]) * (1 + k % 7)), bytes([k & 0xff]) * (1 + k % 7)) for k in range(2100)]
    assert bam.bgzf_inflate(ctx, _file(small)).tobytes() == b"".join(p for _, p in small)
    assert bam.inflate_last(ctx)["blocks"] == 2100


def test_every_refusal_in_block_1_of_three(ctx):
    from nanopore_amd import _lib, bam
    first, third = cases.payloads()["bam-like"][:30000], b"the third block"
    good = lambda p: cases.block(cases.WAYS["level 6"](p), len(p), zlib.crc32(p))
    for name, (body, isize, crc, want) in cases.refusals().items():
        data = np.frombuffer(good(first) + cases.block(body, isize, crc) + good(third) + cases.EOF_BLOCK, np.uint8)
        total = len(first) + isize + len(third)
        assert ctx._L.npr_bgzf_inflate(ctx._h, _lib.ptr(data), len(data), None, 0) == total, name
        out = np.full(total + 64, 0xa5, np.uint8)
        with pytest.raises(_lib.NprError) as e:
            bam.bgzf_inflate(ctx, data, out=out)
        assert e.value.code == _lib.ERR_INVALID and "block 1" in str(e.value), name
        last = bam.inflate_last(ctx)
        assert (last["blocks"], last["failed_block"], cases.STATUS[last["status"]]) == (3, 1, want), (name, last)
        assert (out == 0xa5).all(), name


def test_capacity_and_files_that_are_not_bgzf(ctx):
    from nanopore_amd import _lib, bam
    p = cases.payloads()["four values"]
    data = np.frombuffer(_file([(cases.WAYS["level 6"](p), p)]), np.uint8)
    out = np.full(len(p) + 8, 0xa5, np.uint8)
    assert ctx._L.npr_bgzf_inflate(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), len(p) - 1) == _lib.ERR_CAPACITY and (out == 0xa5).all()
    assert ctx._L.npr_bgzf_inflate(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), len(p)) == len(p)
    assert out[:len(p)].tobytes() == p and (out[len(p):] == 0xa5).all()
    for bad in (data[:-28], data[:-1], data[1:]):   # no end-of-file block, a cut one, a shifted file
        with pytest.raises(_lib.NprError):
            bam.bgzf_inflate(ctx, np.ascontiguousarray(bad))

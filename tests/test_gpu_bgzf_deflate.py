"""npr_bgzf_deflate (csrc/npr_deflate.hip) read back by tests/bgzf_deflate_reference.py: every block one final DEFLATE block that a
fresh inflater ends at the trailer, CRC-32, ISIZE, the block table against the reader's file offsets, the stored length as the upper
bound, the same bytes from two calls; and three sizes that follow from the format at a full block.

The periodic payloads: a period begins with 300 random bytes and is zeros from there on.  The zeros enter only one entry of the match
table, so the candidate of a position in the second period's random part is the same position of the first period: a match at distance
32 768 exactly, the farthest legal one, for the period 32 768, and one at 32 769, which must be refused, for the period 32 769."""
import numpy as np
import pytest

import bgzf_deflate_reference as dref

pytestmark = pytest.mark.gpu

P = dref.P
LENGTHS = (1, 2, 3, 258, 259, 65279, 65280, 65281, 2 * 65280 + 17)


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


def _periodic(n, period):
    one = np.zeros(period, np.uint8)
    one[:300] = np.random.default_rng(period).integers(1, 256, 300)
    return np.tile(one, n // period + 1)[:n]


def _bam_like(n):
    """8 kb records: fixed fields, a name, cigar words, packed ACGT, a run of 0xFF qualities."""
    rng = np.random.default_rng(5)
    out, k = [], 0
    while sum(len(o) for o in out) < n:
        l_seq = 8000 + 2 * int(rng.integers(0, 200))
        fixed = np.array([36 + 8 + 16 + l_seq // 2 + l_seq, 0, 1000 * k, 0x1e4908, 0x00000004, l_seq, 0xffffffff, 0xffffffff, 0], dtype=np.uint32)
        name = np.frombuffer(b"read%03d\0" % (k % 1000), dtype=np.uint8)
        cigar = (rng.integers(1, 60, 4).astype(np.uint32) << 4 | rng.integers(0, 3, 4).astype(np.uint32))
        nib = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, l_seq)]
        out += [fixed.view(np.uint8), name, cigar.view(np.uint8), nib[0::2] << 4 | nib[1::2], np.full(l_seq, 0xff, np.uint8)]
        k += 1
    return np.concatenate(out)[:n]


def _payloads(n):
    rng = np.random.default_rng(n)
    acgt = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], np.uint8)
    return {"zeros": np.zeros(n, np.uint8), "one value": np.full(n, 0xa7, np.uint8), "two values": rng.integers(0, 2, n).astype(np.uint8) * 0x5a,
            "16 values": acgt[rng.integers(0, 16, n)], "random": rng.integers(0, 256, n).astype(np.uint8),
            "counter": (np.arange(n) % 251).astype(np.uint8), "period 32768": _periodic(n, 32768), "period 32769": _periodic(n, 32769),
            "bam-like": _bam_like(n)}


@pytest.mark.parametrize("n", LENGTHS)
def test_every_block_reads_back(ctx, n):
    from nanopore_amd import bam
    for kind, data in _payloads(n).items():
        out, block_off = bam.bgzf_deflate(ctx, data)
        raw = out.tobytes()
        stream, blocks = dref.bgzf_read(raw)
        assert stream == data.tobytes(), kind
        assert len(blocks) == (n + P - 1) // P == len(block_off) - 1, kind
        assert [b[0] for b in blocks] + [len(raw) - 28] == block_off.tolist(), kind
        stored = n + 31 * len(blocks) + 28
        assert len(raw) <= stored, kind
        print("%-13s n %6d: %6d bytes of %6d stored, BTYPE %s" % (kind, n, len(raw), stored, dref.block_types(raw)))
        again, again_off = bam.bgzf_deflate(ctx, data)
        assert again.tobytes() == raw and again_off.tolist() == block_off.tolist(), kind
        for u in sorted({0, 1, P - 1, P, P + 1, n - 1, n} & set(range(n + 1))):
            v = dref.voffset_by_walking(blocks, u, n, len(raw))
            assert v == int(block_off[u // P]) << 16 | u % P, (kind, u)


def test_an_empty_stream_is_the_end_of_file_block(ctx):
    from nanopore_amd import bam
    out, block_off = bam.bgzf_deflate(ctx, np.zeros(0, np.uint8))
    assert out.tobytes() == dref.EOF_BLOCK and block_off.tolist() == [0]


def test_sizes_that_follow_from_the_format(ctx):
    from nanopore_amd import bam
    data = _payloads(P)
    size = {}
    for kind in ("random", "zeros", "16 values", "period 32768", "period 32769", "bam-like"):
        out, _ = bam.bgzf_deflate(ctx, data[kind])
        size[kind] = len(out) - 28
        print("%-13s %6d bytes" % (kind, size[kind]), dref.block_types(out.tobytes()))
    # uniform random bytes: the code header alone costs more than a Huffman code can save at that entropy, so stored wins
    assert size["random"] == P + 31
    # zeros: literals alone are at least a bit a byte (8 160 bytes); 253 matches of 258 are about 64 bytes and the code header
    assert size["zeros"] <= 1024
    # 16 values at random: four bits for fifteen literals, five for the rarest (at most P / 16 of them) and the end of block; the code
    # header is under 286 bytes
    assert size["16 values"] <= P * (4 + 1 / 16) / 8 + 512
    # a match at distance 32 768 is taken (the second period's 300 random bytes cost a few bytes), one at 32 769 is not (they cost
    # about 300 bytes more)
    assert size["period 32768"] + 200 < size["period 32769"]


def test_capacity_is_checked_and_nothing_written_past_it(ctx):
    from nanopore_amd import _lib
    data = _bam_like(70000)
    bound = 70000 + 2 * 31 + 28
    assert ctx._L.npr_bgzf_deflate(ctx._h, _lib.ptr(data), len(data), None, 0, None) == bound
    out = np.full(bound + 64, 0xa5, dtype=np.uint8)
    off = np.full(3, -7, dtype=np.int64)
    for cap in (0, 27, bound - 1):
        rc = ctx._L.npr_bgzf_deflate(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), cap, _lib.ptr(off))
        assert rc == _lib.ERR_CAPACITY and (out == 0xa5).all() and (off == -7).all()
    total = ctx._L.npr_bgzf_deflate(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), bound, _lib.ptr(off))
    assert 28 < total < bound and (out[total:] == 0xa5).all()
    assert dref.bgzf_read(out[:total].tobytes())[0] == data.tobytes() and off[2] == total - 28
    assert ctx._L.npr_bgzf_deflate(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), bound, None) == total


def test_more_blocks_than_workgroups_and_scan_tiles(ctx):
    """2 100 blocks: a workgroup takes every 512th block, so it uses its LDS and its distance scratch again four times, and the prefix sum
    of the block lengths spans two tiles of 2 048.  Most blocks are runs with a counter (cheap to make and to inflate); every 7th holds
    16 values at random and every 97th random bytes, so the three encodings and many block lengths occur."""
    from nanopore_amd import bam
    blocks, n = 2100, 2099 * P + 4321
    rng = np.random.default_rng(2100)
    data = np.full(blocks * P, 0xff, np.uint8).reshape(blocks, P)
    data[:, 0] = np.arange(blocks) & 0xff
    data[:, 1] = np.arange(blocks) >> 8
    acgt = np.array([a << 4 | b for a in (1, 2, 4, 8) for b in (1, 2, 4, 8)], np.uint8)
    data[::7, 100:] = acgt[rng.integers(0, 16, (len(data[::7]), P - 100))]
    data[::97] = rng.integers(0, 256, (len(data[::97]), P), dtype=np.uint8)
    data = data.reshape(-1)[:n]
    out, block_off = bam.bgzf_deflate(ctx, data)
    raw = out.tobytes()
    stream, found = dref.bgzf_read(raw)
    assert stream == data.tobytes() and len(found) == blocks
    assert [b[0] for b in found] + [len(raw) - 28] == block_off.tolist()
    last = bam.deflate_last(ctx)
    types = dref.block_types(raw)
    assert last["stream_bytes"] == n and last["a"] + last["b"] + last["c"] == blocks
    assert last["c"] == types.count(0) == len(range(0, blocks, 97)) and last["a"] + last["b"] == types.count(2)
    assert last["a"] > 1500
    print("2100 blocks: %d bytes of %d, chosen %s" % (len(raw), n, last))

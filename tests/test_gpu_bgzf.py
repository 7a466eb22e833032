"""npr_bgzf_frame (csrc/npr_bam.hip: k_bgzf_frame) read back by the specification's reader (tests/bam_reference.py): every block's
header, BSIZE, stored-block bytes, CRC-32 (zlib.crc32) and ISIZE, the end-of-file block, gzip.decompress of the whole stream; lengths
around a slice (255), a block (65 280) and several blocks."""
import numpy as np
import pytest

import bam_reference as ref

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 254, 255, 256, 65279, 65280, 65281, 2 * 65280, 3 * 65280 + 17)


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


def _payloads(n):
    rng = np.random.default_rng(n)
    return {"zeros": np.zeros(n, np.uint8), "ones": np.full(n, 0xff, np.uint8), "counter": (np.arange(n) % 251).astype(np.uint8),
            "random": rng.integers(0, 256, n).astype(np.uint8)}


@pytest.mark.parametrize("n", LENGTHS)
def test_every_block_reads_back(ctx, n):
    from nanopore_amd import bam
    for kind, data in _payloads(n).items():
        out = bam.bgzf_frame(ctx, data).tobytes()
        assert len(out) == n + 31 * ((n + ref.P - 1) // ref.P) + 28, kind
        stream, blocks = ref.bgzf_read(out)
        assert stream == data.tobytes(), kind
        assert len(blocks) == (n + ref.P - 1) // ref.P
        for u in sorted({0, 1, 254, 255, ref.P - 1, ref.P, ref.P + 1, n - 1, n} & set(range(n + 1))):
            assert ref.voffset(u) == ref.voffset_by_walking(blocks, u, n), (kind, u)
    if n == 0:
        assert out == ref.EOF_BLOCK


def test_capacity_is_checked_and_nothing_written_past_it(ctx):
    from nanopore_amd import _lib
    data = np.arange(70000, dtype=np.int64).astype(np.uint8)
    need = 70000 + 2 * 31 + 28
    out = np.full(need + 64, 0xa5, dtype=np.uint8)
    for cap in (0, 27, need - 1):
        rc = ctx._L.npr_bgzf_frame(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), cap)
        assert rc == _lib.ERR_CAPACITY and (out == 0xa5).all()
    assert ctx._L.npr_bgzf_frame(ctx._h, _lib.ptr(data), len(data), _lib.ptr(out), need) == need
    assert (out[need:] == 0xa5).all()
    assert ref.bgzf_read(out[:need].tobytes())[0] == data.tobytes()

"""The inputs of the BAM -> BAM tests (tests/test_bam_merge_host.py, tests/test_gpu_bam_merge.py): a few hundred records on the three
references of tests/bam_region_cases.py, encoded by tests/bam_pileup_reference.py (stored bin 0 everywhere: the writer's patch is visible),
chosen so that a gather of whole records between unaligned places can go wrong.  Imports nothing from the product.
  stream_a   unsorted.  Sixteen records equal but for their names of 1 .. 16 letters (every size modulo 16; one key: their order is the
             stable sort's to keep); the smallest legal record (block_size 33: no name letter, no cigar, no base); the record of 65 537
             operations of bam_region_cases (about 360 KB under the placeholder cigar with CG:B:I: larger than many gather pieces and five
             BGZF blocks); a hundred records of 40 to 600 bytes around it, so that records straddle the 65 280-byte boundaries of the output;
             refID -1 records in the middle; FLAG 4 with a position; a pos of -1 on a real reference.
  stream_b   unsorted, 60 records, a third of them with a (tid, pos, flag) that stream_a has too: ties across streams.
  empty      the header alone.
  The files: stream_a in stored-size zlib members, stream_b in another writer's 4 KB members with one block of ISIZE 0 among them."""
import numpy as np

import bam_pileup_reference as bp
import bam_reference as ref
import bam_region_cases as rc

REFS = rc.REFS
HEADER_TEXT = rc.HEADER_TEXT.replace("SO:coordinate", "SO:unsorted")
_CACHE = {}


def _nib(rng, n):
    return [int(v) for v in rng.choice([1, 2, 4, 8], n)]


def _plain(rng, name, flag, tid, pos, m):
    return bp.record(name, flag, tid, pos, [m << 4], _nib(rng, m), aux=b"NMC\x03")


def stream_a():
    if "a" in _CACHE:
        return _CACHE["a"]
    rng = np.random.default_rng(51)
    recs = []
    for k in range(60):
        recs.append(_plain(rng, "p%d" % k, 16 * (k & 1), 0, int(rng.integers(0, 250000)), int(rng.integers(2, 380))))
    for k in range(1, 17):
        recs.append(bp.record("n" * k, 0, 0, 500, [7 << 4], [1, 2, 4, 8, 1, 2, 4]))
    recs.append(bp.record("", 4, -1, -1, [], []))                                       # block_size 33
    assert len(recs[-1]) == 37
    recs.append(bp.record("u_mid", 4, -1, -1, [], _nib(rng, 30)))
    words = bp.cigar_words(rc.LONG_OPS)
    recs.append(bp.cg_record("long", 0, 0, 200000, words, _nib(rng, bp.consumed(words, bp.READ_OPS)), aux_before=b"XAZbefore\0", aux_after=b"XBi\x01\x02\x03\x04"))
    recs.append(bp.record("unmapped_placed", 4, 0, 20000, [300 << 4], _nib(rng, 300)))
    recs.append(bp.record("pos_minus_one", 0, 1, -1, [10 << 4], _nib(rng, 10)))
    recs.append(bp.record("far", 0, 0, 5000, bp.cigar_words("150M140000N150M"), _nib(rng, 300)))
    recs.append(bp.record("ends_16384", 16, 0, 16384 - 300, [300 << 4], _nib(rng, 300)))
    for k in range(40):
        recs.append(_plain(rng, "q%d" % k, 0, 1, int(rng.integers(0, 39000)), int(rng.integers(1, 40))))
    recs.append(bp.record("u_end", 4, -1, -1, [], _nib(rng, 5)))
    _CACHE["a"] = bp.header(REFS, text=HEADER_TEXT) + b"".join(recs)
    return _CACHE["a"]


def stream_b():
    if "b" in _CACHE:
        return _CACHE["b"]
    rng = np.random.default_rng(52)
    _, a = bp.split(stream_a())
    ties = [ref.bam_decode(bp.header(REFS, text=HEADER_TEXT) + r, any_writer=True)[2][0] for r in a[:20]]
    recs = []
    for k in range(40):
        recs.append(_plain(rng, "b%d" % k, 16 * (k % 3 == 0), k % 2, int(rng.integers(0, 39000)), int(rng.integers(1, 700))))
    for k, t in enumerate(ties):
        recs.append(_plain(rng, "tie%d" % k, t["flag"], t["tid"], t["pos"], 11 + k))
    recs.insert(7, bp.record("n" * 5, 0, 0, 500, [7 << 4], [8, 4, 2, 1, 8, 4, 2]))   # the key of stream_a's sixteen
    recs.insert(30, bp.record("b_unmapped", 4, -1, -1, [], _nib(rng, 12)))
    _CACHE["b"] = bp.header(REFS, text=HEADER_TEXT) + b"".join(recs)
    return _CACHE["b"]


def empty():
    return bp.header(REFS, text=HEADER_TEXT)


def with_empty_block(data, after=3):
    """a BGZF file image with a block of ISIZE 0 (the bytes of the end-of-file block) put in after its first `after` blocks"""
    at = rc.bgzf_blocks(data)[after][0]
    return data[:at] + ref.EOF_BLOCK + data[at:]


def file_a():
    return bp.bgzf(stream_a())


def file_b():
    return with_empty_block(rc.rebgzf(stream_b()))


def file_empty():
    return bp.bgzf(empty())


def foreign_sorted(stream):
    """a sorted stream as another writer's file: 4 KB members, one block of ISIZE 0 among them"""
    return with_empty_block(rc.rebgzf(stream), after=5)


def refusal_streams():
    """-> {what: a stream of three records whose second makes npr_bam_streams_bam refuse the call}"""
    rng = np.random.default_rng(53)
    head = bp.header(REFS, text=HEADER_TEXT)
    ok1, ok2 = _plain(rng, "ok1", 0, 0, 100, 20), _plain(rng, "ok2", 0, 0, 300, 20)
    nib = _nib(rng, 20)
    return {"an operation code 9": head + ok1 + bp.record("op9", 0, 0, 200, [10 << 4, 10 << 4 | 9], nib) + ok2,
            "malformed auxiliary fields under a placeholder": head + ok1 + bp.cg_record("cut", 0, 0, 200, [20 << 4], nib, aux_after=b"XX") + ok2}

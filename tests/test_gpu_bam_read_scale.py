"""The BAM reader on other writers' records and past its table sizes (npr_bam_sam: csrc/npr_bamread.hip; npr_bam_open + npr_pileup_add_bam:
csrc/npr_bampile.hip; the host side of both: csrc/npr_bam_api.cpp), on the constructed files of tests/bam_read_cases.py, which
tests/test_bam_read_cases_host.py holds to the specification's decoder and the restated pileup rules without a GPU.
  fields        records this project's writer never makes -- operation lengths at every decimal boundary, 255 / 256 / 257 / 513 operations
                stored and folded into CG, the extremes of every column, CG first, in the middle, last and alone -- through BOTH readers
  refusals      what only the device refuses in npr_bam_sam: a stored operation code above 8, a malformed auxiliary field, and a stored pos
                or next_pos of INT32_MAX, which k_bam_walk refuses (POS = pos + 1 ends at 2^31 - 1 in SAM), so npr_bam_open refuses it too
  walk rounds   WALK - 1, WALK, WALK + 1 and 2 WALK + 1 records: the resume offset, the write base of a later round, a stream that ends on a
                round's last record, the device table doubling (twice at 2 WALK + 1); these counts also make k_bam_gather_aux and
                k_bampile_add stride (GATHER_GRID, PILE_RECORDS)
  every tagged  GATHER_GRID + 1500 records with auxiliary bytes in each: a record k_bam_gather_aux drops or moves twice shows in the text
  a later round a refused record's index and stream byte in the message of the second round, both entry points
  emit grid     EMIT_GRID + 5 records, one (record, tile) item each: the only case in which k_bam_emit strides
Every comparison is exact: text byte for byte, counts and tables integer for integer.
MEASURED (one MI355X, one run, wall seconds: host build of the case / bam_sam / comparing the text / bam_open + add_bam + counts + compare):
  WALK - 1, WALK, WALK + 1   0.19 / 0.20 / 0.00 / 0.19 each, 0.6 s a test
  2 WALK + 1                 0.41 / 0.39 / 0.00 / 0.38, 1.2 s
  EMIT_GRID + 5              0.84 / 0.78 / 0.00 / 0.75, 2.4 s (a 49 MB stream, 34 MB of text)
  GATHER_GRID + 1500, every record tagged   0.06 / 0.10 / 0.00 / 0.06, 0.2 s
  a refused record in a later round 0.6 s; the fields and the refusals under 0.1 s each; the module 6.9 s.
The largest case stays far below the 15 s at which the 2 WALK + 1 case would have given up its bam_sam half: both keep both readers.  The
one-lane walk (a dependent load a record) does not dominate at a million records: the whole bam_sam call, inflate and text included, is 0.8 s."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import bam_pileup_reference as bp
import bam_read_cases as cases
from nanopore_amd import _lib
from nanopore_amd.realign import NprError

pytestmark = pytest.mark.gpu
WALK, GATHER_GRID, EMIT_GRID = cases.WALK, cases.GATHER_GRID, cases.EMIT_GRID


def _clock(label, since):
    now = time.perf_counter()
    print("%s %.2f s" % (label, now - since))
    return now


def _pileup_of(ctx, file):
    """bam_open + add_bam on a new pileup -> (n_records of the stream, counts, raised for a refused record, the table)"""
    with ctx.bam_open(file) as stream:
        pileup = ctx.pileup(stream.lengths)
        try:
            try:
                counts, raised = pileup.add_bam(stream), False
            except NprError as e:
                assert e.code == _lib.ERR_INVALID
                counts, raised = pileup.last_bam_counts, True
            return stream.n_records, counts, raised, pileup.counts()
        finally:
            pileup.close()


def test_fields_other_writers_make(gpu_ctx):
    from nanopore_amd import bam
    c = cases.field_cases()
    text, n = bam.bam_sam(gpu_ctx, c["file"])
    got = text.tobytes().decode()
    assert n == len(c["names"]) and got.startswith(c["header_text"]) and got.endswith("\n")
    lines = got[len(c["header_text"]):].split("\n")[:-1]
    assert len(lines) == n
    for name, a, b in zip(c["names"], lines, c["lines"]):
        assert a == b, (name, a[:300], b[:300])
    # the same file through the other reader
    want, want_counts, _ = bp.pileup(c["stream"])
    n_records, counts, raised, table = _pileup_of(gpu_ctx, c["file"])
    print(counts)
    assert n_records == n and counts == want_counts and raised == (want_counts["refused"] > 0) and want_counts["refused"] == 3
    assert np.array_equal(table, want), np.argwhere(table != want)[:10]


def test_refusals_only_the_device_raises(gpu_ctx, tmp_path):
    L = gpu_ctx._L
    for name, c in cases.refusal_cases().items():
        image = np.frombuffer(c["file"], dtype=np.uint8)
        out, n = np.full(6 * len(c["stream"]) + 64, 0xa5, dtype=np.uint8), C.c_int64(-7)
        assert L.npr_bam_sam(gpu_ctx._h, _lib.ptr(image), len(image), _lib.ptr(out), len(out), C.byref(n)) == _lib.ERR_INVALID, name
        assert (out == 0xa5).all() and n.value == -7, name
        assert L.npr_bam_sam(gpu_ctx._h, _lib.ptr(image), len(image), None, 0, None) == _lib.ERR_INVALID, name   # the sizing call too
        path = str(tmp_path / "bad.bam")
        with open(path, "wb") as fh:
            fh.write(c["file"])
        with pytest.raises(NprError) as e:
            gpu_ctx.bam_to_sam(path, path + ".sam")
        assert e.value.code == _lib.ERR_INVALID, name
        assert not os.path.exists(path + ".sam") and not os.path.exists(path + ".sam.tmp"), name
        if c["walk"]:   # refused in the walk: the message says which record and where, and the other entry point shares the walk
            at = bp.header_end(c["stream"]) + len(bp.split(c["stream"])[1][0])
            assert "record 1 at stream byte %d is refused (walk status 6)" % at in str(e.value), (name, str(e.value))
            with pytest.raises(NprError) as e:
                gpu_ctx.bam_open(c["file"])
            assert e.value.code == _lib.ERR_INVALID and "record 1 at stream byte %d is refused (walk status 6)" % at in str(e.value), (name, str(e.value))
        else:       # not a matter of the walk: the stream opens (a pileup has its own verdict on such a record)
            with gpu_ctx.bam_open(c["file"]) as stream:
                assert stream.n_records == 3


def _first_difference(got, want):
    a, b = got.split(b"\n"), want.split(b"\n")
    k = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
    return "line %d of %d / %d (%d past a multiple of WALK, %d past a multiple of GATHER_GRID): got %r, want %r" % (
        k, len(a) - 1, len(b) - 1, k % WALK, k % GATHER_GRID, a[k][:120] if k < len(a) else None, b[k][:120] if k < len(b) else None)


def _both_readers(ctx, n, tag_every=1000):
    from nanopore_amd import bam
    t = time.perf_counter()
    m = cases.many(n, tag_every)
    t = _clock("n = %d: host build" % n, t)
    text, got_n = bam.bam_sam(ctx, m["file"])
    t = _clock("n = %d: bam_sam" % n, t)
    got, want = text.tobytes(), m["header_text"].encode() + m["body"]
    assert got_n == n
    assert got == want, _first_difference(got[len(m["header_text"]):], m["body"])
    t = _clock("n = %d: compare" % n, t)
    n_records, counts, raised, table = _pileup_of(ctx, m["file"])
    assert n_records == n and counts == m["counts"] and not raised
    assert np.array_equal(table, m["table"]), np.argwhere(table != m["table"])[:10]
    _clock("n = %d: bam_open, add_bam, counts, compare" % n, t)


@pytest.mark.parametrize("n", (WALK - 1, WALK, WALK + 1, 2 * WALK + 1))
def test_record_counts_around_a_walk_round(gpu_ctx, n):
    """WALK - 1: one round that does not fill its table.  WALK: the stream ends exactly on the round's last record (no second launch).
    WALK + 1: a second round of one record; npr_bam_open doubles its table once, before that round.  2 WALK + 1: three rounds, and
    npr_bam_open doubles its table TWICE (before the second round to 2 WALK, before the third to 4 WALK), each time copying what it has.
    All four are above GATHER_GRID and PILE_RECORDS: k_bam_gather_aux and k_bampile_add make several trips, with tagged records (every
    1000th) and 2M1D1M records (every 4099th) in the first trip and in later ones."""
    _both_readers(gpu_ctx, n)


def test_every_record_tagged_past_the_gather_grid(gpu_ctx):
    """Auxiliary bytes in EVERY record, one trip of k_bam_gather_aux and the start of the next.  With a tag every 1000th record only, a
    gather stride of gridDim.x + 1 goes unseen: it skips the records 65536 + 65537 j alone, none of them a multiple of 1000 below
    EMIT_GRID + 5, so it skips no byte."""
    _both_readers(gpu_ctx, GATHER_GRID + 1500, tag_every=1)


def test_a_refused_record_in_a_later_round(gpu_ctx):
    from nanopore_amd import bam
    k = WALK + 5
    file, at = cases.with_block_size(cases.many(WALK + 10), k, 32)
    with pytest.raises(NprError) as e:
        bam.bam_sam(gpu_ctx, file)
    assert e.value.code == _lib.ERR_INVALID and "npr_bam_sam: record %d at stream byte %d is refused (walk status 1)" % (k, at) in str(e.value), str(e.value)
    with pytest.raises(NprError) as e:
        gpu_ctx.bam_open(file)
    assert e.value.code == _lib.ERR_INVALID and "npr_bam_open: record %d at stream byte %d is refused (walk status 1)" % (k, at) in str(e.value), str(e.value)


def test_more_items_than_the_emit_grid(gpu_ctx):
    """EMIT_GRID + 5 records of one tile each: five workgroups of k_bam_emit take a second item.  Five walk rounds; npr_bam_open's table
    doubles three times."""
    _both_readers(gpu_ctx, EMIT_GRID + 5)

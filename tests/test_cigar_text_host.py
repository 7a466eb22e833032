"""npr_sam_splice_text (include/nprealign.h, csrc/npr_io.cpp; host code, no GPU): records spliced from cigars that are text already
equal the records npr_sam_splice makes from the packed words, byte for byte and offset for offset -- the writer's half of
realignSamFile3TargetFn (nanopore/analyses/utils.py:597-605) for a job that takes its cigars as text from the device."""
import numpy as np
import pytest

from nanopore_amd import _lib, ingest, realign
from nanopore_amd._lib import ptr

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _seeded_sam(tmp_path, eol):
    """A SAM text with soft / hard clips, tags, mate fields, a record without a reference, one whose RNAME the header does not name and one
    with an operation the parser refuses (column 15 not NPR_OK for those three), lines ending in `eol`."""
    rng = np.random.default_rng(20)
    lines = ["@HD\tVN:1.0", "@SQ\tSN:chr1\tLN:100000", "@SQ\tSN:chr2\tLN:5000", "@PG\tID:seeded"]
    for i in range(60):
        ops = []
        if rng.random() < 0.3:
            ops.append("%dH" % rng.integers(1, 9))
        lead = int(rng.integers(0, 4)) if rng.random() < 0.5 else 0
        if lead:
            ops.append("%dS" % lead)
        length = lead
        for _ in range(int(rng.integers(1, 8))):
            k = int(rng.integers(1, 40))
            op = "MID"[int(rng.integers(0, 3))]
            ops.append("%d%s" % (k, op))
            length += k if op != "D" else 0
        trail = int(rng.integers(0, 4)) if rng.random() < 0.5 else 0
        if trail:
            ops.append("%dS" % trail)
        length += trail
        seq = BASES[rng.integers(0, 4, size=max(length, 1))].tobytes().decode()
        f = ["read_%d" % i, str(int(rng.choice([0, 16]))), "chr%d" % rng.integers(1, 3), str(int(rng.integers(1, 4000))), str(int(rng.integers(0, 61))),
             "".join(ops), "=" if i % 7 == 0 else "*", "0", "0", seq, "I" * len(seq) if i % 3 else "*"]
        if i % 4 == 0:
            f += ["NM:i:%d" % rng.integers(0, 50), "XX:Z:tag with blanks"]
        lines.append("\t".join(f))
    lines.insert(9, "lost\t4\t*\t0\t0\t*\t*\t0\t0\tACGT\t*")
    lines.insert(17, "stray\t0\tchrUn\t5\t1\t4M\t*\t0\t0\tACGT\t*")
    lines.insert(31, "odd\t0\tchr1\t5\t1\t2M3N2M\t*\t0\t0\tACGT\t*")
    p = str(tmp_path / "seeded.sam")
    with open(p, "w", newline="") as fh:
        fh.write(eol.join(lines) + eol)
    return p


def _new_cigars(n, rng):
    """Packed cigars for n records, placed out of order in `words`; list 5 is empty ("*"), the lengths cover one to ten digits."""
    lens = np.array([1, 9, 10, 99, 100, 12345, 999999, 1000000, (1 << 30) - 1, 0], dtype=np.uint32)
    nops = rng.integers(1, 9, size=n).astype(np.int64)
    nops[5] = 0
    order = rng.permutation(n)
    woff = np.zeros(n, dtype=np.int64)
    at = 3
    for i in order:
        woff[i] = at
        at += int(nops[i]) + int(rng.integers(0, 3))
    words = np.full(at + 2, 0xfffffffe, dtype=np.uint32)  # (the gaps hold words no list owns)
    for i in range(n):
        k = int(nops[i])
        words[woff[i]:woff[i] + k] = (lens[rng.integers(0, len(lens), size=k)] << 2) | rng.integers(0, 3, size=k).astype(np.uint32)
    return woff, nops, words


def _splice_text_raw(st, sp, ff, str_off, text, out, cap):
    rec_off = np.full(len(ff) + 1, -1, dtype=np.int64)
    rc = _lib.load().npr_sam_splice_text(ptr(st.text), ptr(sp), ptr(ff), len(ff), ptr(str_off), ptr(text), ptr(rec_off), ptr(out), cap)
    return rc, rec_off


@pytest.mark.parametrize("eol", ["\n", "\r\n"], ids=["lf", "crlf"])
def test_spliced_text_equals_spliced_words(tmp_path, eol):
    st = ingest.SamText(_seeded_sam(tmp_path, eol))
    ff = st.parse()
    sp = np.ascontiguousarray(st.span)
    n = len(ff)
    status = ff[:, ingest.F_STATUS]
    assert n == 63 and (status != 0).sum() == 3 and {int(s) for s in status} == {0, -1, ingest.SAM_NO_REFERENCE, ingest.SAM_UNKNOWN_REFERENCE}
    woff, nops, words = _new_cigars(n, np.random.default_rng(21))
    text, str_off = realign.format_cigars_packed(woff, nops, words)
    assert bytes(text[str_off[5]:str_off[6]]) == b"*"
    # the restatement of the grammar (utils.py:597-605 / pysam's cigarstring) on every list
    for i in range(n):
        want = "".join("%d%s" % (int(w) >> 2, "MID"[int(w) & 3]) for w in words[woff[i]:woff[i] + nops[i]]) or "*"
        assert bytes(text[str_off[i]:str_off[i + 1]]).decode() == want
    L = _lib.load()
    rec_w = np.zeros(n + 1, dtype=np.int64)
    total = L.npr_sam_splice(ptr(st.text), ptr(sp), ptr(ff), n, ptr(woff), ptr(nops), ptr(words), ptr(rec_w), None, 0)
    assert total > 0
    want = np.empty(total, dtype=np.uint8)
    assert L.npr_sam_splice(ptr(st.text), ptr(sp), ptr(ff), n, ptr(woff), ptr(nops), ptr(words), ptr(rec_w), ptr(want), total) == total
    # sizing call: offsets and total, nothing written
    rc, rec_t = _splice_text_raw(st, sp, ff, str_off, text, None, 0)
    assert rc == total and np.array_equal(rec_t, rec_w)
    got = np.full(total + 7, 0x55, dtype=np.uint8)
    rc, rec_t = _splice_text_raw(st, sp, ff, str_off, text, got, total)
    assert rc == total and np.array_equal(rec_t, rec_w)
    assert bytes(got[:total]) == bytes(want) and (got[total:] == 0x55).all()
    assert bytes(want).count(b"\n") == n and (eol == "\n" or b"\r" not in bytes(want))
    # one byte short
    short = np.full(total, 0x55, dtype=np.uint8)
    rc, _ = _splice_text_raw(st, sp, ff, str_off, text, short, total - 1)
    assert rc == _lib.ERR_CAPACITY and (short == 0x55).all()
    # the binding, with and without a pool
    assert bytes(st.splice_text(sp, ff, str_off, text)) == bytes(want)
    pooled = st.splice_text(sp, ff, str_off, text, take=lambda nbytes: np.full(nbytes + 3, 0x55, dtype=np.uint8))
    assert bytes(pooled) == bytes(want) == bytes(st.splice(sp, ff, woff, nops, words))
    # a sub-range of the records with offsets that do not start at zero (how a job hands over the second half of a chunk)
    m = n // 2
    assert bytes(st.splice_text(sp[m:], ff[m:], str_off[m:], text)) == bytes(want[rec_w[m]:])
    assert bytes(st.splice_text(sp[m:], ff[m:], str_off[m:] - str_off[m], text[str_off[m]:])) == bytes(want[rec_w[m]:])


def test_bad_arguments(tmp_path):
    st = ingest.SamText(_seeded_sam(tmp_path, "\n"))
    ff = st.parse()
    sp = np.ascontiguousarray(st.span)
    n = len(ff)
    text = np.frombuffer(b"1M" * n, dtype=np.uint8)
    str_off = 2 * np.arange(n + 1, dtype=np.int64)
    rc, _ = _splice_text_raw(st, sp, ff, str_off, text, None, 0)
    assert rc > 0
    bad = str_off.copy()
    bad[4] = bad[3] - 1                       # offsets that decrease
    rc, _ = _splice_text_raw(st, sp, ff, bad, text, None, 0)
    assert rc == _lib.ERR_INVALID
    L = _lib.load()
    rec = np.zeros(n + 1, dtype=np.int64)
    assert L.npr_sam_splice_text(ptr(st.text), ptr(sp), ptr(ff), -1, ptr(str_off), ptr(text), ptr(rec), None, 0) == _lib.ERR_INVALID
    assert L.npr_sam_splice_text(ptr(st.text), ptr(sp), ptr(ff), n, None, ptr(text), ptr(rec), None, 0) == _lib.ERR_INVALID
    assert L.npr_sam_splice_text(None, None, None, 0, None, None, ptr(rec), None, 0) == 0

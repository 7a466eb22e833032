"""The rules of npr_pileup_add_bam without a GPU: the restatement the GPU tests compare with (tests/bam_pileup_reference.py) gives tables worked
out by hand here on three tiny files, and csrc/npr_bamrec.h -- the record checks k_bampile_check runs, one body for host and device -- built
as a stand-alone program with AddressSanitizer and UBSan (tests/native/bamrec_check.cpp) gives the restatement's verdict, cigar source,
operation count and sums on every record of every constructed case (tests/bam_pileup_cases.py).  Nothing is loaded into Python under a
sanitizer."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_pileup_cases
import bam_pileup_reference as bp
import bam_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T, N, EQ = 1, 2, 4, 8, 15, 0


def _table(rows, entries):
    t = np.zeros((rows, 8), dtype=np.int32)
    for row, word, value in entries:
        t[row, word] = value
    return t


def test_a_deletion_an_insertion_and_another_base_by_hand():
    stream = bp.header([("r", 10)]) + bp.record("x", 0, 0, 2, bp.cigar_words("2M1I1M2D1M"), [A, C, G, T, N])
    table, counts, _ = bp.pileup(stream)
    want = _table(10, [(2, 0, 1), (2, 7, 1), (3, 1, 1), (3, 6, 1), (4, 3, 1), (5, 5, 1), (6, 5, 1), (7, 4, 1)])
    assert (table == want).all() and counts == dict(records=1, selected=1, added=1, refused=0)


def test_skips_clips_and_the_insertion_rule_by_hand():
    """2I before the first column: nothing; 3N advances the reference; 1I after it belongs to the last column before the N; the 2I behind it
    counts there, once; 1S advances the read and nothing else."""
    stream = bp.header([("r", 8)]) + bp.record("x", 0x800, 0, 0, bp.cigar_words("2I2M3N1I2I1M1S"), [A, A, C, G, T, A, A, T, C])
    table, counts, _ = bp.pileup(stream)
    want = _table(8, [(0, 1, 1), (0, 7, 1), (1, 2, 1), (1, 6, 1), (5, 3, 1)])
    assert (table == want).all() and counts == dict(records=1, selected=1, added=1, refused=0)


def test_two_sequences_a_refusal_and_a_duplicate_by_hand():
    records = [bp.record("ends with its sequence", 0, 1, 3, bp.cigar_words("3M"), [EQ, A, C]),
               bp.record("one past", 0, 0, 2, bp.cigar_words("3M"), [A, A, A]),
               bp.record("duplicate", 0x400, 0, 0, bp.cigar_words("3M"), [A, A, A]),
               bp.record("D first", 16, 1, 0, bp.cigar_words("2D1M"), [T])]
    table, counts, verdicts = bp.pileup(bp.header([("p", 4), ("q", 6)]) + b"".join(records))
    want = _table(10, [(7, 4, 1), (7, 7, 1), (8, 0, 1), (9, 1, 1), (4, 5, 1), (4, 7, 1), (5, 5, 1), (6, 3, 1)])
    assert (table == want).all() and counts == dict(records=4, selected=3, added=2, refused=1)
    assert [(v["verdict"], v["why"]) for v in verdicts] == [(bp.ADD, "none"), (bp.REFUSED, "ref"), (bp.SKIP, "none"), (bp.ADD, "none")]


def test_the_cases_hold_what_they_are_meant_to():
    """... and the encoder's files are files to other readers: gzip reads the blocks, the specification's decoder the well-formed records."""
    cases = bam_pileup_cases.cases()
    why = set()
    for name, c in cases.items():
        assert gzip.decompress(c["file"]) == c["stream"], name
        refs, records = bp.split(c["stream"])
        assert refs == list(c["refs"]) and records == list(c["records"]), name
        table, counts, verdicts = bp.pileup(c["stream"])
        why |= {v["why"] for v in verdicts}
        assert (table >= 0).all()
        c["counts"] = counts
    assert why == set(bp.WHY) - {"parts"}
    assert cases["no records"]["counts"] == dict(records=0, selected=0, added=0, refused=0)
    assert cases["not one selected"]["counts"] == dict(records=2, selected=0, added=0, refused=0)
    assert cases["not selected"]["counts"] == dict(records=10, selected=2, added=2, refused=0)   # 0x800 and 0x10 are counted
    assert cases["validation"]["counts"] == dict(records=6, selected=6, added=2, refused=4)
    assert cases["reference bounds"]["counts"] == dict(records=5, selected=5, added=3, refused=2)
    assert cases["malformed auxiliary bytes"]["counts"] == dict(records=11, selected=11, added=4, refused=7)
    assert cases["long cigar"]["counts"] == dict(records=7, selected=6, added=6, refused=0)
    assert [len(bp.check(r, [3000])["words"]) for r in cases["cigar lengths"]["records"]] == [1, 63, 64, 65, 128, 129]
    long_ = [bp.check(r, [70000]) for r in cases["long cigar"]["records"]]
    assert [(v["from_cg"], len(v["words"])) for v in long_] == [(1, 65536), (1, 65536), (1, 3), (0, 2), (1, 1), (1, 0), (0, 1)]
    for name in ("cigar lengths", "sequence edges", "insertion rule", "several sequences"):
        _, _, decoded = ref.bam_decode(cases[name]["stream"])
        assert [(d["u1"] - d["u0"], d["n_ops"]) for d in decoded] == [(len(r), r[16] | r[17] << 8) for r in cases[name]["records"]], name


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bamrec") / "bamrec_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nanopore_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bamrec_check.cpp"), "-o", exe])

    def run(items):
        """items: [(flag mask, reference lengths, record bytes)] -> [(verdict, why, from_cg, n_ops, ref_sum, read_sum)]"""
        path = exe + ".cases"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<I", len(items)))
            for mask, ref_len, rec in items:
                fh.write(struct.pack("<iI%dqI" % len(ref_len), mask, len(ref_len), *ref_len, len(rec)) + rec)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        lines = out.stdout.split("\n")
        assert out.returncode == 0 and lines[len(items)] == "bamrec_check ok", out.stdout[-2000:] + out.stderr[-4000:]
        rows = [tuple(int(v) for v in line.split()) for line in lines[:len(items)]]
        assert [r[0] for r in rows] == list(range(len(items)))
        return [(r[1], bp.WHY[r[2]]) + r[3:] for r in rows]
    return run


def test_the_shared_record_checks_give_the_restatements_verdicts(check):
    items, want, names = [], [], []
    for name, c in bam_pileup_cases.cases().items():
        ref_len = [ln for _, ln in c["refs"]]
        for mask in (bp.FLAG_MASK, 0, 0x10):
            for k, rec in enumerate(c["records"]):
                items.append((mask, ref_len, rec))
                want.append(bp.check(rec, ref_len, mask))
                names.append((name, k, mask))
    assert len(items) > 200
    for got, v, name in zip(check(items), want, names):
        assert got[:3] == (v["verdict"], v["why"], v["from_cg"]), (name, got)
        if v["why"] != "aux" and v["verdict"] != bp.SKIP:
            assert got[3:] == (len(v["words"]), v["ref_sum"], v["read_sum"]), (name, got)


def test_the_shared_record_checks_on_records_cut_and_bent(check):
    """Every byte of a record with a CG field bent in turn (the fixed fields, the name, the placeholder, the bases, the auxiliary bytes), and
    the record's block_size lowered so that it ends inside every one of its parts: the program reads no byte outside the record (it runs under
    AddressSanitizer on buffers of the record's size) and agrees with the restatement on all of them."""
    rec = bp.cg_record("r", 0, 0, 5, bp.cigar_words("3M1I2D3M"), [A, C, G, T, A, C, G], aux_before=b"XzZab\0XbBs" + struct.pack("<I2h", 2, -1, 7), aux_after=b"XiC\7")
    assert bp.check(rec, [100])["verdict"] == bp.ADD and bp.check(rec, [100])["from_cg"] == 1
    items = []
    for at in range(len(rec)):
        for flip in (0x01, 0x80, 0xff):
            b = bytearray(rec)
            b[at] ^= flip
            items.append((bp.FLAG_MASK, [100], bytes(b)))
    for size in range(32, len(rec) - 4):
        items.append((bp.FLAG_MASK, [100], struct.pack("<i", size) + rec[4:4 + size]))
    got = check(items)
    seen = set()
    for (mask, ref_len, b), g in zip(items, got):
        v = bp.check(b, ref_len, mask)
        assert g[:3] == (v["verdict"], v["why"], v["from_cg"]), (b.hex(), g)
        seen.add((v["verdict"], v["why"]))
    assert {(bp.REFUSED, w) for w in ("parts", "aux", "op", "pos", "ref", "read")} <= seen and (bp.SKIP, "none") in seen and (bp.ADD, "none") in seen

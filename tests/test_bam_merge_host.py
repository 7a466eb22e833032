"""The BAM -> BAM writer without a GPU (include/nprealign.h, "BAM streams to BAM files"): csrc/npr_bamrec.h's measure body (what
k_merge_measure runs) and virtual-offset search (what the index kernels run on a foreign file's blocks), built as a stand-alone program with
AddressSanitizer and UBSan (tests/native/bammerge_check.cpp), give exactly the restatement's end, bin, size and refusal for every record of
tests/bam_merge_cases.py and bam_reference.voffset_by_walking for every record boundary; and the restatement (tests/bam_merge_reference.py)
is checked against itself: the index of the expected sorted stream answers every region as the brute-force filter does.  Nothing is loaded
into Python under a sanitizer."""
import os
import struct
import subprocess

import pytest

import bam_merge_cases as cases
import bam_merge_reference as mref
import bam_pileup_reference as bp
import bam_read_cases
import bam_reference as ref
import bam_region_cases as rc
from helpers import ROOT

WHY_AUX, WHY_OP = 2, 3   # csrc/npr_bamrec.h BR_WHY_AUX, BR_WHY_OP


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bammerge") / "bammerge_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nanopore_amd", "csrc"), os.path.join(ROOT, "tests", "native", "bammerge_check.cpp"), "-o", exe])

    def run(records, tables):
        """records: [bytes]; tables: [(blocks [(file offset, stream offset, ISIZE)], eof offset, stream length, [u])]
        -> ([(end, bin, size, refused)], [[v(u)]])"""
        path = exe + ".cases"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<I", len(records)))
            for rec in records:
                fh.write(struct.pack("<I", len(rec)) + rec)
            fh.write(struct.pack("<I", len(tables)))
            for blocks, eof, stream_len, us in tables:
                k = len(blocks)
                fh.write(struct.pack("<I%dq%dq" % (k + 1, k + 1), k, *([b[0] for b in blocks] + [eof]), *([b[1] for b in blocks] + [stream_len])))
                fh.write(struct.pack("<I%dq" % len(us), len(us), *us))
        out = subprocess.run([exe, path], capture_output=True, text=True)
        lines = out.stdout.split("\n")
        assert out.returncode == 0 and lines[-2] == "bammerge_check ok", out.stdout[-2000:] + out.stderr[-4000:]
        rows = [tuple(int(v) for v in line.split()) for line in lines[:len(records)]]
        assert [r[0] for r in rows] == list(range(len(records)))
        vs = [[] for _ in tables]
        for line in lines[len(records):-2]:
            _, t, q, v = line.split()
            assert int(q) == len(vs[int(t)])
            vs[int(t)].append(int(v))
        return [r[1:] for r in rows], vs
    return run


def test_measure_equals_the_restatement_on_every_record(check):
    seen = 0
    for stream in (cases.stream_a(), cases.stream_b(), bam_read_cases.field_cases()["stream"], rc.sorted_stream()):
        _, records = mref.measured(stream)
        got, _ = check([r["raw"] for r in records], [])
        assert got == [(r["end"], r["bin"], r["size"], 0) for r in records]
        seen += len(records)
    assert seen > 500
    _, a = mref.measured(cases.stream_a())
    by_name = {r["line"].split("\t")[0]: r for r in a}
    assert by_name["long"]["n_ops"] == 65537 and by_name["long"]["n_cigar_op"] == 2 and by_name["long"]["size"] > 5 * ref.P
    assert by_name["long"]["bin"] == ref.reg2bin(200000, 200000 + 32768 + 20000) and by_name["unmapped_placed"]["end"] == 20001
    assert by_name[""]["size"] == 37 and by_name[""]["bin"] == 4680 and by_name["pos_minus_one"]["bin"] == 4681
    assert {r["size"] % 16 for r in a if r["line"].startswith("n")} == set(range(16))


def test_refused_records(check):
    nib = [1] * 20
    recs = [bp.record("op9", 0, 0, 200, [10 << 4, 10 << 4 | 9], nib),
            bp.cg_record("op9_in_cg", 0, 0, 200, [10 << 4, 10 << 4 | 12], nib),
            bp.cg_record("cut", 0, 0, 200, [20 << 4], nib, aux_after=b"XX"),
            bp.cg_record("cut_flag4", 4, 0, 200, [20 << 4], nib, aux_after=b"XX"),
            bp.cg_record("cut_no_ref", 0, -1, -1, [20 << 4], nib, aux_after=b"XX"),
            bp.cg_record("no_cg", 0, 0, 200, [20 << 4], nib, with_cg=False)]
    got, _ = check(recs, [])
    assert [g[3] for g in got] == [WHY_OP, WHY_OP, WHY_AUX, 0, 0, 0]
    assert got[3][:2] == (201, 4681) and got[4][1] == 4680 and got[5][0] == 220   # the stored <l_seq>S<20>N counts where no CG field does


def test_virtual_offsets_in_any_writers_blocks(check):
    tables = []
    for stream, data in ((cases.stream_b(), cases.file_b()), (cases.stream_a(), cases.file_a()), (cases.stream_a(), mref.stored_frame(cases.stream_a())),
                         (cases.empty(), cases.file_empty())):
        blocks = rc.bgzf_blocks(data)
        _, records = mref.measured(stream)
        us = sorted({r["u0"] for r in records} | {r["u1"] for r in records} | {len(stream), 0} | {b[1] for b in blocks} | {b[1] - 1 for b in blocks if b[1]})
        tables.append((blocks, len(data) - 28, len(stream), us))
    full = b"\0" * (2 * ref.P)   # a last block that is full: the end lies at the end-of-file block
    tables.append((rc.bgzf_blocks(mref.stored_frame(full)), len(mref.stored_frame(full)) - 28, len(full), [0, ref.P - 1, ref.P, 2 * ref.P - 1, 2 * ref.P]))
    assert any(b[2] == 0 for b in tables[0][0]), "a block of ISIZE 0 among the foreign file's"
    _, got = check([], tables)
    for (blocks, eof, stream_len, us), vs in zip(tables, got):
        assert vs == [ref.voffset_by_walking(blocks, u, stream_len) for u in us]
    assert got[-1][-1] == tables[-1][1] << 16
    stored = tables[2]
    assert got[2] == [ref.voffset(u) for u in stored[3]], "the closed form of the stored writer"


def test_the_restatement_against_itself():
    """the index of the expected sorted stream of the region cases answers every region as the brute-force filter does"""
    unsorted = bp.header(rc.REFS, text=rc.HEADER_TEXT) + b"".join(bp.split(rc.sorted_stream())[1][::-1])
    header = bp.header(rc.REFS, text=rc.HEADER_TEXT)
    stream, order = mref.merged([unsorted], True, header)
    _, records = mref.measured(stream)
    assert mref.in_coordinate_order(records) and not mref.in_coordinate_order(mref.measured(unsorted)[1]) and len(records) == len(rc.records())
    assert all(r["bin"] == struct.unpack_from("<H", stream, r["u0"] + 14)[0] for r in records) and any(r["bin"] != 0 for r in records)
    for data in (mref.stored_frame(stream), cases.foreign_sorted(stream)):
        blocks = rc.bgzf_blocks(data)
        bai = mref.index_of(stream, blocks)
        for region in rc.host_regions():
            assert rc.query_by_walking(bai, records, blocks, len(stream), *region) == ref.brute_overlaps(records, *region), region
    assert ref.bgzf_read(mref.stored_frame(stream))[0] == stream

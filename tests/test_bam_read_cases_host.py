"""The constructed files of tests/bam_read_cases.py are what they are named for, and their two reference routes agree: many()'s formatted
SAM body against the specification's decoder, its numpy pileup table against the restated rules record by record, its numpy-built bytes
against the plain encoder; every field case carries the field its name says; every refusal case is one the decoder cannot read or reads as
a column SAM does not allow; zlib reads every file back; and the sizes the GPU tests stand on are still the sources'.  No GPU."""
import gzip
import os
import struct

import numpy as np
import pytest

import bam_pileup_reference as bp
import bam_read_cases as cases
import bam_reference as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nanopore_amd", "csrc")


def test_the_size_constants_are_the_sources():
    for name, lines in cases.SOURCE.items():
        for file, text, count in lines:
            assert open(os.path.join(CSRC, file)).read().count(text) == count, (name, file, text)
    assert cases.WALK == 1 << 18 and cases.GATHER_GRID == 65536 and cases.EMIT_GRID == 1 << 20 and cases.PILE_RECORDS == 4096 * (256 // 64)
    # the GPU test's record counts cross every one of them
    assert cases.PILE_RECORDS < cases.GATHER_GRID < cases.WALK - 1 and 2 * cases.WALK + 1 < cases.EMIT_GRID


def test_many_5000_both_routes_agree():
    m = cases.many(5000)
    text, refs, records = ref.bam_decode(m["stream"])
    assert text == m["header_text"] and refs == cases.MANY_REFS and len(records) == 5000
    assert m["body"].decode().split("\n") == [r["line"] for r in records] + [""]
    assert [r["u0"] for r in records] + [len(m["stream"])] == m["offsets"].tolist()
    table, counts, verdicts = bp.pileup(m["stream"])
    assert counts == m["counts"] and np.array_equal(table, m["table"])
    assert m["table"][:, 5].sum() == 2 and m["table"][:, 7].sum() == 5000   # 2M1D1M at 0 and 4099
    assert cases.many(5000) is m
    # what the description promises
    lines = m["body"].decode().split("\n")
    assert lines[0].endswith("\tXi:i:0") and lines[1000].endswith("\tXi:i:1000") and lines[4099].split("\t")[5] == "2M1D1M"
    assert [lines[k].split("\t")[0] for k in (0, 35, 36, 1295, 1296, 4999)] == ["0", "z", "10", "zz", "100", "3uv"]
    assert {int(v) % 8 for v in m["offsets"]} == set(range(8))   # record offsets take every alignment


def test_many_with_a_tag_in_every_record():
    m = cases.many(1500, tag_every=1)
    records = ref.bam_decode(m["stream"])[2]
    assert m["body"].decode().split("\n") == [r["line"] for r in records] + [""]
    assert all(r["line"].endswith("\tXi:i:%d" % k) for k, r in enumerate(records))
    assert np.array_equal(m["table"], cases.many(1500)["table"]) and cases.many(1500)["body"].count(b"Xi:i:") == 2
    # the records a gather stride of GATHER_GRID + 1 would skip carry no tag at a spacing of 1000: hence this case
    assert all(k % 1000 for k in range(cases.GATHER_GRID, cases.EMIT_GRID + 5, cases.GATHER_GRID + 1))


def test_many_builds_the_bytes_of_the_plain_encoder():
    """the numpy-built stream against bp.record, record by record, where the name grows to four letters and a record is tagged"""
    m = cases.many(47005)
    names = cases._names(47005)
    assert [int(q, 36) for q in names[::97]] == list(range(0, 47005, 97)) and len(names[46655]) == 3 and len(names[46656]) == 4
    for i in list(range(0, 40)) + list(range(1290, 1300)) + [4099, 8198, 36000] + list(range(46650, 46660)) + [47000, 47004]:
        special = i % 4099 == 0
        nib = [1 << (i & 3)] * (3 if special else 1)
        want = bp.record(names[i], 16 * (i & 1), 0, (7 * i) % 4999, bp.cigar_words("2M1D1M" if special else "1M"), nib, qual=bytes([i % 94] * len(nib)),
                         aux=b"Xii" + struct.pack("<i", i) if i % 1000 == 0 else b"")
        assert m["stream"][int(m["offsets"][i]):int(m["offsets"][i + 1])] == want, i
    assert m["body"].count(b"\n") == 47005


def test_the_refused_2m1d1m_records_are_the_rules():
    """special_fits (and with it many()'s table and counts) against bam_pileup_reference.check on every 4099th record the GPU tests reach"""
    refused = []
    for i in range(0, cases.EMIT_GRID + 5, 4099):
        r = bp.record("x", 0, 0, (7 * i) % (cases.L - 1), bp.cigar_words("2M1D1M"), [1, 1, 1], qual=b"\0\0\0")
        v = bp.check(r, [cases.L])
        assert (v["verdict"] == bp.ADD) == bool(cases.special_fits(i)) and v["why"] in ("none", "ref"), i
        refused.append(v["verdict"] == bp.REFUSED)
    print("refused 2M1D1M records:", sum(refused), "of", len(refused))


def test_every_field_case_is_what_it_is_named_for():
    c = cases.field_cases()
    by = dict(zip(c["names"], c["lines"]))
    col = lambda name, k: by[name].split("\t")[k]
    assert len(c["refs"]) == 3000 and len(c["names"]) >= 36
    for name, line in by.items():
        assert line.split("\t")[0] == name and not line.endswith("\t") and "\t\t" not in line, name
    edges = "".join("%d%s" % (v, "HP"[k % 2]) for k, v in enumerate(cases.DIGIT_EDGES)) + "5M"
    assert col("lengths at the digit edges", 5) == edges and "99999999P100000000H268435455P" in edges and edges.startswith("0H9P10H")
    assert col("lengths at the digit edges folded", 5).endswith("100000000P268435455H5M") and len(by["lengths at the digit edges folded"].split("\t")) == 11
    assert col("lengths at the digit edges on N and D", 5).startswith("5M0N9D10N")
    assert col("a length of 0 first and last", 5) == "0M5M0I0D"
    for n in (255, 256, 257, 513):
        for name in ("%d operations" % n, "%d operations folded" % n):
            assert sum(col(name, 5).count(op) for op in "MID") == n and len(by[name].split("\t")) == 11, name
    assert (col("flag 65535 and mapq 255", 1), col("flag 65535 and mapq 255", 4)) == ("65535", "255")
    assert (col("pos -1 on a real refID", 2), col("pos -1 on a real refID", 3)) == ("r5", "0")
    assert (col("the largest pos and next_pos", 3), col("the largest pos and next_pos", 7)) == ("2147483647", "2147483647")
    assert (col("tlen INT32_MIN", 8), col("tlen INT32_MAX", 8), col("tlen -1", 8)) == ("-2147483648", "2147483647", "-1")
    assert (col("next_pos -1 beside a next_refID", 6), col("next_pos -1 beside a next_refID", 7)) == ("r3", "0")
    assert [col("refID -1 with a next_refID", k) for k in (2, 3, 6, 7)] == ["*", "0", c["refs"][cases.LONG_NAME][0], "12"]
    assert [col("refID -1 with a one-letter next_refID", k) for k in (2, 6, 7)] == ["*", "q", "1"]
    assert [col("a one-letter RNAME, a long RNEXT", k) for k in (2, 6)] == ["q", c["refs"][cases.LONG_NAME][0]]
    assert [col("a long RNAME, a one-letter RNEXT", k) for k in (2, 6)] == [c["refs"][cases.LONG_NAME][0], "q"]
    assert [col("next_refID equal to refID", k) for k in (2, 6, 8)] == ["q", "=", "-40"]
    assert "x" in by and "n" * 254 in by
    assert (col("odd l_seq, garbage in the unused nibble", 9), col("odd l_seq, garbage in the unused nibble", 10)) == ("ACGTA", "!\"#$%")
    assert (col("one base, garbage in the unused nibble", 9), col("one base, garbage in the unused nibble", 10)) == ("T", "~")
    assert col("qualities 0 to 93", 10) == "".join(chr(33 + v) for v in range(94))
    assert by["no cigar, no bases"] == "no cigar, no bases\t4\t*\t0\t30\t*\t*\t0\t0\t*\t*"
    assert by["CG the only field"].split("\t")[5:] == ["3M2I3M", "*", "0", "0"] + by["CG the only field"].split("\t")[9:11]
    assert by["CG first"].split("\t")[11:] == ["Xz:Z:some text", "Xc:i:7"] and col("CG first", 5) == "3M2I3M"
    assert by["CG in the middle"].split("\t")[11:] == ["Xz:Z:some text", "Xb:B:s,-3,4", "Xc:i:7"] and col("CG in the middle", 5) == "3M2I3M"
    assert by["CG last"].split("\t")[11:] == ["Xc:i:7", "Xb:B:s,-3,4"] and col("CG last", 5) == "3M2I3M"
    assert by["CG of no element"].split("\t")[5] == "*" and by["CG of no element"].split("\t")[11:] == ["Xc:i:7"]
    assert col("a second CG stays a tag", 5) == "4M" and by["a second CG stays a tag"].split("\t")[11:] == ["CG:B:I,50"]
    assert col("CG without the placeholder stays a tag", 5) == "4M" and by["CG without the placeholder stays a tag"].split("\t")[11:] == ["CG:B:I,112"]
    # the fields the text does not show
    stream, at = c["stream"], bp.header_end(c["stream"])
    recs = dict(zip(c["names"], bp.split(stream)[1]))
    assert struct.unpack_from("<H", recs["a non-zero bin"], 14)[0] == 37449
    odd = recs["odd l_seq, garbage in the unused nibble"]
    assert odd[36 + len("odd l_seq, garbage in the unused nibble") + 1 + 4 + 2] == 0x1f
    assert recs["n" * 254][12] == 255 and recs["x"][12] == 2
    # the default decoder holds this project's writer to more: it takes neither the garbage nibble nor a CG before other tags
    for name in ("odd l_seq, garbage in the unused nibble", "CG first", "CG without the placeholder stays a tag"):
        with pytest.raises(AssertionError):
            ref.bam_decode(stream[:at] + recs[name])
    # a pileup adds some, skips some, refuses some
    _, counts, verdicts = bp.pileup(stream)
    why = {n: v["why"] for n, v in zip(c["names"], verdicts) if v["verdict"] == bp.REFUSED}
    assert why == {"lengths at the digit edges on N and D": "ref", "pos -1 on a real refID": "pos", "the largest pos and next_pos": "ref"}
    assert counts["added"] >= 25 and counts["records"] - counts["selected"] >= 5


def test_every_refusal_case_is_one():
    for name, c in cases.refusal_cases().items():
        if c["walk"]:
            lines = [r["line"].split("\t") for r in ref.bam_decode(c["stream"])[2]]
            assert len(lines) == 3 and int(lines[1][{"POS": 3, "PNEXT": 7}[c["decoder"]]]) == 1 << 31, name   # SAM: at most 2^31 - 1
        else:
            with pytest.raises(c["decoder"]):
                ref.bam_decode(c["stream"])
        assert len(bp.split(c["stream"])[1]) == 3
        # the records around it are fine: the stream without the second one decodes
        first, second, third = bp.split(c["stream"])[1]
        assert len(ref.bam_decode(c["stream"][:bp.header_end(c["stream"])] + first + third)[2]) == 2


def test_zlib_reads_every_file_back():
    c = cases.field_cases()
    assert gzip.decompress(c["file"]) == c["stream"] and c["file"].endswith(ref.EOF_BLOCK)
    for c in cases.refusal_cases().values():
        assert gzip.decompress(c["file"]) == c["stream"]
    m = cases.many(5000)
    assert gzip.decompress(m["file"]) == m["stream"] and m["file"].count(bytes([0x1f, 0x8b, 8, 4])) >= 3
    file, at = cases.with_block_size(m, 4000, 32)
    back = gzip.decompress(file)
    assert at == m["offsets"][4000] and struct.unpack_from("<i", back, at)[0] == 32 and back[:at] == m["stream"][:at] and back[at + 4:] == m["stream"][at + 4:]

"""The host side of the SAM -> BAM conversion (csrc/npr_bam_host.cpp, bioio.faToTwoBit, the hub's text), no GPU: the tag converter,
the tail parser, the header, the BAI writer against the parser of tests/bam_reference.py, the .2bit round trip, and the three text files.
(The same entry points run under AddressSanitizer and UBSan in tests/native/bam_host_sanitize.cpp: `make -C nanopore_amd/csrc check-bam`.)"""
import os
import struct

import numpy as np
import pytest

import bam_reference as ref


def _sam(tmp_path, body, header="@SQ\tSN:chr1\tLN:1000\n@SQ\tSN:chr2\tLN:500\n", newline="\n"):
    from nanopore_amd import ingest
    path = str(tmp_path / "x.sam")
    with open(path, "wb") as fh:
        fh.write((header + "".join(ln + newline for ln in body)).encode())
    return ingest.SamText(path)


def _tags_of(tmp_path, tags):
    from nanopore_amd import bam
    sam = _sam(tmp_path, ["r\t0\tchr1\t1\t9\t4M\t*\t0\t0\tACGT\tIIII" + ("\t" + tags if tags else "")])
    tail = bam.parse_tail(sam, sam.parse())
    assert tail[0, bam.T_STATUS] == 0
    off, out = bam.bam_tags(sam.text, tail)
    assert off.tolist() == [0, len(out)]
    return out.tobytes()


@pytest.mark.parametrize("value,type_,fmt", [(-129, "s", "<h"), (-128, "c", "<b"), (127, "C", "<B"), (128, "C", "<B"), (255, "C", "<B"), (256, "S", "<H"),
                                             (65535, "S", "<H"), (65536, "I", "<I"), (2 ** 31 - 1, "I", "<I"), (2 ** 31, "I", "<I"), (-2 ** 31, "i", "<i"),
                                             (0, "C", "<B"), (-32768, "s", "<h"), (-32769, "i", "<i"), (2 ** 32 - 1, "I", "<I")])
def test_integer_tags_take_the_smallest_type(tmp_path, value, type_, fmt):
    assert _tags_of(tmp_path, "XI:i:%d" % value) == b"XI" + type_.encode() + struct.pack(fmt, value)


def test_every_tag_type(tmp_path):
    got = _tags_of(tmp_path, "Xa:A:q\tXf:f:1.5\tXz:Z:two  words \tXh:H:1AE301\tXe:Z:")
    assert got == b"XaAq" + b"Xff" + struct.pack("<f", 1.5) + b"XzZtwo  words \0" + b"XhH1AE301\0" + b"XeZ\0"
    assert _tags_of(tmp_path, "") == b""
    for sub, fmt, vals in (("c", "b", [-128, 127]), ("C", "B", [0, 255]), ("s", "h", [-32768, 32767]), ("S", "H", [0, 65535]), ("i", "i", [-2 ** 31, 2 ** 31 - 1]),
                           ("I", "I", [0, 2 ** 32 - 1]), ("f", "f", [0.5, -2.0, 1e10])):
        text = "XB:B:" + ",".join([sub] + [("%g" % v) if sub == "f" else str(v) for v in vals])
        assert _tags_of(tmp_path, text) == b"XBB" + sub.encode() + struct.pack("<I", len(vals)) + struct.pack("<%d%s" % (len(vals), fmt), *vals)
        assert _tags_of(tmp_path, "XB:B:" + sub) == b"XBB" + sub.encode() + struct.pack("<I", 0)
    assert ref._aux_text(_tags_of(tmp_path, "NM:i:7\tXB:B:s,-3,4")) == ["NM:i:7", "XB:B:s,-3,4"]


@pytest.mark.parametrize("tags", ["X:i:1", "XX:i:", "XX:i:1.5", "XX:i:4294967296", "XX:i:-2147483649", "XX:q:1", "XX:A:ab", "XX:A:", "XX:f:abc", "XX:H:ABC", "XX:H:GG",
                                  "XX:B:c,128", "XX:B:C,-1", "XX:B:S,65536", "XX:B:x,1", "XX:B:", "XX:B:c,", "XX:B:c1", "XX:i:1\t", "XX:i:1\t\tYY:i:2", "XXi:1"])
def test_malformed_tags_are_refused(tmp_path, tags):
    from nanopore_amd import _lib
    with pytest.raises(_lib.NprError) as e:
        _tags_of(tmp_path, tags)
    assert e.value.code == _lib.ERR_INVALID


@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_tail_parser(tmp_path, newline):
    from nanopore_amd import bam
    body = ["a\t0\tchr2\t7\t9\t4M\t=\t11\t-5\tACGT\tIIII",                        # 11 columns, "="
            "b\t16\tchr1\t7\t9\t4M\t*\t0\t0\tACGT\t*\tNM:i:1\tXZ:Z:x y",         # "*", QUAL "*", tags
            "c\t0\tchr1\t7\t9\t4M\tchr2\t1\t2147483647\tACGT\tIIII\tNM:i:1",     # a name
            "d\t0\tchr1\t7\t9\t4M\tchrX\t1\t0\tACGT\tIIII",                      # unknown RNEXT
            "e\t0\tchr1\t7\t9\t4M\t*\t0\t0\tACGT\tIII",                          # QUAL too short
            "f\t0\tchr1\t7\t9\t4M\t*\t0\t0\t*\tIIII",                            # QUAL without SEQ
            "g\t0\tchr1\t7\t9\t4M\t*\t0\t0\tACGT",                               # 10 columns
            "h\t0\tchr1\t7\t9\t4M\t*\tx\t0\tACGT\tIIII",                         # PNEXT not a number
            "i\t65536\tchr1\t7\t9\t4M\t*\t0\t0\tACGT\tIIII",                     # FLAG too large
            "j\t0\t*\t0\t0\t*\t=\t0\t0\t*\t*"]                                   # "=" of a record without a reference
    sam = _sam(tmp_path, body, newline=newline)
    fields = sam.parse()
    tail = bam.parse_tail(sam, fields)
    text = sam.text.tobytes()
    assert tail[:, bam.T_STATUS].tolist() == [0, 0, 0, 0, -1, -1, -1, -1, -1, 0]
    assert tail[:4, bam.T_RNEXT].tolist() == [1, -1, 1, -1] and tail[9, bam.T_RNEXT] == -1
    assert tail[:3, bam.T_PNEXT].tolist() == [10, -1, 0] and tail[:3, bam.T_TLEN].tolist() == [-5, 0, 2147483647]
    assert [text[a:b] for a, b in tail[:3, bam.T_QUAL_LO:bam.T_QUAL_HI + 1]] == [b"IIII", b"*", b"IIII"]
    assert [text[a:b] for a, b in tail[:3, bam.T_TAGS_LO:bam.T_TAGS_HI + 1]] == [b"", b"NM:i:1\tXZ:Z:x y", b"NM:i:1"]
    off, out = bam.bam_tags(sam.text, tail)
    assert np.diff(off).tolist() == [0, 4 + 7, 4, 0, 0, 0, 0, 0, 0, 0]       # a line with a bad status has no bytes


def test_header(tmp_path):
    from nanopore_amd import _lib, bam
    sq = "@SQ\tSN:chr1\tLN:1000\n@SQ\tLN:500\tSN:c2\tM5:x\n"

    def parts(header, sort=True):
        out, lengths = bam.bam_header(header.encode(), sort)
        stream = out.tobytes() + b""
        text, refs, records = ref.bam_decode(stream)
        assert records == [] and lengths.tolist() == [r[1] for r in refs]
        return text, refs
    assert parts(sq) == ("@HD\tVN:1.0\tSO:coordinate\n" + sq, [("chr1", 1000), ("c2", 500)])
    assert parts(sq, sort=False)[0] == "@HD\tVN:1.0\tSO:unsorted\n" + sq
    assert parts("@HD\tVN:1.4\tSO:queryname\tGO:none\n" + sq + "@PG\tID:x\n")[0] == "@HD\tVN:1.4\tSO:coordinate\tGO:none\n" + sq + "@PG\tID:x\n"
    assert parts("@HD\tVN:1.4\tSO:coordinate\n" + sq, sort=False)[0] == "@HD\tVN:1.4\tSO:unsorted\n" + sq
    assert parts("@HD\tVN:1.4\n" + sq)[0] == "@HD\tVN:1.4\tSO:coordinate\n" + sq
    for bad in ("", "@HD\tVN:1.0\n", "@SQ\tSN:a\n", "@SQ\tLN:5\n", "@SQ\tSN:a\tLN:0\n", "@SQ\tSN:a\tLN:x\n"):
        with pytest.raises(_lib.NprError) as e:
            bam.bam_header(bad.encode())
        assert e.value.code == _lib.ERR_INVALID


def test_bai_writer_against_the_parser():
    from nanopore_amd import _lib, bam
    ref_len = [40000, 10, 100000]
    none = ref.NONE
    run_tid, run_bin = [0, 0, 0, 2, -1], [0, 4681, 4681, 4683, 4680]
    run_beg, run_end = [5, 100, 300, 400, 900], [100, 200, 400, 900, 950]
    linear = [none, 100, 300] + [none] + [none, none, 400, none, none, none, none]
    meta = [[5, 400, 3, 1], [none, 0, 0, 0], [400, 900, 2, 0]]
    data = bam.bai_write(ref_len, run_tid, run_bin, run_beg, run_end, linear, meta, 4).tobytes()
    index, no_coor = ref.bai_parse(data)
    assert no_coor == 4
    assert index[0] == ({0: [(5, 100)], 4681: [(100, 200), (300, 400)], 37450: [(5, 400), (3, 1)]}, [100, 100, 300])
    assert index[1] == ({}, [])
    assert index[2] == ({4683: [(400, 900)], 37450: [(400, 900), (2, 0)]}, [400, 400, 400])
    bins = [{0: [(5, 100)], 4681: [(100, 200), (300, 400)]}, {}, {4683: [(400, 900)]}]
    assert data == ref.bai_bytes(bins, [[100, 100, 300], [], [400, 400, 400]], [[5, 400, 3, 1], None, [400, 900, 2, 0]], 4)
    with pytest.raises(_lib.NprError):
        bam.bai_write(ref_len, [2, 0], [1, 1], [0, 0], [1, 1], linear, meta, 0)      # runs out of order
    with pytest.raises(_lib.NprError):
        bam.bai_write(ref_len, [3], [1], [0], [1], linear, meta, 0)                   # a tid the table does not have
    empty = bam.bai_write([], [], [], [], [], [], np.zeros((0, 4)), 0).tobytes()
    assert empty == b"BAI\1" + struct.pack("<iQ", 0, 0)


def test_reg2bin_and_reg2bins_agree():
    rng = np.random.default_rng(1)
    for _ in range(2000):
        beg = int(rng.integers(0, 1 << 29))
        end = min(1 << 29, beg + 1 + int(rng.choice([0, 1, 100, 16384, 1 << 20, 1 << 27])))
        assert ref.reg2bin(beg, end) in ref.reg2bins(beg, end)
    assert ref.reg2bin(0, 1) == 4681 and ref.reg2bin(16383, 16385) == 585 and ref.reg2bin(0, 1 << 29) == 0


def test_fa_to_two_bit_round_trip(tmp_path):
    from nanopore_amd.bioio import faToTwoBit
    rng = np.random.default_rng(2)
    seqs = [("len%d" % n, "".join(rng.choice(list("ACGTacgtNn"), n))) for n in range(10)]
    seqs += [("runs", "NNNNacgtACGTnnnnNNNNacgNNN"), ("long", "".join(rng.choice(list("ACGT"), 1003))), ("lowerN", "nnnn"), ("edge", "aCgTn" * 5 + "N")]
    fa, out = str(tmp_path / "x.fa"), str(tmp_path / "x.2bit")
    with open(fa, "w") as fh:
        for name, s in seqs:
            fh.write(">%s some description\n" % name + "".join(s[i:i + 7] + "\n" for i in range(0, len(s), 7)))
    faToTwoBit(fa, out)
    data = open(out, "rb").read()
    assert ref.twobit_decode(data) == seqs
    assert struct.unpack_from("<IIII", data) == (0x1A412743, 0, len(seqs), 0)
    one = str(tmp_path / "one.fa")
    with open(one, "w") as fh:
        fh.write(">s\nTCAGN\n")
    faToTwoBit(one, out)
    assert open(out, "rb").read() == struct.pack("<IIII", 0x1A412743, 0, 1, 0) + b"\x01s" + struct.pack("<I", 22) + struct.pack("<IIII", 5, 1, 4, 1) + \
        struct.pack("<II", 0, 0) + bytes([0b00011011, 0])


def test_hub_text_files():
    from nanopore_amd.metaAnalyses import customTrackAssemblyHub as hub
    exp = "experiment_r7_2D.fastq_ecoli.fa_LastChain"
    assert hub.trackDbText(exp, 3) == ("track 3_\nlongLabel experiment_r7_2D.fastq_ecoli.fa_LastChain\nshortLabel 2D_LastChain\npriority 10\nvisibility pack\n"
                                      "colorByStrand 150,100,30 230,170,40\ncolor 150,100,30\naltColor 230,170,40\n"
                                      "bigDataUrl bamFiles/experiment_r7_2D.fastq_ecoli.fa_LastChain.sorted.bam\ntype bam\ngroup 2D\nhtml assembly\n\n")
    assert hub.genomesText("ecoli", "gi|1", 4641652) == ("genome ecoli\ntrackDb ecoli/trackDb.txt\ngroups groups.txt\ndescription ecoli\ntwoBitPath ecoli/ecoli.2bit\n"
                                                         "organism ecoli\ndefaultPos gi|1:1-4641652\n\n")
    assert hub.GROUPS_TEXT == "name readType\nlabel readType\npriority 1\ndefaultIsClosed 0\n\n"
    assert hub.referenceHeader("/a/b/ecoli.fa") == "ecoli" and hub.referenceHeader("x/ecoli.k12.fasta") == "ecoli.k12"


def test_hub_is_reachable_by_name_and_not_a_default():
    from nanopore_amd import pipeline
    from nanopore_amd.metaAnalyses.abstractMetaAnalysis import AbstractMetaAnalysis
    found = pipeline.resolveClasses("CustomTrackAssemblyHub", "nanopore_amd.metaAnalyses", AbstractMetaAnalysis)
    assert [c.__name__ for c in found] == ["CustomTrackAssemblyHub"] and found[0] not in pipeline.metaAnalyses


def test_hub_reports_a_failed_conversion(tmp_path, monkeypatch):
    """An experiment without a mapping: the text files are still written, and the failure is raised for the driver's _failed path."""
    from nanopore_amd.analyses import utils
    from nanopore_amd.metaAnalyses.customTrackAssemblyHub import CustomTrackAssemblyHub
    fa = str(tmp_path / "ref.fa")
    with open(fa, "w") as fh:
        fh.write(">s1 x\nACGT\n>s2\nACGTAC\n")
    calls = []

    def convert(samFile, bamFile, ctx=None):
        calls.append((samFile, bamFile))
        if "bad" in samFile:
            raise IOError("no such file")
        open(bamFile, "wb").close()
    monkeypatch.setattr(utils, "samToSortedBamFile", convert)
    out = str(tmp_path / "hub")
    os.mkdir(out)

    class Mapper(object):
        pass
    experiments = [("r.fastq", "2D", fa, Mapper, [], str(tmp_path / "experiment_r.fastq_ref.fa_Mapper")),
                   ("r.fastq", "2D", fa, Mapper, [], str(tmp_path / "experiment_bad.fastq_ref.fa_Mapper"))]
    with pytest.raises(RuntimeError) as e:
        CustomTrackAssemblyHub(out, experiments).run()
    assert "experiment_bad.fastq_ref.fa_Mapper" in str(e.value) and len(calls) == 2
    assert sorted(os.listdir(out)) == ["genomes.txt", "groups.txt", "ref"]
    assert sorted(os.listdir(os.path.join(out, "ref"))) == ["bamFiles", "ref.2bit", "ref.fa", "trackDb.txt"]
    assert open(os.path.join(out, "genomes.txt")).read().endswith("defaultPos s2:1-6\n\n")
    assert open(os.path.join(out, "ref", "trackDb.txt")).read().startswith("track 1_\nlongLabel experiment_r.fastq_ref.fa_Mapper\nshortLabel r_Mapper\n")
    assert ref.twobit_decode(open(os.path.join(out, "ref", "ref.2bit"), "rb").read()) == [("s1", "ACGT"), ("s2", "ACGTAC")]

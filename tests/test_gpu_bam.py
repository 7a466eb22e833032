"""npr_sam_bam through Context.sam_to_bam: a constructed SAM file converted on the device and read back with the specification's decoder
(tests/bam_reference.py) -- the records in stable key order, byte for byte; the long-cigar form; the BAI against the restated rules and
against brute-force region queries; the unsorted variant; a bad line; and the track hub through the pipeline driver.

Sizes behind the test below.  A record takes 36 + l_name + 1 + 4 n_cigar + (l_seq + 1) / 2 + l_seq + tag bytes (+ 8 + 4 n_ops with a CG
tag).  The first two records in sorted order (POS 0, then POS 1 with a padded Z tag) are sized so that the second ends exactly on the
first BGZF block edge; the 70 001-base record is longer than a block and must straddle one."""
import os

import numpy as np
import pytest

import bam_reference as ref

pytestmark = pytest.mark.gpu

TILE = 4096
REFS = [("chr1", 300000), ("chr2", 100000), ("chr3", 200000)]
HEADER = "@HD\tVN:1.4\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "@PG\tID:test\tCL:a b\n"
TAGS = "NM:i:3\tXa:A:q\tXf:f:1.5\tXg:f:-0.25\tXz:Z:two words\tXh:H:1AE301\tXb:B:c,-1,2\tXs:B:S,65535,0\tXe:B:f,0.5,-2\tXi:i:-70000\tXn:B:i"
LETTERS = "=ACMGRSVTWYHKDBNacmgrsvtwyhkdbn.?"


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _qual(rng, n):
    return "".join(chr(33 + c) for c in rng.integers(0, 60, n))


def _records():
    rng = np.random.default_rng(12)
    out = []

    def add(name, flag, rname, pos, cigar, seq, qual=None, tags="", mapq=30, rnext="*", pnext=0, tlen=0):
        qual = _qual(rng, len(seq)) if qual is None and seq != "*" else (qual or "*")
        out.append("\t".join([name, str(flag), rname, str(pos), str(mapq), cigar, rnext, str(pnext), str(tlen), seq, qual] + ([tags] if tags else [])))

    for k, n in enumerate((1, 2, 3, 255, 256, 257, TILE - 1, TILE, TILE + 1, 70001)):
        add("len%d" % n, 16 * (k & 1), "chr1" if k & 2 else "chr3", int(rng.integers(2, 90000)), "%dM" % n, _seq(rng, n), tags=TAGS if k % 3 == 0 else "")
    add("noseq", 0, "chr1", 5000, "*", "*", "*")
    add("noqual", 0, "chr1", 5000, "20M", _seq(rng, 20), "*", tags="RG:Z:g")
    add("n", 0, "chr3", 16384, "4M", "ACGT")
    add("N" * 254, 16, "chr3", 16385, "4M", "ACGT", rnext="=", pnext=17000, tlen=-616)
    add("allops", 0, "chr1", 131000, "5H3S10M2I4D100N5=3X1P2M4S", _seq(rng, 29), tags=TAGS, rnext="chr3", pnext=77, tlen=12)
    add("letters", 0, "chr1", 131072, "%dM" % len(LETTERS), LETTERS)
    add("pos0", 4, "chr1", 0, "*", _seq(rng, 10))
    add("unmapped_placed", 4, "chr1", 131073, "*", _seq(rng, 7), rnext="=", pnext=131073)
    add("unmapped", 4, "*", 0, "*", _seq(rng, 9))
    add("unmapped2", 4 + 16, "*", 0, "*", "*", "*", tags="Xq:i:255")
    for ops in (65535, 65536, 70000):
        add("ops%d" % ops, 0, "chr1", 100 + ops, "1M1I" * (ops // 2) + ("1M" if ops & 1 else ""), _seq(rng, ops), tags="XA:i:-129" if ops != 65536 else "")
    for k in range(40):   # a crowd around window and bin edges
        add("w%d" % k, 16 * (k & 1), "chr1" if k < 25 else "chr3", 16384 * (1 + k % 9) - 10 + 3 * (k % 7), "%dM" % (5 + 3 * k), _seq(rng, 5 + 3 * k))
    return out


def _header_bytes():
    text = HEADER.replace("SO:unsorted", "SO:coordinate")
    return 12 + len(text) + sum(9 + len(n) for n, _ in REFS)


def _sam_text():
    """The records, with the padded POS 1 record sized so that it ends on the first block edge, shuffled."""
    lines = _records()
    first = [ln for ln in lines if ln.startswith("pos0\t")][0].split("\t")
    size_first = 36 + len(first[0]) + 1 + (len(first[9]) + 1) // 2 + len(first[9])
    pad = ref.P - _header_bytes() - size_first - (36 + 4 + 1 + 4 + 2 + 4 + 4)   # name "edge", cigar 4M, SEQ ACGT, tag XP:Z: + NUL
    lines.append("\t".join(["edge", "0", "chr1", "1", "9", "4M", "*", "0", "0", "ACGT", "IIII", "XP:Z:" + "p" * pad]))
    order = np.random.default_rng(3).permutation(len(lines))
    return [lines[i] for i in order]


def _normalised(line):
    f = line.split("\t")
    f[9] = "".join(c.upper() if c.upper() in ref.BASES else "N" for c in f[9]) if f[9] != "*" else "*"
    return "\t".join(f)


def _key(line):
    f = line.split("\t")
    tid = [n for n, _ in REFS].index(f[2]) if f[2] != "*" else -1
    return ref.sort_key(tid, int(f[3]) - 1, int(f[1]), len(REFS))


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def converted(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("bam")
    lines = _sam_text()
    sam = str(d / "in.sam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "\n".join(lines) + "\n")
    bam = str(d / "out.sorted.bam")
    counts = ctx.sam_to_bam(sam, bam)
    stream, blocks = ref.bgzf_read(open(bam, "rb").read())
    text, refs, records = ref.bam_decode(stream)
    return dict(dir=d, sam=sam, bam=bam, lines=lines, counts=counts, stream=stream, blocks=blocks, text=text, refs=refs, records=records)


def test_round_trip_in_stable_key_order(converted):
    c = converted
    assert c["text"] == HEADER.replace("SO:unsorted", "SO:coordinate") and c["refs"] == REFS
    want = [_normalised(ln) for ln in sorted(c["lines"], key=_key)]
    got = [r["line"] for r in c["records"]]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w, (g[:200], w[:200])
    assert c["counts"]["records"] == len(want) and c["counts"]["no_coordinate"] == 2 and c["counts"]["unmapped"] == 4
    for r in c["records"]:
        assert r["bin"] == ref.record_bin(r), r["line"][:80]


def test_long_cigars_take_the_placeholder_form(converted):
    by_name = {r["line"].split("\t")[0]: r for r in converted["records"]}
    assert by_name["ops65535"]["n_cigar_op"] == 65535 == by_name["ops65535"]["n_ops"]
    for ops in (65536, 70000):
        r = by_name["ops%d" % ops]
        assert r["n_cigar_op"] == 2 and r["n_ops"] == ops     # (bam_decode checked the placeholder and unfolded CG)


def test_records_at_block_edges(converted):
    records, blocks = converted["records"], converted["blocks"]
    assert len(blocks) >= 4
    assert any(r["u1"] % ref.P == 0 for r in records), "no record ends exactly on a block edge"
    assert records[1]["line"].startswith("edge\t") and records[1]["u1"] == ref.P
    assert any(r["u0"] // ref.P != (r["u1"] - 1) // ref.P for r in records), "no record straddles a block edge"
    n = len(converted["stream"])
    for r in records:
        for u in (r["u0"], r["u1"]):
            assert ref.voffset(u) == ref.voffset_by_walking(blocks, u, n)


def test_index_bytes_and_region_queries(converted):
    records = converted["records"]
    bai = open(converted["bam"] + ".bai", "rb").read()
    bins, linear, meta, no_coor = ref.expected_index(records, [ln for _, ln in REFS])
    assert bai == ref.bai_bytes(bins, linear, meta, no_coor)
    index, n_no_coor = ref.bai_parse(bai)
    assert n_no_coor == 2 and index[1] == ({}, [])            # chr2 has no record
    rng = np.random.default_rng(8)
    regions = [(t, 0, ln) for t, (_, ln) in enumerate(REFS)]
    for edge in (16384, 32768, 131072, 131072 + 16384, 262144):
        regions += [(0, edge - 1, edge), (0, edge, edge + 1), (2, edge % 200000, edge % 200000 + 1)]
    regions += [(0, 290000, 300000), (2, 190000, 200000), (1, 5, 50000), (0, 0, 1)]
    while len(regions) < 200:
        t = int(rng.choice([0, 0, 2, 1]))
        beg = int(rng.integers(0, REFS[t][1] - 1))
        regions.append((t, beg, min(REFS[t][1], beg + int(rng.choice([1, 10, 1000, 20000, 150000])))))
    hits = 0
    for t, beg, end in regions:
        got = ref.bai_query(index, records, t, beg, end)
        assert got == ref.brute_overlaps(records, t, beg, end), (t, beg, end)
        hits += bool(got)
    assert 50 < hits < len(regions)


def test_unsorted_variant_keeps_file_order_and_writes_no_index(ctx, converted):
    out = str(converted["dir"] / "unsorted.bam")
    from nanopore_amd.analyses import utils
    utils.samToBamFile(converted["sam"], out, ctx=ctx)
    assert not os.path.exists(out + ".bai")
    text, refs, records = ref.bam_decode(ref.bgzf_read(open(out, "rb").read())[0])
    assert text == HEADER and [r["line"] for r in records] == [_normalised(ln) for ln in converted["lines"]]


@pytest.mark.parametrize("bad", ("r\t0\tchr1\t5\t9\t4M\t*\t0\t0\tACGT", "r\t0\tchr1\t5\t9\t4M\t*\t0\t0\tACGT\tIII", "r\t0\tchr9\t5\t9\t4M\t*\t0\t0\tACGT\tIIII",
                                 "r\t0\tchr1\t5\t9\t4Q\t*\t0\t0\tACGT\tIIII", "r\t0\tchr1\t5\t9\t4M\t*\t0\t0\tACGT\tIIII\tXX:i:1.5"))
def test_a_bad_line_fails_the_call_and_leaves_no_file(ctx, tmp_path, bad):
    from nanopore_amd import _lib
    sam, out = str(tmp_path / "bad.sam"), str(tmp_path / "bad.bam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "ok\t0\tchr1\t5\t9\t4M\t*\t0\t0\tACGT\tIIII\n" + bad + "\n")
    with pytest.raises(_lib.NprError):
        ctx.sam_to_bam(sam, out)
    assert os.listdir(str(tmp_path)) == ["bad.sam"]


def test_track_hub_through_the_pipeline_driver(tmp_path):
    from nanopore_amd import pipeline
    from test_gpu_pipeline_driver import _experiment, _processed, _working_dir
    work = _working_dir(tmp_path / "work")
    assert pipeline.main([work, "--mappers", "SeedMapperChain", "--analyses", "Hmm", "--metaAnalyses", "CustomTrackAssemblyHub"]) == 0
    assert pipeline.metaAnalyses == [m for m in pipeline.metaAnalyses if m.__name__ != "CustomTrackAssemblyHub"]   # not a default
    hub = os.path.join(work, "output", "metaAnalysis_CustomTrackAssemblyHub")
    exp = _experiment(work, "SeedMapperChain")
    name = os.path.basename(exp)
    assert sorted(os.listdir(hub)) == ["genomes.txt", "groups.txt", "reference"]
    assert sorted(os.listdir(os.path.join(hub, "reference"))) == ["bamFiles", "reference.2bit", "reference.fa", "trackDb.txt"]
    assert sorted(os.listdir(os.path.join(hub, "reference", "bamFiles"))) == [name + ".sorted.bam", name + ".sorted.bam.bai"]
    from nanopore_amd.bioio import fastaRead
    fasta = [(n.split()[0], s) for n, s in fastaRead(_processed(work)[1])]
    assert open(os.path.join(hub, "genomes.txt")).read() == (
        "genome reference\ntrackDb reference/trackDb.txt\ngroups groups.txt\ndescription reference\ntwoBitPath reference/reference.2bit\n"
        "organism reference\ndefaultPos %s:1-%d\n\n" % (fasta[-1][0], len(fasta[-1][1])))
    assert ("bigDataUrl bamFiles/%s.sorted.bam\n" % name) in open(os.path.join(hub, "reference", "trackDb.txt")).read()
    sam = [ln for ln in open(os.path.join(exp, "mapping.sam")).read().split("\n") if ln and not ln.startswith("@")]
    names =[f[3:] for ln in open(os.path.join(exp, "mapping.sam")).read().split("\n") if ln.startswith("@SQ") for f in ln.split("\t") if f.startswith("SN:")]
    text, refs, records = ref.bam_decode(ref.bgzf_read(open(os.path.join(hub, "reference", "bamFiles", name + ".sorted.bam"), "rb").read())[0])
    assert [r[0] for r in refs] == names

    def key(line):
        f = line.split("\t")
        return ref.sort_key(names.index(f[2]) if f[2] != "*" else -1, int(f[3]) - 1, int(f[1]), len(names))
    assert [r["line"] for r in records] == [_normalised(ln) for ln in sorted(sam, key=key)] and len(records) == 2
    index, _ = ref.bai_parse(open(os.path.join(hub, "reference", "bamFiles", name + ".sorted.bam.bai"), "rb").read())
    assert ref.bai_query(index, records, 0, 0, refs[0][1]) == [0, 1]
    assert ref.twobit_decode(open(os.path.join(hub, "reference", "reference.2bit"), "rb").read()) == fasta

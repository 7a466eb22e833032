"""npr_sam_bam_deflate through Context.sam_to_bam(compress=True): the file read with tests/bgzf_deflate_reference.py holds the same
stream as the stored file, byte for byte, sorted and unsorted; it is smaller; its index answers every region query of the stored-file
test through its own block list, and every virtual offset in it points at the stream byte the stored index's points at; the refusals
are the stored path's; the track hub with compressed files.

The SAM input is that of tests/test_gpu_bam.py (copied: the two records sized so that the second ends exactly on the first BGZF block
edge, through a padded Z tag, and the 70 001-base record that straddles one)."""
import os

import numpy as np
import pytest

import bam_reference as ref
import bgzf_deflate_reference as dref

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
    add("longnoqual", 0, "chr3", 150000, "9000M", _seq(rng, 9000), "*")
    add("n", 0, "chr3", 16384, "4M", "ACGT")
    add("N" * 254, 16, "chr3", 16385, "4M", "ACGT", rnext="=", pnext=17000, tlen=-616)
    add("allops", 0, "chr1", 131000, "5H3S10M2I4D100N5=3X1P2M4S", _seq(rng, 29), tags=TAGS, rnext="chr3", pnext=77, tlen=12)
    add("letters", 0, "chr1", 131072, "%dM" % len(LETTERS), LETTERS)
    add("pos0", 4, "chr1", 0, "*", _seq(rng, 10))
    add("unmapped_placed", 4, "chr1", 131073, "*", _seq(rng, 7), rnext="=", pnext=131073)
    add("unmapped", 4, "*", 0, "*", _seq(rng, 9))
    add("unmapped2", 4 + 16, "*", 0, "*", "*", "*", tags="Xq:i:255")
    for k in range(40):   # a crowd around window and bin edges
        add("w%d" % k, 16 * (k & 1), "chr1" if k < 25 else "chr3", 16384 * (1 + k % 9) - 10 + 3 * (k % 7), "%dM" % (5 + 3 * k), _seq(rng, 5 + 3 * k))
    return out


def _header_bytes():
    text = HEADER.replace("SO:unsorted", "SO:coordinate")
    return 12 + len(text) + sum(9 + len(n) for n, _ in REFS)


def _sam_text(last_edge=False):
    """The records, with the padded POS 1 record sized so that it ends on the first block edge, shuffled.  last_edge: only the two
    records before that edge, so the stream ends exactly on it."""
    lines = _records()
    first = [ln for ln in lines if ln.startswith("pos0\t")][0].split("\t")
    size_first = 36 + len(first[0]) + 1 + (len(first[9]) + 1) // 2 + len(first[9])
    pad = ref.P - _header_bytes() - size_first - (36 + 4 + 1 + 4 + 2 + 4 + 4)   # name "edge", cigar 4M, SEQ ACGT, tag XP:Z: + NUL
    edge = "\t".join(["edge", "0", "chr1", "1", "9", "4M", "*", "0", "0", "ACGT", "IIII", "XP:Z:" + "p" * pad])
    if last_edge:
        return [edge, "\t".join(first)]
    lines.append(edge)
    order = np.random.default_rng(3).permutation(len(lines))
    return [lines[i] for i in order]


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


def _read(path, reader):
    data = open(path, "rb").read()
    stream, blocks = reader(data)
    return dict(data=data, stream=stream, blocks=blocks)


@pytest.fixture(scope="module")
def converted(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("bamz")
    sam = str(d / "in.sam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "\n".join(_sam_text()) + "\n")
    stored, packed = str(d / "stored.bam"), str(d / "packed.bam")
    counts_s = ctx.sam_to_bam(sam, stored)
    counts_p = ctx.sam_to_bam(sam, packed, compress=True)
    s, p = _read(stored, ref.bgzf_read), _read(packed, dref.bgzf_read)
    records = ref.bam_decode(p["stream"])[2]
    return dict(dir=d, sam=sam, stored=stored, packed=packed, s=s, p=p, counts_s=counts_s, counts_p=counts_p, records=records)


def test_same_stream_in_a_smaller_file(converted):
    c = converted
    assert c["p"]["stream"] == c["s"]["stream"]
    assert len(c["p"]["data"]) < len(c["s"]["data"])
    print("stored %d bytes, compressed %d" % (len(c["s"]["data"]), len(c["p"]["data"])), "BTYPE", dref.block_types(c["p"]["data"]))
    assert "stream_bytes" not in c["counts_s"]
    assert c["counts_p"] == dict(c["counts_s"], bytes=len(c["p"]["data"]), stream_bytes=len(c["p"]["stream"]))
    records, n = c["records"], len(c["p"]["stream"])
    assert len(c["p"]["blocks"]) >= 3
    assert records[1]["line"].startswith("edge\t") and records[1]["u1"] == ref.P
    assert any(r["u0"] // ref.P != (r["u1"] - 1) // ref.P for r in records), "no record straddles a block edge"


def test_unsorted_variant(ctx, converted):
    from nanopore_amd.analyses import utils
    a, b = str(converted["dir"] / "u_stored.bam"), str(converted["dir"] / "u_packed.bam")
    utils.samToBamFile(converted["sam"], a, ctx=ctx)
    utils.samToBamFile(converted["sam"], b, ctx=ctx, compress=True)
    assert not os.path.exists(b + ".bai")
    assert dref.bgzf_read(open(b, "rb").read())[0] == ref.bgzf_read(open(a, "rb").read())[0]
    assert os.path.getsize(b) < os.path.getsize(a)


def test_index_offsets_and_region_queries(converted):
    c = converted
    records, blocks, n, file_len = c["records"], c["p"]["blocks"], len(c["p"]["stream"]), len(c["p"]["data"])
    bai_s, bai_p = open(c["stored"] + ".bai", "rb").read(), open(c["packed"] + ".bai", "rb").read()
    assert len(bai_s) == len(bai_p)
    # every virtual offset of the compressed index points at the stream byte the stored index's does
    (idx_s, no_s), (idx_p, no_p) = ref.bai_parse(bai_s), ref.bai_parse(bai_p)
    assert no_s == no_p == 2
    seen = 0
    for (bins_s, lin_s), (bins_p, lin_p) in zip(idx_s, idx_p):
        assert sorted(bins_s) == sorted(bins_p) and len(lin_s) == len(lin_p)
        pairs = list(zip(lin_s, lin_p))
        for b in bins_s:
            assert len(bins_s[b]) == len(bins_p[b])
            if b == 37450:   # the second pseudo-chunk holds counts, not offsets
                assert bins_s[b][1] == bins_p[b][1]
                pairs += list(zip(bins_s[b][0], bins_p[b][0]))
            else:
                pairs += [(x, y) for cs, cp in zip(bins_s[b], bins_p[b]) for x, y in zip(cs, cp)]
        for vs, vp in pairs:
            us = (vs >> 16) // (ref.P + 31) * ref.P + (vs & 0xffff)
            assert dref.voffset_to_stream(blocks, vp, n, file_len) == us
            seen += 1
    assert seen > 0
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
        got = dref.bai_query_blocks(idx_p, records, blocks, n, file_len, t, beg, end)
        assert got == ref.brute_overlaps(records, t, beg, end), (t, beg, end)
        hits += bool(got)
    assert 50 < hits < len(regions)


def test_a_stream_that_ends_on_a_block_edge(ctx, tmp_path):
    sam = str(tmp_path / "edge.sam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "\n".join(_sam_text(last_edge=True)) + "\n")
    a, b = str(tmp_path / "a.bam"), str(tmp_path / "b.bam")
    ctx.sam_to_bam(sam, a)
    ctx.sam_to_bam(sam, b, compress=True)
    s, p = _read(a, ref.bgzf_read), _read(b, dref.bgzf_read)
    assert p["stream"] == s["stream"] and len(p["stream"]) == ref.P and len(p["blocks"]) == 1
    (idx_s, _), (idx_p, _) = ref.bai_parse(open(a + ".bai", "rb").read()), ref.bai_parse(open(b + ".bai", "rb").read())
    # the end of the last record is the end-of-file block's offset in both layouts
    assert idx_s[0][0][37450][0][1] == (ref.P + 31) << 16
    assert idx_p[0][0][37450][0][1] == (len(p["data"]) - 28) << 16
    records = ref.bam_decode(p["stream"])[2]
    assert dref.bai_query_blocks(idx_p, records, p["blocks"], ref.P, len(p["data"]), 0, 0, 300000) == [0, 1]


@pytest.mark.parametrize("bad", ("r\t0\tchr9\t5\t9\t4M\t*\t0\t0\tACGT\tIIII", "r\t0\tchr1\t5\t9\t4Q\t*\t0\t0\tACGT\tIIII"))
def test_a_bad_line_fails_the_call_and_leaves_no_file(ctx, tmp_path, bad):
    from nanopore_amd import _lib
    sam, out = str(tmp_path / "bad.sam"), str(tmp_path / "bad.bam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "ok\t0\tchr1\t5\t9\t4M\t*\t0\t0\tACGT\tIIII\n" + bad + "\n")
    with pytest.raises(_lib.NprError):
        ctx.sam_to_bam(sam, out, compress=True)
    assert os.listdir(str(tmp_path)) == ["bad.sam"]


def test_compressed_track_hub_through_the_pipeline_driver(tmp_path):
    from nanopore_amd import pipeline
    from test_gpu_pipeline_driver import _experiment, _working_dir
    work = _working_dir(tmp_path / "work")
    assert pipeline.main([work, "--mappers", "SeedMapperChain", "--analyses", "Hmm", "--metaAnalyses", "CustomTrackAssemblyHubCompressed"]) == 0
    assert "CustomTrackAssemblyHubCompressed" not in [m.__name__ for m in pipeline.metaAnalyses]   # not a default
    hub = os.path.join(work, "output", "metaAnalysis_CustomTrackAssemblyHubCompressed")
    name = os.path.basename(_experiment(work, "SeedMapperChain"))
    assert sorted(os.listdir(hub)) == ["genomes.txt", "groups.txt", "reference"]
    assert sorted(os.listdir(os.path.join(hub, "reference"))) == ["bamFiles", "reference.2bit", "reference.fa", "trackDb.txt"]
    assert sorted(os.listdir(os.path.join(hub, "reference", "bamFiles"))) == [name + ".sorted.bam", name + ".sorted.bam.bai"]
    data = open(os.path.join(hub, "reference", "bamFiles", name + ".sorted.bam"), "rb").read()
    stream, blocks = dref.bgzf_read(data)
    assert len(data) <= len(stream) + 31 * len(blocks) + 28
    print("hub file: %d bytes for a stream of %d, BTYPE %s" % (len(data), len(stream), dref.block_types(data)))
    text, refs, records = ref.bam_decode(stream)
    assert len(records) == 2
    index, _ = ref.bai_parse(open(os.path.join(hub, "reference", "bamFiles", name + ".sorted.bam.bai"), "rb").read())
    assert dref.bai_query_blocks(index, records, blocks, len(stream), len(data), 0, 0, refs[0][1]) == [0, 1]

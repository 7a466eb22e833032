"""Region queries on an indexed BAM file on the device (include/nprealign.h, "region queries": npr_bam_open_region, npr_bam_stream_restrict,
npr_bam_stream_sam; csrc/npr_bamregion.hip; Context.bam_open(index=, region=), BamStream.restrict / sam_text, bam.bam_region_to_sam,
analyses/pileup.py pileup_of_bam(region=), analyses/utils.py bamDepthFile(region=)) on three files of the records of
tests/bam_region_cases.py: the device writer's stored and compressed ones with the index it made, and the same stream cut into another
writer's 4 KB blocks with an index built by the specification's rules in Python.  The record set of a query equals the reader through the
index restated in Python and the brute-force filter, as SAM lines of the specification's decoder; the blocks inflated are the ones the
chunks and the header need; pileup rows inside the region equal the whole file's.  Counts and bytes: every comparison is exact."""
import gzip
import os

import numpy as np
import pytest

import bam_reference as ref
import bam_region_cases as cases
from nanopore_amd import _lib, bam
from nanopore_amd.realign import NprError

pytestmark = pytest.mark.gpu

NAMES = ("stored", "compressed", "foreign")
REF_LEN = [ln for _, ln in cases.REFS]
ROW0 = [0, 300000, 340000]
PILEUP_REGIONS = [(0, 16383, 16384), (0, 100000, 103000), (0, 240000, 240010), (1, 1000, 30000), (2, 0, 5000), (0, 290000, 300000)]


@pytest.fixture(scope="module")
def files(gpu_ctx, tmp_path_factory):
    """name -> dict(path, data, bai, stream, decoded, lines, blocks, head_end, table, depth): the references, computed once, never changed"""
    from nanopore_amd.analyses import utils
    from nanopore_amd.analyses.pileup import pileup_of_bam
    d = tmp_path_factory.mktemp("bamregion")
    sam = str(d / "in.sam")
    with open(sam, "w") as fh:
        fh.write(cases.sam_text())
    out = {}
    for name in NAMES:
        path = str(d / (name + ".bam"))
        if name == "foreign":
            data = cases.rebgzf(out["stored"]["stream"])
            with open(path, "wb") as fh:
                fh.write(data)
        else:
            gpu_ctx.sam_to_bam(sam, path, sort=True, index=True, compress=name == "compressed")
            data = open(path, "rb").read()
        stream = gzip.decompress(data)
        text, refs, decoded = ref.bam_decode(stream, any_writer=True)
        blocks = cases.bgzf_blocks(data)
        if name == "foreign":
            with open(path + ".bai", "wb") as fh:
                fh.write(cases.spec_index(decoded, REF_LEN, blocks, len(stream)))
        names, lengths, pileup = pileup_of_bam(gpu_ctx, path)
        try:
            table = pileup.counts()
        finally:
            pileup.close()
        table.setflags(write=False)
        utils.bamDepthFile(path, path + ".depth", ctx=gpu_ctx)
        assert refs == cases.REFS and len(decoded) == len(cases.records()) and len(blocks) >= 5 and table[:, :4].sum() > 100000
        out[name] = dict(path=path, data=np.frombuffer(data, dtype=np.uint8), bai=open(path + ".bai", "rb").read(), stream=stream, text=text, decoded=decoded,
                         lines=[r["line"] for r in decoded], blocks=blocks, head_end=cases.header_end(stream), table=table, depth=open(path + ".depth").read())
    assert out["stored"]["stream"] == out["compressed"]["stream"] and len(out["compressed"]["data"]) < len(out["stored"]["data"]) // 2
    long_ = [r for r in out["stored"]["decoded"] if r["line"].startswith("long\t")]
    assert len(long_) == 1 and long_[0]["n_cigar_op"] == 2 and long_[0]["n_ops"] == 65537, "the long record lies under the placeholder cigar"
    return out


def _sam(stream):
    """sam_text() -> (header text, [line])"""
    text = stream.sam_text().tobytes().decode()
    return text[:stream.l_text], text[stream.l_text:].split("\n")[:-1]


def _expect(f, tid, beg, end):
    """the record set by the brute-force filter, which the reader through the index (restated in Python) must find too"""
    want = ref.brute_overlaps(f["decoded"], tid, beg, end)
    assert cases.query_by_walking(f["bai"], f["decoded"], f["blocks"], len(f["stream"]), tid, beg, end) == want
    return want


@pytest.mark.parametrize("name", NAMES)
def test_the_record_set_and_the_blocks_inflated(gpu_ctx, files, name):
    f = files[name]
    predicted = {r: cases.blocks_rule(f["blocks"], cases.chunks_rule(f["bai"], *r), f["head_end"]) for r in cases.gpu_regions()}
    partial = [r for r, need in predicted.items() if len(need) < len(f["blocks"])]
    assert partial and len(predicted[(0, 0, 300000)]) > len(predicted[(0, 16383, 16384)]), "computed before anything runs: some regions need fewer blocks than the file has"
    print(name, "blocks", len(f["blocks"]), {r: len(need) for r, need in predicted.items()})
    sizes = set()
    for region in cases.gpu_regions():
        want = _expect(f, *region)
        if name == "stored":
            assert ref.bai_query(ref.bai_parse(f["bai"])[0], f["decoded"], *region) == want
        with gpu_ctx.bam_open(f["data"], index=f["bai"], region=region) as s:
            last = bam.inflate_last(gpu_ctx)
            need = predicted[region]
            assert last["blocks"] == len(need) and last["failed_block"] == -1, region
            assert s.stream_bytes == last["stream_bytes"] == sum(f["blocks"][k][2] for k in need), region
            assert s.n_records == len(want) and s.references == [n for n, _ in cases.REFS] and s.lengths.tolist() == REF_LEN
            header, lines = _sam(s)
            assert header == f["text"] and lines == [f["lines"][i] for i in want], region
        with gpu_ctx.bam_open(f["data"]) as whole:
            assert whole.n_records == len(f["decoded"]) and bam.inflate_last(gpu_ctx)["blocks"] == len(f["blocks"])
            assert whole.restrict(region) == len(want) == whole.n_records
            assert _sam(whole) == (f["text"], [f["lines"][i] for i in want]), region
        sizes.add(len(want))
    assert 0 in sizes and max(sizes) > 300
    for region in ((2, 0, 5000), (0, 290000, 300000)):   # the empty reference, and past the last record
        assert _expect(f, *region) == []


def test_regions_as_strings_and_without_an_index(gpu_ctx, files):
    f = files["compressed"]
    for text, region in (("chrB", (1, 0, 40000)), ("chrA:16384-16384", (0, 16383, 16384)), ("chrA:100,001-103,000", (0, 100000, 103000)), ("chrC", (2, 0, 5000)),
                         ("chrA:262144", (0, 262143, 300000))):
        want = [f["lines"][i] for i in _expect(f, *region)]
        named = (cases.REFS[region[0]][0],) + region[1:]
        with gpu_ctx.bam_open(f["data"], index=f["bai"], region=text) as a, gpu_ctx.bam_open(f["data"], index=f["bai"], region=named) as b, \
                gpu_ctx.bam_open(f["data"], region=text) as c:
            assert _sam(a)[1] == _sam(b)[1] == _sam(c)[1] == want, text
    with pytest.raises(KeyError):
        gpu_ctx.bam_open(f["data"], index=f["bai"], region="chrD:1-5")
    with pytest.raises(ValueError):
        gpu_ctx.bam_open(f["data"], index=f["bai"])


@pytest.mark.parametrize("name", NAMES)
def test_the_pileup_inside_a_region_is_the_whole_files(gpu_ctx, files, name):
    from nanopore_amd.analyses import utils
    from nanopore_amd.analyses.pileup import pileup_of_bam
    f = files[name]
    for tid, beg, end in PILEUP_REGIONS:
        names, lengths, pileup = pileup_of_bam(gpu_ctx, f["path"], region=(tid, beg, end))
        try:
            got, counts = pileup.counts(), pileup.last_bam_counts
        finally:
            pileup.close()
        assert bam.inflate_last(gpu_ctx)["blocks"] == len(cases.blocks_rule(f["blocks"], cases.chunks_rule(f["bai"], tid, beg, end), f["head_end"]))   # (x.bam.bai was found)
        want = _expect(f, tid, beg, end)
        assert counts["records"] == len(want) and counts["refused"] == 0
        lo, hi = ROW0[tid] + beg, ROW0[tid] + min(end, REF_LEN[tid])
        assert np.array_equal(got[lo:hi], f["table"][lo:hi]), (tid, beg, end)   # all eight words
        if not want:
            assert not got.any()
        else:
            assert (got <= f["table"]).all() and got.any()
        depth = f["path"] + ".region.depth"
        utils.bamDepthFile(f["path"], depth, ctx=gpu_ctx, region=(tid, beg, end))
        lines = [ln for ln in f["depth"].split("\n")[:-1] if ln.split("\t")[0] == cases.REFS[tid][0] and beg < int(ln.split("\t")[1]) <= end]
        assert open(depth).read() == "".join(ln + "\n" for ln in lines), (tid, beg, end)
    assert f["table"][ROW0[0] + 100000:ROW0[0] + 103000, :4].any()


def test_restrict_on_an_unsorted_file_and_twice(gpu_ctx, files, tmp_path):
    sam, path = str(tmp_path / "in.sam"), str(tmp_path / "unsorted.bam")
    with open(sam, "w") as fh:
        fh.write(cases.sam_text())
    gpu_ctx.sam_to_bam(sam, path, sort=False, index=False)
    data = open(path, "rb").read()
    _, _, decoded = ref.bam_decode(gzip.decompress(data), any_writer=True)
    assert [r["line"].split("\t")[0] for r in decoded] == [r["name"] for r in cases.records()], "the file's order is the SAM file's"
    for region in ((0, 100000, 103000), (0, 0, 300000), (1, 16384, 16385), (2, 0, 5000)):
        want = ref.brute_overlaps(decoded, *region)
        with gpu_ctx.bam_open(data, region=region) as s:
            assert _sam(s)[1] == [decoded[i]["line"] for i in want]
    a, b = (0, 90000, 150000), (0, 140000, 210000)
    both = sorted(set(ref.brute_overlaps(decoded, *a)) & set(ref.brute_overlaps(decoded, *b)))
    assert 0 < len(both) < len(ref.brute_overlaps(decoded, *a))
    with gpu_ctx.bam_open(data) as s:
        assert s.restrict(a) == len(ref.brute_overlaps(decoded, *a)) and s.restrict(b) == len(both)
        assert _sam(s)[1] == [decoded[i]["line"] for i in both]
        assert s.restrict((1, 0, 40000)) == 0 and _sam(s)[1] == []
        with pytest.raises(NprError) as e:
            s.restrict((0, 5, 5))
        assert e.value.code == _lib.ERR_INVALID and s.n_records == 0


def test_bam_region_to_sam(gpu_ctx, files, tmp_path):
    f = files["compressed"]
    out = str(tmp_path / "region.sam")
    want = _expect(f, 0, 100000, 103000)
    counts = bam.bam_region_to_sam(gpu_ctx, f["path"], "chrA:100001-103000", out)
    assert counts["indexed"] and counts["records"] == len(want) and counts["blocks"] < len(f["blocks"])
    assert open(out).read() == f["text"] + "".join(f["lines"][i] + "\n" for i in want) and not os.path.exists(out + ".tmp")
    other = str(tmp_path / "copy.bam")   # no index beside it: the whole file, restricted
    with open(other, "wb") as fh:
        fh.write(f["data"].tobytes())
    counts = bam.bam_region_to_sam(gpu_ctx, other, ("chrA", 100000, 103000), out)
    assert not counts["indexed"] and counts["blocks"] == len(f["blocks"]) and open(out).read() == f["text"] + "".join(f["lines"][i] + "\n" for i in want)


# ---------------------------------------------------------------- refusals: malformed input is refused by a check, nothing here is meant to fault
def _index_of_one_chunk(vb, ve):
    """a BAI file of the three references whose only chunk, in the bin of window 0 of the first, is [vb, ve)"""
    return ref.bai_bytes([{4681: [(vb, ve)]}, {}, {}], [[0], [], []], [None, None, None], 0)


@pytest.mark.parametrize("name", NAMES)
def test_malformed_indices_are_refused_and_the_context_stays_usable(gpu_ctx, files, name):
    f = files[name]
    blocks, stream_len = f["blocks"], len(f["stream"])
    first = next(r for r in f["decoded"] if r["tid"] == 0 and r["pos"] < 16000)
    k = next(i for i, (at, u, isize) in enumerate(blocks) if u <= first["u0"] < u + isize)
    vo = lambda u: ref.voffset_by_walking(blocks, u, stream_len)   # noqa: E731
    good = _index_of_one_chunk(vo(first["u0"]), vo(first["u1"]))
    region = (0, first["pos"], first["pos"] + 1)
    with gpu_ctx.bam_open(f["data"], index=good, region=region) as s:
        assert _sam(s)[1] == [first["line"]]
    assert first["u0"] + 40 < blocks[k][1] + blocks[k][2], "forty bytes on lie in the same block"
    assert blocks[k][2] < 65535 and k + 1 < len(blocks)
    after = blocks[k + 1][0] << 16   # (a chunk must not end before it begins: the index reader refuses that before the file is looked at)
    bad = {   # what: (the index, a word of the refusal that tells which check made it)
        "an index of a file with another n_ref": (cases.spec_index(f["decoded"], REF_LEN + [77], blocks, stream_len), "number of reference sequences"),
        "a block offset that is no block": (_index_of_one_chunk((blocks[k][0] + 1) << 16, after), "in a block of the file"),
        "an end in no block": (_index_of_one_chunk(vo(first["u0"]), (blocks[-1][0] + 3) << 16), "in a block of the file"),
        "low bits past ISIZE": (_index_of_one_chunk(blocks[k][0] << 16 | (blocks[k][2] + 1), after), "ISIZE"),
        "low bits of the end past ISIZE": (_index_of_one_chunk(vo(first["u0"]), blocks[k][0] << 16 | (blocks[k][2] + 1)), "ISIZE"),
        "a chunk that starts in the middle of a record": (_index_of_one_chunk(vo(first["u0"]) + 5, vo(first["u1"])), "walk status"),
        "a chunk that ends in the middle of a record": (_index_of_one_chunk(vo(first["u0"]), vo(first["u0"]) + 40), "walk status 7"),
    }
    for what, (index, word) in bad.items():
        before = len(gpu_ctx._open)
        with pytest.raises(NprError) as e:
            gpu_ctx.bam_open(f["data"], index=index, region=region)
        assert e.value.code == _lib.ERR_INVALID and word in str(e.value), (what, str(e.value))
        assert len(gpu_ctx._open) == before, "no object"
        print(what, "->", str(e.value)[:200])
        with gpu_ctx.bam_open(f["data"], index=f["bai"], region=region) as s:   # a good query after it
            assert first["line"] in _sam(s)[1], what

"""Sorted, merged and region BAM files straight from BAM streams on the device, and the index of a file as it stands (include/nprealign.h,
"BAM streams to BAM files": npr_bam_streams_bam, npr_bam_index; csrc/npr_bammerge.hip; Context.bam_merge / bam_index, bam.bam_sort /
bam_merge / bam_region_to_bam / bam_index, mappers/bamFileMapper.py CombinedBamFile) on the inputs of tests/bam_merge_cases.py against the
rules restated in tests/bam_merge_reference.py.  Bytes and counts: every comparison is exact."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

import bam_merge_cases as cases
import bam_merge_reference as mref
import bam_read_cases
import bam_reference as ref
import bam_region_cases as rc
from nanopore_amd import _lib, bam
from nanopore_amd._lib import ptr
from nanopore_amd.realign import NprError

pytestmark = pytest.mark.gpu

def _header(text, sort):
    return bam.bam_header(text.encode() if isinstance(text, str) else text, sort=sort)[0].tobytes()


def _names(stream):
    return [r["line"].split("\t")[0] for r in mref.measured(stream)[1]]


@pytest.fixture(scope="module")
def sorted_files(gpu_ctx, tmp_path_factory):
    """the region cases through the SAM route: the unsorted file, and the sorted stored and compressed ones with the index the writer made"""
    d = tmp_path_factory.mktemp("bammerge")
    sam = str(d / "in.sam")
    with open(sam, "w") as fh:
        fh.write(rc.sam_text())
    out = {"dir": d, "unsorted": str(d / "unsorted.bam")}
    gpu_ctx.sam_to_bam(sam, out["unsorted"], sort=False, index=False)
    for name in ("stored", "compressed"):
        out[name] = str(d / (name + ".bam"))
        gpu_ctx.sam_to_bam(sam, out[name], sort=True, index=True, compress=name == "compressed")
    return out


def test_sort_equals_the_reference(gpu_ctx):
    for stream, data in ((cases.stream_a(), cases.file_a()), (bam_read_cases.field_cases()["stream"], bam_read_cases.field_cases()["file"])):
        text = ref.bam_decode(stream[:rc.header_end(stream)])[0]
        want, order = mref.merged([stream], True, _header(text, True))
        assert order != sorted(order), "the input is not sorted"
        with gpu_ctx.bam_open(data) as s:
            image, bai = gpu_ctx.bam_merge([s])
            packed, bai_packed = gpu_ctx.bam_merge([s], compress=True)
            last = gpu_ctx.bam_merge_last()
        assert gzip.decompress(image.tobytes()) == want and image.tobytes() == mref.stored_frame(want)
        assert bai.tobytes() == mref.index_of(want, rc.stored_blocks(len(want)))
        assert gzip.decompress(packed.tobytes()) == want and len(packed) < len(image)
        assert bai_packed.tobytes() == mref.index_of(want, rc.bgzf_blocks(packed.tobytes()))
        assert last["records"] == len(order) and last["stream_bytes"] == len(want) and last["gather_ns"] > 0
    # the foreign fields came through byte for byte: the records are the input's but for bin
    _, got = mref.measured(want)
    _, had = mref.measured(stream)
    assert sorted(r["raw"][:14] + r["raw"][16:] for r in got) == sorted(r["raw"][:14] + r["raw"][16:] for r in had)


@pytest.mark.parametrize("sort", (True, False))
def test_merge_three_streams(gpu_ctx, sort):
    streams = [cases.stream_a(), cases.stream_b(), cases.empty(), cases.stream_a()]   # (a stream may appear twice)
    want, order = mref.merged(streams, sort, _header(cases.HEADER_TEXT, sort))
    with gpu_ctx.bam_open(cases.file_a()) as a, gpu_ctx.bam_open(cases.file_b()) as b, gpu_ctx.bam_open(cases.file_empty()) as e:
        assert e.n_records == 0 and bam.inflate_last(gpu_ctx)["blocks"] == 1
        before = [s.sam_text().tobytes() for s in (a, b, e)]
        image, bai = gpu_ctx.bam_merge([a, b, e, a], sort=sort)
        assert gpu_ctx.bam_merge_last()["records"] == len(order) == 2 * a.n_records + b.n_records
        assert [s.sam_text().tobytes() for s in (a, b, e)] == before, "the streams are unchanged"
    assert gzip.decompress(image.tobytes()) == want and image.tobytes() == mref.stored_frame(want)
    if sort:
        assert bai.tobytes() == mref.index_of(want, rc.stored_blocks(len(want)))
        names = _names(want)   # ties keep stream order: stream_a's sixteen, stream_b's one of the same key, stream_a's again
        k = names.index("n")
        assert names[k:k + 16] == ["n" * j for j in range(1, 17)] and names[k + 16] == "nnnnn" and names[k + 17:k + 33] == ["n" * j for j in range(1, 17)]
    else:
        assert bai is None and _names(want) == [n for s in streams for n in _names(s)]


def test_bam_route_equals_sam_route(gpu_ctx, sorted_files):
    for name in ("stored", "compressed"):
        out = str(sorted_files["dir"] / ("direct_" + name + ".bam"))
        counts = bam.bam_sort(gpu_ctx, sorted_files["unsorted"], out, compress=name == "compressed")
        assert counts["records"] == len(rc.records())
        assert open(out, "rb").read() == open(sorted_files[name], "rb").read()
        assert open(out + ".bai", "rb").read() == open(sorted_files[name] + ".bai", "rb").read()


def test_region_to_bam(gpu_ctx, sorted_files, tmp_path):
    path = sorted_files["compressed"]
    _, _, decoded = ref.bam_decode(gzip.decompress(open(path, "rb").read()), any_writer=True)
    out = str(tmp_path / "region.bam")
    for region in rc.gpu_regions():
        want = ref.brute_overlaps(decoded, *region)
        counts = bam.bam_region_to_bam(gpu_ctx, path, region, out)
        assert counts["indexed"] and counts["records"] == len(want)
        data = open(out, "rb").read()
        _, refs, got = ref.bam_decode(gzip.decompress(data), any_writer=True)
        assert refs == rc.REFS and [r["line"] for r in got] == [decoded[i]["line"] for i in want], region
        tid, beg, end = region
        sub = (tid, beg + (end - beg) // 3, end - (end - beg) // 4)
        with gpu_ctx.bam_open(np.frombuffer(data, dtype=np.uint8), index=open(out + ".bai", "rb").read(), region=sub) as s:
            lines = s.sam_text().tobytes().decode()[s.l_text:].split("\n")[:-1]
        assert lines == [got[i]["line"] for i in ref.brute_overlaps(got, *sub)], (region, sub)


def test_index_of_a_foreign_file(gpu_ctx, sorted_files, tmp_path):
    stream = gzip.decompress(open(sorted_files["stored"], "rb").read())
    foreign = cases.foreign_sorted(stream)
    blocks = rc.bgzf_blocks(foreign)
    assert any(b[2] == 0 for b in blocks)
    assert gpu_ctx.bam_index(foreign).tobytes() == mref.index_of(stream, blocks)
    for name in ("stored", "compressed"):
        assert gpu_ctx.bam_index(open(sorted_files[name], "rb").read()).tobytes() == open(sorted_files[name] + ".bai", "rb").read()
    path = str(tmp_path / "foreign.bam")
    with open(path, "wb") as fh:
        fh.write(foreign)
    assert bam.bam_index(gpu_ctx, path)["bytes"] == len(mref.index_of(stream, blocks)) and open(path + ".bai", "rb").read() == mref.index_of(stream, blocks)
    # two records swapped: refused
    _, records = mref.measured(stream)
    k = next(i for i in range(len(records) - 1) if records[i]["tid"] == 0 and records[i + 1]["tid"] == 0 and records[i]["pos"] < records[i + 1]["pos"])
    a, b = records[k], records[k + 1]
    swapped = stream[:a["u0"]] + b["raw"] + a["raw"] + stream[b["u1"]:]
    with pytest.raises(NprError) as e:
        gpu_ctx.bam_index(rc.rebgzf(swapped))
    assert e.value.code == _lib.ERR_INVALID and "coordinate order" in str(e.value)
    with pytest.raises(NprError) as e:   # ... and the unsorted file of the SAM route
        gpu_ctx.bam_index(open(sorted_files["unsorted"], "rb").read())
    assert e.value.code == _lib.ERR_INVALID


def _call(ctx, handles, header, out, cap, sort=1):
    """npr_bam_streams_bam itself, with index arrays of room for 1000 records"""
    arr = (C.c_void_p * max(len(handles), 1))(*handles)
    n = 1000
    tid, bin_, beg, end = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros(n, np.uint64)
    linear, meta = np.zeros(64, np.uint64), np.zeros((3, 4), np.uint64)
    n_runs, n_no_coor, n_records = C.c_int64(0), C.c_int64(0), C.c_int64(0)
    return ctx._L.npr_bam_streams_bam(ctx._h, arr, len(handles), ptr(header), len(header), sort, 0, ptr(out), cap, C.byref(n_records), C.byref(n_runs), ptr(tid), ptr(bin_),
                                      ptr(beg), ptr(end), ptr(linear), ptr(meta), C.byref(n_no_coor))


def test_refusals(gpu_ctx):
    """every one a refused input with a bounded, checked path: nothing here is meant to fault"""
    from nanopore_amd import realign
    header = np.frombuffer(_header(cases.HEADER_TEXT, True), dtype=np.uint8)
    out = np.full(1 << 20, 0xA5, dtype=np.uint8)
    for what, stream in cases.refusal_streams().items():
        with gpu_ctx.bam_open(rc.rebgzf(stream)) as s:
            assert s.n_records == 3
            assert _call(gpu_ctx, [s._h], header, out, len(out)) == _lib.ERR_INVALID, what
            assert what.split()[-1] in gpu_ctx.last_error() or "above 8" in gpu_ctx.last_error(), gpu_ctx.last_error()
        assert (out == 0xA5).all(), what
    with gpu_ctx.bam_open(cases.file_b()) as b, gpu_ctx.bam_open(bam_read_cases.field_cases()["file"]) as other:
        assert _call(gpu_ctx, [b._h, other._h], header, out, len(out)) == _lib.ERR_INVALID and "reference sequences differ" in gpu_ctx.last_error()
        wrong = np.frombuffer(_header(bam_read_cases.field_cases()["header_text"], True), dtype=np.uint8)
        assert _call(gpu_ctx, [b._h], wrong, out, len(out)) == _lib.ERR_INVALID and "not a BAM header" in gpu_ctx.last_error()
        assert _call(gpu_ctx, [], header, out, len(out)) == _lib.ERR_INVALID
        assert _call(gpu_ctx, [b._h], header, out, 1000) == _lib.ERR_CAPACITY
        second = realign.Context(0)
        try:
            with second.bam_open(cases.file_b()) as foreign:
                assert _call(gpu_ctx, [b._h, foreign._h], header, out, len(out)) == _lib.ERR_INVALID and "another context" in gpu_ctx.last_error()
        finally:
            second.close()
        assert (out == 0xA5).all()
        total = _call(gpu_ctx, [b._h], header, out, len(out))   # a good call after them
        assert total > 0 and gzip.decompress(out[:total].tobytes()) == mref.merged([cases.stream_b()], True, header.tobytes())[0]
    with pytest.raises(NprError):
        gpu_ctx.bam_merge([])


def test_streams_are_unchanged(gpu_ctx, sorted_files):
    data = np.fromfile(sorted_files["compressed"], dtype=np.uint8)
    with gpu_ctx.bam_open(data, index=open(sorted_files["compressed"] + ".bai", "rb").read(), region=(0, 100000, 103000)) as s, gpu_ctx.bam_open(cases.file_a()) as a:
        before = (s.sam_text().tobytes(), a.sam_text().tobytes(), s.n_records, a.n_records)
        gpu_ctx.bam_merge([s], sort=True)
        gpu_ctx.bam_merge([a, a], sort=False, compress=True)
        assert (s.sam_text().tobytes(), a.sam_text().tobytes(), s.n_records, a.n_records) == before


def test_combined_mapper(gpu_ctx, tmp_path, monkeypatch):
    from nanopore_amd.analyses import utils
    from nanopore_amd.mappers.bamFileMapper import CombinedBamFile
    monkeypatch.setitem(utils._shared_ctx, 0, gpu_ctx)
    d = tmp_path / "bams" / "2D"
    os.makedirs(str(d))
    for name, data in (("reads.ref.b_second.bam", cases.file_b()), ("reads.ref.a_first.bam", cases.file_a()), ("reads.other.x.bam", cases.file_b())):
        with open(str(d / name), "wb") as fh:
            fh.write(data)
    monkeypatch.setattr(CombinedBamFile, "bamDir", str(tmp_path / "bams"))
    sam = str(tmp_path / "mapping.sam")
    CombinedBamFile(str(tmp_path / "reads.fastq"), "2D", str(tmp_path / "ref.fasta"), sam, None).run()
    lines = [r["line"] for s in (cases.stream_a(), cases.stream_b()) for r in mref.measured(s)[1]]
    assert open(sam).read() == cases.HEADER_TEXT + "".join(ln + "\n" for ln in lines)
    with pytest.raises(FileNotFoundError) as e:
        CombinedBamFile(str(tmp_path / "none.fastq"), "2D", str(tmp_path / "ref.fasta"), sam, None).run()
    assert "none.ref.*.bam" in str(e.value)
    out = str(tmp_path / "merged.bam")
    counts = utils.mergeBamFiles([str(d / "reads.ref.a_first.bam"), str(d / "reads.ref.b_second.bam")], out, ctx=gpu_ctx)
    assert counts["files"] == 2 and counts["records"] == len(lines)
    assert utils.indexBamFile(out, out + ".again.bai", ctx=gpu_ctx)["bytes"] == os.path.getsize(out + ".bai") and open(out + ".again.bai", "rb").read() == open(out + ".bai", "rb").read()
    utils.sortBamFile(str(d / "reads.ref.a_first.bam"), out, ctx=gpu_ctx)
    assert gzip.decompress(open(out, "rb").read()) == mref.merged([cases.stream_a()], True, _header(cases.HEADER_TEXT, True))[0]


def test_a_region_pileup_makes_the_index_it_lacks(gpu_ctx, sorted_files, tmp_path):
    """pileup_of_bam(region=) / bamDepthFile(region=) on a sorted file without a .bai beside it: the index is made in memory and only the
    blocks it names are inflated; the table is the one the file's own .bai gives.  An unsorted file has no index: it is restricted whole."""
    from nanopore_amd.analyses import utils
    from nanopore_amd.analyses.pileup import pileup_of_bam, region_index
    region = (0, 100000, 103000)
    data = open(sorted_files["compressed"], "rb").read()
    bare = str(tmp_path / "bare.bam")
    with open(bare, "wb") as fh:
        fh.write(data)
    tables, blocks = [], []
    for path in (sorted_files["compressed"], bare, sorted_files["unsorted"]):
        _, _, pileup = pileup_of_bam(gpu_ctx, path, region=region)
        try:
            tables.append(pileup.counts())
        finally:
            pileup.close()
        blocks.append(bam.inflate_last(gpu_ctx)["blocks"])
    assert np.array_equal(tables[0], tables[1]) and np.array_equal(tables[0], tables[2]) and tables[0].any()
    assert blocks[1] == blocks[0] < len(rc.bgzf_blocks(data)) and blocks[2] == len(rc.bgzf_blocks(open(sorted_files["unsorted"], "rb").read()))
    assert region_index(bare, region, ctx=gpu_ctx).tobytes() == open(sorted_files["compressed"] + ".bai", "rb").read()
    assert region_index(sorted_files["unsorted"], region, ctx=gpu_ctx) is None and region_index(bare, None, ctx=gpu_ctx) is None and not os.path.exists(bare + ".bai")
    utils.bamDepthFile(bare, bare + ".depth", ctx=gpu_ctx, region=region)
    utils.bamDepthFile(sorted_files["compressed"], bare + ".depth2", ctx=gpu_ctx, region=region)
    assert open(bare + ".depth").read() == open(bare + ".depth2").read() != ""

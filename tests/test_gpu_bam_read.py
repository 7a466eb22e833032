"""npr_bam_sam through Context.bam_to_sam (csrc/npr_inflate.hip, csrc/npr_bamread.hip): the SAM text of tests/test_gpu_bam.py -- with the
records of 65 535 / 65 536 / 70 000 cigar operations, the record that ends on a block edge and the 70 001-base record -- written as four
BAM files (stored, compressed; sorted, unsorted) and read back: header and lines against the specification's decoder
(tests/bam_reference.py bam_decode), the fixed point through sam_to_bam(sort=False), the same stream re-blocked by zlib at uneven member
sizes, the refusals (each leaving no file), and the BamFile mapper through the pipeline driver."""
import os
import struct
import zlib

import numpy as np
import pytest

import bam_reference as ref
import bgzf_deflate_reference as dref
import inflate_cases as cases
from test_gpu_bam import HEADER, _sam_text

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from nanopore_amd import realign
    c = realign.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def files(ctx, tmp_path_factory):
    d = tmp_path_factory.mktemp("bamread")
    sam = str(d / "in.sam")
    with open(sam, "w") as fh:
        fh.write(HEADER + "\n".join(_sam_text()) + "\n")
    out = {}
    for compress in (False, True):
        for sort in (False, True):
            path = str(d / ("%s_%s.bam" % ("compressed" if compress else "stored", "sorted" if sort else "unsorted")))
            ctx.sam_to_bam(sam, path, sort=sort, index=False, compress=compress)
            data = open(path, "rb").read()
            stream = (dref if compress else ref).bgzf_read(data)[0]
            out[(compress, sort)] = dict(path=path, data=data, stream=stream, decoded=ref.bam_decode(stream))
    return dict(dir=d, bams=out)


def _split(text, header):
    assert text.startswith(header)
    body = text[len(header):]
    assert body == "" or body.endswith("\n")
    return body.split("\n")[:-1]


@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("sort", (False, True))
def test_header_and_lines_are_the_decoders(ctx, files, compress, sort):
    f = files["bams"][(compress, sort)]
    text, refs, records = f["decoded"]
    sam = f["path"] + ".sam"
    counts = ctx.bam_to_sam(f["path"], sam)
    got = open(sam).read()
    lines = _split(got, text)
    want = [r["line"] for r in records]
    assert len(lines) == len(want) == 64
    for a, b in zip(lines, want):
        assert a == b, (a[:200], b[:200])
    blocks = len((dref if compress else ref).bgzf_read(f["data"])[1])
    assert counts == {"records": len(want), "references": len(refs), "bytes": len(got), "stream_bytes": len(f["stream"]), "blocks": blocks}
    assert not os.path.exists(sam + ".tmp")
    # the fixed point: the produced SAM gives the original file's stream byte for byte.  (The writer names its own `sort` argument in @HD SO:,
    # so the SAM of a sorted file goes back with sort=True -- a stable sort of sorted records moves nothing --, the other with sort=False.)
    back = sam + ".bam"
    ctx.sam_to_bam(sam, back, sort=sort, index=False, compress=False)
    assert ref.bgzf_read(open(back, "rb").read())[0] == f["stream"]


def test_the_stream_reblocked_with_zlib_at_uneven_member_sizes(ctx, files):
    from nanopore_amd import bam
    f = files["bams"][(False, True)]
    stream = f["stream"]
    rng = np.random.default_rng(9)
    parts, at = [], 0
    while at < len(stream):   # members of 1 .. 65 280 bytes that split records anywhere, an empty one among them
        n = int(rng.integers(1, 65281)) if len(parts) != 3 else 0
        parts.append(stream[at:at + n])
        at += n
    data = b"".join(cases.block(cases.WAYS["level 6"](p), len(p), zlib.crc32(p)) for p in parts) + cases.EOF_BLOCK
    text, n = bam.bam_sam(ctx, data)
    assert n == 64 and _split(text.tobytes().decode(), f["decoded"][0]) == [r["line"] for r in f["decoded"][2]]
    assert bam.inflate_last(ctx)["blocks"] == len(parts)


def _as_file(stream):
    return b"".join(cases.block(cases.WAYS["level 1"](stream[at:at + 65280]), len(stream[at:at + 65280]), zlib.crc32(stream[at:at + 65280]))
                    for at in range(0, len(stream), 65280)) + cases.EOF_BLOCK


def test_refusals_leave_no_file(ctx, files):
    from nanopore_amd import _lib
    f = files["bams"][(False, False)]
    stream = bytearray(f["stream"])
    records = f["decoded"][2]
    first, second = records[0]["u0"], records[1]["u0"]
    n_ref = len(f["decoded"][1])
    bad = {}
    b = bytearray(stream)
    b[3] = 2
    bad["bad BAM magic"] = b
    b = bytearray(stream)
    last = records[-1]["u0"]
    b[last:last + 4] = struct.pack("<i", records[-1]["u1"] - last - 4 + 1)
    bad["a record running past the stream"] = b
    bad["a stream cut inside a record"] = bytearray(stream[:records[-1]["u1"] - 5])
    b = bytearray(stream)
    b[second + 12] = 0
    bad["l_read_name 0"] = b
    b = bytearray(stream)
    b[first + 4:first + 8] = struct.pack("<i", n_ref)
    bad["refID equal to n_ref"] = b
    b = bytearray(stream)
    b[second + 24:second + 28] = struct.pack("<i", -2)
    bad["next_refID -2"] = b
    b = bytearray(stream)
    b[second:second + 4] = struct.pack("<i", 32)
    bad["block_size 32"] = b
    for name, image in bad.items():
        path = str(files["dir"] / "bad.bam")
        with open(path, "wb") as fh:
            fh.write(_as_file(bytes(image)))
        with pytest.raises(_lib.NprError) as e:
            ctx.bam_to_sam(path, path + ".sam")
        assert e.value.code == _lib.ERR_INVALID, name
        assert not os.path.exists(path + ".sam") and not os.path.exists(path + ".sam.tmp"), name
    # a block that does not inflate: the CRC of the first block
    data = bytearray(files["bams"][(True, False)]["data"])
    size = struct.unpack("<H", data[16:18])[0] + 1
    data[size - 8] ^= 1
    path = str(files["dir"] / "crc.bam")
    with open(path, "wb") as fh:
        fh.write(bytes(data))
    with pytest.raises(_lib.NprError):
        ctx.bam_to_sam(path, path + ".sam")
    assert not os.path.exists(path + ".sam")
    # capacity: nothing written
    image = np.frombuffer(files["bams"][(True, True)]["data"], np.uint8)
    total = ctx._L.npr_bam_sam(ctx._h, _lib.ptr(image), len(image), None, 0, None)
    assert total > len(files["bams"][(True, True)]["decoded"][0])
    out = np.full(total, 0xa5, np.uint8)
    assert ctx._L.npr_bam_sam(ctx._h, _lib.ptr(image), len(image), _lib.ptr(out), total - 1, None) == _lib.ERR_CAPACITY and (out == 0xa5).all()


def test_a_header_alone_and_no_header_text(ctx):
    from nanopore_amd import bam
    for text, refs in ((b"@SQ\tSN:a\tLN:5\n", [(b"a", 5)]), (b"", [])):
        stream = b"BAM\1" + struct.pack("<i", len(text)) + text + struct.pack("<i", len(refs))
        for name, ln in refs:
            stream += struct.pack("<i", len(name) + 1) + name + b"\0" + struct.pack("<i", ln)
        got, n = bam.bam_sam(ctx, _as_file(stream))
        assert n == 0 and got.tobytes() == text


def test_bam_file_realign_through_the_pipeline_driver(ctx, tmp_path):
    """BamFileRealign, fed the BAM that SeedMapperChain's SAM converts to, writes the mapping.sam that realigning that SAM writes.  (The
    BAM writer puts an @HD line in front of a header that has none: @HD lines are left out of the comparison.)"""
    from nanopore_amd import pipeline
    from nanopore_amd.mappers.abstractMapper import AbstractMapper
    from test_gpu_pipeline_driver import _experiment, _processed, _working_dir
    work = _working_dir(tmp_path / "work")
    assert pipeline.main([work, "--mappers", "SeedMapperChain", "--analyses", "", "--metaAnalyses", ""]) == 0
    chained = os.path.join(_experiment(work, "SeedMapperChain"), "mapping.sam")
    bam_dir = tmp_path / "bams"
    os.makedirs(str(bam_dir / "2D"))
    with pytest.raises(RuntimeError) as e:   # no file yet: FileNotFoundError names the path
        pipeline.main([work, "--mappers", "BamFileRealign", "--analyses", "", "--metaAnalyses", "", "--bamDir", str(bam_dir)])
    assert "FileNotFoundError" in str(e.value) and str(bam_dir / "2D" / "reads.reference.bam") in str(e.value)
    ctx.sam_to_bam(chained, str(bam_dir / "2D" / "reads.reference.bam"), sort=False, index=False, compress=True)
    assert pipeline.main([work, "--mappers", "BamFileRealign", "--analyses", "", "--metaAnalyses", "", "--bamDir", str(bam_dir)]) == 0
    got = open(os.path.join(_experiment(work, "BamFileRealign"), "mapping.sam")).read().split("\n")
    fq, fa = _processed(work)
    direct = str(tmp_path / "direct.sam")
    with open(direct, "w") as fh:
        fh.write(open(chained).read())
    m = AbstractMapper(fq, "2D", fa, direct)
    try:
        m.realignSamFile()
        m.runFollowOns()
    finally:
        m.cleanup()
    want = open(direct).read().split("\n")
    strip = lambda lines: [ln for ln in lines if not ln.startswith("@HD")]
    assert len(strip(got)) > 2 and strip(got) == strip(want)

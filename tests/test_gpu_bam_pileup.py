"""The records of a BAM file into a pileup where they lie on the device (include/nprealign.h: npr_bam_open, npr_pileup_add_bam;
csrc/npr_bampile.hip, csrc/npr_bamrec.h; Context.bam_open, Pileup.add_bam, analyses/pileup.py pileup_of_bam, analyses/utils.py bamDepthFile):
every word at every position and the four counts against the restated rules (tests/bam_pileup_reference.py) on the constructed files of
tests/bam_pileup_cases.py, and word for word against the route that exists -- the SAM text through pileup_of_sam -- on a SAM file converted
by the device's own BAM writer.  Counts are integers: every comparison is exact."""
import ctypes as C
import os

import numpy as np
import pytest

import bam_pileup_cases
import bam_pileup_reference as bp
from nanopore_amd import _lib
from nanopore_amd.realign import NprError

pytestmark = pytest.mark.gpu

CASES = bam_pileup_cases.cases()
KEYS = ("records", "selected", "added", "refused")


@pytest.fixture(scope="module")
def expected():
    """name -> (table, counts): the reference, computed once and never changed"""
    out = {}
    for name, c in CASES.items():
        table, counts, _ = bp.pileup(c["stream"])
        table.setflags(write=False)
        out[name] = (table, counts)
    return out


def _add(pileup, stream, **kw):
    """add_bam -> (the counts, whether it raised for a refused record)"""
    try:
        return pileup.add_bam(stream, **kw), False
    except NprError as e:
        assert e.code == _lib.ERR_INVALID
        return pileup.last_bam_counts, True


@pytest.mark.parametrize("name", sorted(CASES))
def test_constructed_cases_equal_the_restated_rules(gpu_ctx, expected, name):
    c = CASES[name]
    want, want_counts = expected[name]
    with gpu_ctx.bam_open(c["file"]) as stream:
        assert stream.references == [n for n, _ in c["refs"]] and stream.lengths.tolist() == [ln for _, ln in c["refs"]]
        assert stream.n_records == len(c["records"]) and stream.stream_bytes == len(c["stream"])
        pileup = gpu_ctx.pileup(stream.lengths)
        try:
            counts, raised = _add(pileup, stream)
            print(name, counts)
            assert counts == want_counts and raised == (want_counts["refused"] > 0)
            got = pileup.counts()
            assert got.dtype == np.int32 and got.shape == want.shape
            assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        finally:
            pileup.close()


def test_another_flag_mask(gpu_ctx):
    c = CASES["not selected"]
    for mask in (0, 0x10, 0x800):
        want, want_counts, _ = bp.pileup(c["stream"], flag_mask=mask)
        with gpu_ctx.bam_open(c["file"]) as stream:
            pileup = gpu_ctx.pileup(stream.lengths)
            try:
                assert pileup.add_bam(stream, flag_mask=mask) == want_counts
                assert np.array_equal(pileup.counts(), want)
            finally:
                pileup.close()


# ---------------------------------------------------------------- against the SAM route
REFS = [("contig_a", 5000), ("contig_b", 3000)]


def _sam_lines():
    """About 200 records of M I D S H operations on two references: both strands, unmapped (with and without a reference), secondary,
    duplicate and supplementary ones, bases outside ACGT."""
    rng = np.random.default_rng(77)
    lines = []
    for k in range(200):
        name, length = REFS[int(rng.integers(0, 2))]
        runs = []
        for j in range(int(rng.integers(1, 40))):
            if j:
                runs += [["%dI"], ["%dD"], ["%dI", "%dD"], ["%dD", "%dI"], ["%dI", "%dI"]][int(rng.integers(0, 5))]
            runs.append("%dM")
        if rng.integers(0, 5) == 0:
            runs.insert(0, "%dI")
        if rng.integers(0, 5) == 0:
            runs.append("%dI")
        runs = [r % int(rng.integers(1, 30 if r == "%dM" else 5)) for r in runs]
        head = [["%dH" % rng.integers(1, 9)], ["%dS" % rng.integers(1, 9)], ["%dH" % rng.integers(1, 9), "%dS" % rng.integers(1, 9)], []][int(rng.integers(0, 4))]
        tail = [["%dH" % rng.integers(1, 9)], ["%dS" % rng.integers(1, 9)], ["%dS" % rng.integers(1, 9), "%dH" % rng.integers(1, 9)], []][int(rng.integers(0, 4))]
        cigar = "".join(head + runs + tail)
        words = bp.cigar_words(cigar)
        span, l_seq = bp.consumed(words, bp.REF_OPS), bp.consumed(words, bp.READ_OPS)
        pos = int(rng.integers(0, length - span + 1)) if k % 17 else length - span   # some end with their sequence
        seq = "".join("ACGTN"[c] for c in rng.choice(5, size=l_seq, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
        flag = [0, 16, 0, 16, 0x100, 0x110, 0x400, 0x800, 0x810, 0x200][k % 10]
        lines.append("\t".join(["r%d" % k, str(flag), name, str(pos + 1), "30", cigar, "*", "0", "0", seq, "*"]))
    for k in range(6):
        seq = "".join("ACGT"[c] for c in rng.integers(0, 4, 20))
        lines.append("\t".join(["u%d" % k, "4", "*", "0", "0", "*", "*", "0", "0", seq, "*"]))
        # (an unmapped record placed on a reference keeps a cigar here: the SAM route's reader takes no "*" beside an RNAME)
        lines.append("\t".join(["p%d" % k, "20", "contig_b", str(100 + k), "0", "20M", "*", "0", "0", seq, "*"]))
    order = rng.permutation(len(lines))
    return [lines[i] for i in order]


@pytest.fixture(scope="module")
def sam_route(gpu_ctx, tmp_path_factory):
    from nanopore_amd.analyses.pileup import depth_text, pileup_of_sam
    d = tmp_path_factory.mktemp("bampile")
    sam, fa = str(d / "in.sam"), str(d / "ref.fa")
    rng = np.random.default_rng(5)
    with open(fa, "w") as fh:
        for name, length in REFS:
            fh.write(">%s\n%s\n" % (name, "".join("ACGT"[c] for c in rng.integers(0, 4, length))))
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.4\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in REFS) + "\n".join(_sam_lines()) + "\n")
    names, lengths, pileup = pileup_of_sam(gpu_ctx, sam, fa)
    try:
        table = pileup.counts()
        depth, covered = pileup.depth()
    finally:
        pileup.close()
    table.setflags(write=False)
    assert names == [n for n, _ in REFS] and table[:, :5].sum() > 10000 and table[:, 5].any() and table[:, 6].any()
    return dict(dir=d, sam=sam, fa=fa, table=table, depth_text=depth_text(names, lengths, depth, covered))


@pytest.mark.parametrize("how", ("stored", "compressed", "unsorted"))
def test_a_converted_sam_file_equals_the_sam_route(gpu_ctx, sam_route, how):
    from nanopore_amd.analyses import utils
    from nanopore_amd.analyses.pileup import pileup_of_bam
    path = str(sam_route["dir"] / (how + ".bam"))
    gpu_ctx.sam_to_bam(sam_route["sam"], path, sort=how != "unsorted", index=False, compress=how == "compressed")
    names, lengths, pileup = pileup_of_bam(gpu_ctx, path, sam_route["fa"])
    try:
        assert names == [n for n, _ in REFS] and lengths.tolist() == [ln for _, ln in REFS]
        assert pileup.last_bam_counts["records"] == 212 and pileup.last_bam_counts["refused"] == 0
        assert pileup.last_bam_counts["selected"] == pileup.last_bam_counts["added"] == 200 * 6 // 10
        got = pileup.counts()
        assert np.array_equal(got, sam_route["table"]), np.argwhere(got != sam_route["table"])[:10]
    finally:
        pileup.close()
    assert utils.bamDepthFile(path, path + ".depth", ctx=gpu_ctx) == len(sam_route["depth_text"])
    assert open(path + ".depth").read() == sam_route["depth_text"]


def test_the_fasta_file_must_hold_the_headers_sequences(gpu_ctx, sam_route, tmp_path):
    from nanopore_amd.analyses.pileup import pileup_of_bam
    path = str(tmp_path / "x.bam")
    gpu_ctx.sam_to_bam(sam_route["sam"], path, sort=False, index=False)
    fa = str(tmp_path / "short.fa")
    with open(fa, "w") as fh:
        fh.write(">contig_a\n%s\n>contig_b\n%s\n" % ("A" * 5000, "C" * 2999))
    with pytest.raises(ValueError):
        pileup_of_bam(gpu_ctx, path, fa)
    with open(fa, "w") as fh:
        fh.write(">contig_a\n%s\n" % ("A" * 5000))
    with pytest.raises(KeyError):
        pileup_of_bam(gpu_ctx, path, fa)


# ---------------------------------------------------------------- accumulation, mismatches, refusals
def test_two_files_and_one_stream_twice_accumulate(gpu_ctx, expected):
    one, two = CASES["other operations"], CASES["insertion rule"]
    want = expected["other operations"][0] + expected["insertion rule"][0]
    pileup = gpu_ctx.pileup([3000])
    try:
        with gpu_ctx.bam_open(one["file"]) as a, gpu_ctx.bam_open(two["file"]) as b:
            pileup.add_bam(a)
            assert np.array_equal(pileup.counts(), expected["other operations"][0])   # (read in between: more may follow)
            pileup.add_bam(b)
            assert np.array_equal(pileup.counts(), want)
            assert pileup.add_bam(a) == expected["other operations"][1]
            pileup.add_bam(b)
            assert np.array_equal(pileup.counts(), 2 * want)
    finally:
        pileup.close()


@pytest.mark.parametrize("lengths", ([500, 700, 301], [500, 700], [500, 700, 300, 1]))
def test_a_header_that_is_not_the_pileups_adds_nothing(gpu_ctx, lengths):
    with gpu_ctx.bam_open(CASES["several sequences"]["file"]) as stream:
        pileup = gpu_ctx.pileup(lengths)
        try:
            with pytest.raises(NprError) as e:
                pileup.add_bam(stream)
            assert e.value.code == _lib.ERR_INVALID and pileup.last_bam_counts == dict.fromkeys(KEYS, 0)
            assert not pileup.counts().any()
        finally:
            pileup.close()


def test_objects_of_two_contexts(gpu_ctx):
    from nanopore_amd import realign
    other = realign.Context(0)
    try:
        pileup = other.pileup([3000])
        with gpu_ctx.bam_open(CASES["insertion rule"]["file"]) as stream:
            with pytest.raises(NprError) as e:
                pileup.add_bam(stream)
            assert e.value.code == _lib.ERR_INVALID and not pileup.counts().any()
    finally:
        other.close()


def test_a_refused_block_or_record_gives_no_object(gpu_ctx):
    from nanopore_amd import bam
    L = gpu_ctx._L

    def opened(image):
        data, h = np.frombuffer(image, dtype=np.uint8), C.c_void_p()
        rc = L.npr_bam_open(gpu_ctx._h, _lib.ptr(data), len(data), C.byref(h))
        assert (rc == _lib.OK) == bool(h)
        if h:
            L.npr_bam_close(h)
        return rc

    c = CASES["cigar lengths"]   # (members of 777 bytes: several blocks)
    assert opened(c["file"]) == _lib.OK
    image = bytearray(c["file"])
    second = int.from_bytes(image[16:18], "little") + 1
    size = int.from_bytes(image[second + 16:second + 18], "little") + 1
    image[second + size - 8] ^= 1   # the CRC-32 of the second block
    assert opened(bytes(image)) == _lib.ERR_INVALID
    last = bam.inflate_last(gpu_ctx)
    assert last["failed_block"] == 1 and last["status"] != 0 and last["reason"] != "unknown"
    with pytest.raises(NprError) as e:
        bam.bam_sam(gpu_ctx, bytes(image))
    assert e.value.code == _lib.ERR_INVALID and bam.inflate_last(gpu_ctx)["failed_block"] == 1 and bam.inflate_last(gpu_ctx)["status"] == last["status"]
    with pytest.raises(NprError):
        gpu_ctx.bam_open(bytes(image))
    assert opened(c["file"][:-28]) == _lib.ERR_INVALID            # no end-of-file block
    stream = bytearray(c["stream"])
    stream[3] = 2
    assert opened(bp.bgzf(bytes(stream))) == _lib.ERR_INVALID     # the magic
    stream = bytearray(c["stream"])
    at = bp.header_end(c["stream"])
    stream[at + 12] = 0                                           # l_read_name 0
    assert opened(bp.bgzf(bytes(stream))) == _lib.ERR_INVALID
    assert opened(bp.bgzf(c["stream"][:-3])) == _lib.ERR_INVALID  # a stream cut inside its last record

"""The read-quality tables on the device (include/nprealign.h: npr_read_quality; csrc/npr_readqual.hip) and the FastQC analysis built
on them: every table equal, count for count, to the numpy restatement of the header's definitions (tests/read_quality_reference.py)."""
import os

import numpy as np
import pytest

import read_quality_reference as ref
from nanopore_amd import _lib, ingest
from nanopore_amd.realign import NprError, ReadQuality

pytestmark = pytest.mark.gpu

TILE = ReadQuality.TILE   # positions of one read a workgroup takes per step
LENGTHS = [0, 1, 15, 16, 17, 31, 32, 33, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 3, 70001]
NAMES = ReadQuality.FIELDS


def _read(rng, n, bases="ACGTACGTACGTNacgtn", q_lo=35, q_hi=75):
    """n bases and n quality bytes that cluster, as a sequencer's do: a slow random walk inside [q_lo, q_hi]"""
    s = np.frombuffer(bases.encode(), dtype=np.uint8)[rng.integers(0, len(bases), size=n)]
    q = np.clip(55 + np.cumsum(rng.integers(-2, 3, size=n)) % 40 - 20, q_lo, q_hi).astype(np.uint8)
    return s.tobytes(), q.tobytes()


_shared = {}


def _length_reads():
    if "reads" not in _shared:
        rng = np.random.default_rng(11)
        _shared["reads"] = [_read(rng, n) for n in LENGTHS]
    return _shared["reads"]


def _compare(got, want, what=""):
    for name, g, w in zip(NAMES, got.arrays(), want):
        assert g.dtype == np.int64 and g.shape == w.shape, (what, name)
        assert np.array_equal(g, w), (what, name, np.argwhere(g != w)[:5].tolist())


def _both(ctx, reads, group=None, n_groups=1):
    text, seq, qual = ref.fastq_text(reads)
    group = [0] * len(reads) if group is None else group
    return ctx.read_quality(text, seq, qual, group, n_groups), ref.tables(text, seq, qual, group, n_groups)


def test_lengths_around_every_bin_and_tile_edge_in_one_call(gpu_ctx):
    got, want = _both(gpu_ctx, _length_reads())
    _shared["first"] = got
    _compare(got, want)
    assert got.totals[0].tolist()[:4] == [len(LENGTHS), sum(LENGTHS), 0, 70001] and got.totals[0, 6] == 1
    assert got.pos_qual.sum() == got.pos_base.sum() == sum(LENGTHS) and got.len_hist.sum() == len(LENGTHS)


@pytest.mark.parametrize("k", range(len(LENGTHS)), ids=[str(n) for n in LENGTHS])
def test_each_length_alone(gpu_ctx, k):
    got, want = _both(gpu_ctx, [_length_reads()[k]])
    _compare(got, want, LENGTHS[k])


def test_repeatable(gpu_ctx):
    first = _shared.get("first") or _both(gpu_ctx, _length_reads())[0]
    again = _both(gpu_ctx, _length_reads())[0]
    for a, b in zip(first.arrays(), again.arrays()):
        assert np.array_equal(a, b)


def test_worst_same_address_case(gpu_ctx):
    got, want = _both(gpu_ctx, [(b"A" * 5000, b"I" * 5000)])
    _compare(got, want)
    assert got.pos_qual[0, :, 40].sum() == 5000 == got.pos_base[0, :, 0].sum() and got.meanq_hist[0, 40] == 1 and got.gc_hist[0, 0] == 1


def test_every_quality_byte_and_letter(gpu_ctx):
    q = bytes(range(33, 127)) + bytes([32, 127, 200])
    s = (b"acgtnACGTNRYKMSWBDHVryk.-*" * 4)[:len(q)]
    clean = bytes(range(33, 127))
    got, want = _both(gpu_ctx, [(s, q), (s[:len(clean)], clean), (b"NNNN", b"!!~~")])
    _compare(got, want)
    assert got.totals[0].tolist() == [3, 2 * 94 + 3 + 4, 4, 97, 32, 200, 0, 1]
    assert got.pos_qual[0, :, 94].sum() == 3 and got.meanq_hist[0, 94] == 1 and got.gc_hist[0, 101] == 1


def test_spans_in_reverse_order_with_other_bytes_between(gpu_ctx):
    rng = np.random.default_rng(5)
    reads = [_read(rng, n) for n in (700, 0, 33, TILE + 9, 1)]
    filler, parts, seq, qual, at = b"ACGTIIII!!~~", [], [], [], 0
    for s, q in reads:   # quality first, then the bases, unrelated bytes around both
        parts += [filler, q, filler[:5], s]
        qual.append((at + len(filler), at + len(filler) + len(q)))
        sa = qual[-1][1] + 5
        seq.append((sa, sa + len(s)))
        at = seq[-1][1]
    parts.append(filler)
    text = np.frombuffer(b"".join(parts), dtype=np.uint8)
    seq, qual = np.array(seq[::-1], dtype=np.int64), np.array(qual[::-1], dtype=np.int64)
    got = gpu_ctx.read_quality(text, seq, qual, [0] * len(reads), 1)
    _compare(got, ref.tables(text, seq, qual, [0] * len(reads), 1))
    _compare(got, _both(gpu_ctx, reads)[1])   # the same reads as a plain file


def test_groups_with_an_empty_one_and_reads_left_out(gpu_ctx):
    rng = np.random.default_rng(6)
    reads = [_read(rng, n) for n in (100, 3000, 0, 40, 5000, 17, 64)]
    group = [0, 2, 2, -1, 0, -1, 2]
    got, want = _both(gpu_ctx, reads, group, 3)
    _compare(got, want)
    assert got.totals[1].tolist() == [0, 0, -1, -1, -1, -1, 0, 0] and got.pos_qual[1].sum() == 0 and got.len_hist[1].sum() == 0
    assert got.totals[0, 0] == 2 and got.totals[2, 0] == 3 and got.totals[2, 6] == 1
    only_empty, want = _both(gpu_ctx, [(b"", b""), (b"ACGT", b"IIII")], [1, -1], 2)   # a group with reads and no base
    _compare(only_empty, want)
    assert only_empty.totals[1].tolist() == [1, 0, 0, 0, -1, -1, 1, 0]


def test_empty_call(gpu_ctx):
    got = gpu_ctx.read_quality(np.zeros(0, dtype=np.uint8), np.zeros((0, 2)), np.zeros((0, 2)), [], 2)
    _compare(got, ref.tables(np.zeros(0, dtype=np.uint8), [], [], [], 2))
    assert got.totals.tolist() == [[0, 0, -1, -1, -1, -1, 0, 0]] * 2


def test_rejections_leave_the_tables_alone(gpu_ctx):
    text = np.frombuffer(b"ACGTACGTACIIIIIIIIII", dtype=np.uint8)
    sb, se = np.array([0, 5], dtype=np.int64), np.array([5, 10], dtype=np.int64)
    qb, qe = np.array([10, 15], dtype=np.int64), np.array([15, 20], dtype=np.int64)

    def call(group, n_groups, sb=sb, se=se, qb=qb, qe=qe):
        out = [np.full(8 * words, -7, dtype=np.int64) for words in (336 * 95, 336 * 5, 336, 95, 102, 8)]
        group = np.array(group, dtype=np.int32)
        rc = gpu_ctx._L.npr_read_quality(gpu_ctx._h, 2, _lib.ptr(text), _lib.ptr(sb), _lib.ptr(se), _lib.ptr(qb), _lib.ptr(qe), _lib.ptr(group), n_groups,
                                         *map(_lib.ptr, out))
        return rc, out

    one = np.array([1], dtype=np.int64)
    for kw in (dict(group=[0, 2], n_groups=2), dict(group=[-2, 0], n_groups=2), dict(group=[0, 8], n_groups=8),    # a bad group
               dict(group=[0, 1], n_groups=2, sb=np.array([0, 7], dtype=np.int64), se=np.array([5, 6], dtype=np.int64)),   # a reversed span
               dict(group=[0, -1], n_groups=2, qb=np.array([10, 17], dtype=np.int64), qe=np.array([15, 16], dtype=np.int64)),   # ... of a read left out
               dict(group=[0, 1], n_groups=2, qe=qe - one),   # unequal quality length
               dict(group=[0, 0], n_groups=0), dict(group=[0, 0], n_groups=9)):
        rc, out = call(**kw)
        assert rc == _lib.ERR_INVALID and all((a == -7).all() for a in out), kw
    rc, out = call([0, -1], 2, qe=np.array([15, 19], dtype=np.int64))   # unequal lengths of a read that is left out: legal
    assert rc == _lib.OK and out[5][:16].tolist() == [1, 5, 5, 5, 73, 73, 0, 0, 0, 0, -1, -1, -1, -1, 0, 0] and (out[5][16:] == -7).all()
    for n_groups in (0, 9):
        with pytest.raises(NprError) as e:
            gpu_ctx.read_quality(text, np.stack([sb, se], 1), np.stack([qb, qe], 1), [0, 0], n_groups)
        assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(NprError):
        gpu_ctx.read_quality(text, np.stack([sb, se], 1), np.stack([qb, qe + one], 1), [0, 0], 1)   # past the text: refused before the library sees it


def test_fastqc_analysis_end_to_end(tmp_path, gpu_ctx):
    from helpers import load_model_arrays
    from nanopore_amd import pipeline, synth
    from nanopore_amd.analyses import fastqc
    from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
    T, E, _ = load_model_arrays()
    w = synth.make_workload(77, 40, 300, T, E, flank=20, length_sigma=0.4, len_min=40, len_max=900)
    sam, fa, fq = (str(tmp_path / k) for k in ("mapping.sam", "ref.fa", "reads.fq"))
    _, names = synth.write_workload_files(w, sam, fa, fastq_path=fq)
    lines = open(sam).read().split("\n")
    head, recs = [ln for ln in lines if ln.startswith("@")], [ln for ln in lines if ln and not ln.startswith("@")]
    assert len(recs) == 40
    with open(sam, "w") as f:   # every other read is dropped from the SAM
        f.write("\n".join(head + recs[::2]) + "\n")
    rng = np.random.default_rng(3)
    reads = []
    with open(fq, "wb") as f:   # the same reads with qualities that vary, and one record whose quality line is short
        for i, name in enumerate(names):
            s = np.ascontiguousarray(w["read"][w["read_off"][i]:w["read_off"][i + 1]], dtype=np.uint8).tobytes()
            reads.append((s, _read(rng, len(s), q_lo=36, q_hi=70)[1]))
            f.write(b"@" + name.encode() + b"\n" + s + b"\n+\n" + reads[-1][1] + b"\n")
        f.write(b"@short\nACGTACGT\n+\nIII\n")
    out = tmp_path / "out"
    out.mkdir()
    assert pipeline.resolveClasses("FastQC", "nanopore_amd.analyses", AbstractAnalysis) == [fastqc.FastQC]
    assert fastqc.FastQC not in pipeline.analyses
    fastqc.FastQC(fq, "2D", fa, sam, str(out)).run(ctx=gpu_ctx)
    assert sorted(os.listdir(str(out))) == ["DONE", "fastqc_data.txt", "fastqc_data_mapped.txt", "fastqc_data_unmapped.txt"]
    text, seq, qual = ref.fastq_text(reads)
    group = [i % 2 for i in range(40)]
    both = ReadQuality(*ref.tables(text, seq, qual, group, 2))
    everything = ReadQuality(*[a[0] for a in ref.tables(text, seq, qual, [0] * 40, 1)])
    assert both.totals[0, 0] == 20 == both.totals[1, 0]
    for got, want in zip(fastqc.mergeTables(both.group(0), both.group(1)).arrays(), everything.arrays()):
        assert np.array_equal(got, want)   # the mapped and the unmapped tables sum to the tables of all reads
    for name, tables, malformed in (("fastqc_data.txt", everything, 1), ("fastqc_data_mapped.txt", both.group(0), 0),
                                    ("fastqc_data_unmapped.txt", both.group(1), 1)):
        assert (out / name).read_text() == fastqc.fastqcDataText(tables, "reads.fq", malformed), name
    assert "#Malformed records\t1\n" in (out / "fastqc_data.txt").read_text()

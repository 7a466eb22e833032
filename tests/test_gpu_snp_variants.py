"""SNP variants on the device (include/nprealign.h: npr_snp_variants_table, npr_batch_snp_variants, npr_pileup_snp_variants;
csrc/npr_snpcall.hip: k_snp_variants_count / _scan / _emit) against the numpy restatement of snp_variants_reference.py: the best base and
its quality equal at every row, (row, base) of the calls equal as sequences -- so their order is checked --, posteriors within 1e-12.

The tolerance: a posterior is about twenty fp64 roundings and an `exp` accurate to 2 ulp on arguments of magnitude below 50 away from
the exact value, a relative error below 1e-14; two more orders cover a different contraction of products and sums.
Exact comparison of thresholded and floored values needs inputs away from the edges: every case first asserts, ON THE REFERENCE ALONE and
before the device is called, that no candidate's posterior lies within 1e-9 of the threshold, that the two largest log posteriors of no
row are closer than 1e-9 (the best base), and that no -10 log10(q) lies within 1e-9 of an integer (the quality).  The seeds below were
chosen on the CPU so that this holds for every case; no row is left out of any comparison."""
import ctypes
import os

import numpy as np
import pytest

from helpers import ROOT
from nanopore_amd import _lib
from nanopore_amd.analyses.marginAlignSnpCaller import FLAT_ERROR_MATRIX, NULL_MATRIX, errorMatrixOfHmm
from nanopore_amd.analyses.utils import trainedModelPath
from snp_variants_reference import snp_variants_reference

pytestmark = pytest.mark.gpu

T = 256          # SNP_VARIANT_TILE of csrc/npr_device.h: the rows of one workgroup of the variant kernels
EDGE = 1e-9
P_TOLERANCE = 1e-12
HMM_ERROR_MATRIX = errorMatrixOfHmm(trainedModelPath("blasr_hmm_20.txt"))
GLOBAL_SAM = os.path.join(ROOT, "tests", "golden", "pileup", "global.sam")
GLOBAL_FA = os.path.join(ROOT, "tests", "golden", "pileup", "global.fa")


def mixed_table(seed, rows, variant_share=0.1, variant_rows=None):
    """A seeded table of about thirty-fold evidence with every kind of row: never seen (some with weights all the same), seen without any
    weight, a reference base outside ACGT, the reference base dominant, and -- a share of variant_share, or exactly the rows
    variant_rows -- another base dominant: the rows that call at threshold one half."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(4, size=rows, p=[0.1, 0.05, 0.05, 0.8])   # 0 unseen, 1 no weight, 2 N, 3 ordinary
    ref = np.where(kind == 2, 4, rng.integers(0, 4, size=rows)).astype(np.uint8)
    variant = rng.random(rows) < variant_share if variant_rows is None else np.isin(np.arange(rows), variant_rows)
    dominant = np.where(variant, (ref + rng.integers(1, 4, size=rows)) % 4, ref % 4)
    weights = rng.random((rows, 4)) * 3.0
    weights[np.arange(rows), dominant] += 20.0 + 10.0 * rng.random(rows)
    weights[kind == 1] = 0.0
    weights[(kind == 0) & (rng.random(rows) < 0.5)] = 0.0
    if rows == 1:
        weights[0], kind[0], ref[0] = (1.0, 40.0, 2.0, 0.5), 3, 0
    return weights, kind != 0, ref


def guarded_reference(weights, seen, ref, error, threshold, evolution=None, ties=False):
    want = snp_variants_reference(weights, seen, ref, error, threshold, evolution)
    print("reference: %d rows, %d callable, %d calls; threshold gap %.3g, lp gap %.3g, quality gap %.3g"
          % (len(want["best"]), want["callable"].sum(), len(want["call_row"]), want["threshold_gap"], want["lp_gap"], want["qual_gap"]))
    assert want["threshold_gap"] > EDGE and want["qual_gap"] > EDGE
    assert want["lp_gap"] > EDGE or ties
    return want


def assert_same_variants(got, want):
    best, qual, call_row, call_alt, call_p = got
    assert (best.dtype, qual.dtype, call_row.dtype, call_alt.dtype, call_p.dtype) == (np.uint8, np.uint8, np.int64, np.uint8, np.float64)
    assert np.array_equal(best, want["best"]), np.flatnonzero(best != want["best"])[:8]
    assert np.array_equal(qual, want["qual"]), np.flatnonzero(qual != want["qual"])[:8]
    assert np.array_equal(call_row, want["call_row"]) and np.array_equal(call_alt, want["call_alt"])
    worst = float(np.abs(call_p - want["call_p"]).max()) if len(call_p) else 0.0
    print("device against reference: %d calls, largest |p_dev - p_ref| %.3g" % (len(call_p), worst))
    assert worst <= P_TOLERANCE


@pytest.mark.parametrize("rows", [1, 63, 64, 65, T, T + 1, 3 * T + 1])
def test_table_variants_equal_the_reference(gpu_ctx, rows):
    weights, seen, ref = mixed_table(300 + rows, rows)
    for error, threshold in ((FLAT_ERROR_MATRIX, 0.0), (FLAT_ERROR_MATRIX, 1.0), (HMM_ERROR_MATRIX, 0.5)):
        want = guarded_reference(weights, seen, ref, error, threshold)
        n_callable = int(want["callable"].sum())
        if threshold == 0.0:     # three calls on every callable row
            assert len(want["call_row"]) == 3 * n_callable
        elif threshold == 1.0:   # none: zero-length arrays
            assert len(want["call_row"]) == 0
        elif rows > 64:          # about one row in ten
            assert 0.04 * rows < len(np.unique(want["call_row"])) < 0.2 * rows
        if rows > 64:
            assert 0 < n_callable < rows and (~np.asarray(seen)).any() and (ref == 4).any()
        got = gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, error, threshold)
        assert_same_variants(got, want)
        if threshold == 1.0:
            assert all(a.shape == (0,) for a in got[2:])


def test_calls_of_the_middle_tile_alone_and_an_impossible_candidate(gpu_ctx):
    """3 T + 1 rows whose only calls lie in the second tile: its offset is behind an empty tile, and two empty tiles follow."""
    rows = 3 * T + 1
    weights, seen, ref = mixed_table(77, rows, variant_rows=np.arange(T + 3, 2 * T - 1, 5))
    want = guarded_reference(weights, seen, ref, HMM_ERROR_MATRIX, 0.5)
    assert len(want["call_row"]) > 30 and want["call_row"].min() >= T and want["call_row"].max() < 2 * T
    assert_same_variants(gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5), want)
    # zeros in the evolution matrix: those candidates have p = 0 and are never the best base
    evolution = np.array([[0.97, 0.01, 0.01, 0.01], [0.0, 1.0, 0.0, 0.5], [0.2, 0.2, 0.4, 0.2], [0.01, 0.0, 0.01, 0.98]])
    want = guarded_reference(weights, seen, ref, HMM_ERROR_MATRIX, 0.3, evolution)
    assert len(want["call_row"]) > 0
    assert_same_variants(gpu_ctx.snp_variants_table(weights, seen, ref, evolution, HMM_ERROR_MATRIX, 0.3), want)


def test_exact_ties_go_to_the_reference_base_else_to_the_lowest_code(gpu_ctx):
    """All weight on one observed base, two candidates with the same entry for it, a flat evolution: the two lp are the same number in
    any arithmetic (one product by 1.0, sums with zeros), so the rule for equal lp is tested without a tolerance."""
    error = np.array([[0.7, 0.1, 0.1, 0.1], [0.1, 0.3, 0.2, 0.4], [0.1, 0.2, 0.3, 0.4], [0.25, 0.25, 0.25, 0.25]])
    weights = np.tile([0.0, 0.0, 0.0, 7.0], (70, 1))
    ref = (np.arange(70) % 3).astype(np.uint8)[::-1].copy()   # G and C: among the tied; A: not
    seen = np.ones(70, dtype=bool)
    want = guarded_reference(weights, seen, ref, error, 0.3, ties=True)
    assert want["lp_gap"] == 0.0 and set(want["best"][ref == 2]) == {2} and set(want["best"][ref == 1]) == {1} and set(want["best"][ref == 0]) == {1}
    assert_same_variants(gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, error, 0.3), want)


def test_pileup_variants_equal_the_reference_on_the_counts(gpu_ctx):
    from nanopore_amd import ingest
    from nanopore_amd.analyses.pileup import pileup_of_sam
    names, lengths, pileup = pileup_of_sam(gpu_ctx, GLOBAL_SAM, GLOBAL_FA)
    try:
        fasta = ingest.FastaTable(GLOBAL_FA)
        ref = np.concatenate([_codes(fasta, name) for name in names])
        counts = pileup.counts()
        seen = counts[:, :5].sum(axis=1) > 0
        want = guarded_reference(counts[:, :4], seen, ref, HMM_ERROR_MATRIX, 0.5)
        assert want["callable"].sum() > 300 and len(want["call_row"]) > 0 and not seen.all()
        assert_same_variants(pileup.snp_variants(ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5), want)
        assert np.array_equal(pileup.counts(), counts)
    finally:
        pileup.close()


def _codes(fasta, name):
    code = np.full(256, 4, dtype=np.uint8)
    for k, c in enumerate(b"ACGT"):
        code[c] = code[c + 32] = k
    k = fasta.index[name]
    return code[np.asarray(fasta.seq[fasta.off[k]:fasta.off[k + 1]])]


def test_batch_variants_equal_the_reference_on_the_fetched_expectations(gpu_ctx):
    from test_gpu_snp_calls import _stage_small_batch
    batch, ref_lengths, ref_code, _ = _stage_small_batch(gpu_ctx)
    try:
        batch.run(), batch.finish()
        assert (batch.results()["status"] == 0).all()
        use = (np.random.default_rng(2).random(20) < 0.5).astype(np.uint8)
        expect, seen = batch.base_expectations(ref_lengths, use=use)
        want = guarded_reference(expect, seen, ref_code, HMM_ERROR_MATRIX, 0.5)
        assert want["callable"].sum() > 300 and 0 < len(want["call_row"]) < 100
        assert_same_variants(batch.snp_variants(ref_lengths, ref_code, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5, use=use), want)
        again, _ = batch.base_expectations(ref_lengths, use=use)   # the call left the batch as it was
        assert np.array_equal(again, expect)
    finally:
        batch.close()


def _raw_table_call(ctx, weights, seen8, ref, evolution, error, threshold, cap):
    """npr_snp_variants_table itself, every output filled with 0x5a first -> (return value, n_calls, best, qual, row, alt, p)."""
    rows = len(weights)
    best, qual = np.full(rows, 0x5a, dtype=np.uint8), np.full(rows, 0x5a, dtype=np.uint8)
    size = max(cap, 8)
    row, alt, p = np.full(size, 0x5a5a5a5a, dtype=np.int64), np.full(size, 0x5a, dtype=np.uint8), np.full(size, -7.0)
    n = ctypes.c_int64(-77)
    evolution, error = np.ascontiguousarray(evolution, dtype=np.float64), np.ascontiguousarray(error, dtype=np.float64)
    rc = _lib.load().npr_snp_variants_table(ctx._h, rows, _lib.ptr(weights), _lib.ptr(seen8), _lib.ptr(ref), _lib.ptr(evolution), _lib.ptr(error),
                                            threshold, _lib.ptr(best), _lib.ptr(qual), _lib.ptr(row), _lib.ptr(alt), _lib.ptr(p), cap, ctypes.byref(n))
    return rc, n.value, best, qual, row, alt, p


def test_capacity_one_short_reports_the_count_and_the_binding_grows_once(gpu_ctx):
    rows = 40 * T   # more calls than the room the binding offers first: rows // 16 + 64
    weights, seen, ref = mixed_table(12, rows, variant_share=0.2)
    want = guarded_reference(weights, seen, ref, HMM_ERROR_MATRIX, 0.5)
    count = len(want["call_row"])
    assert count > rows // 16 + 64
    seen8 = seen.astype(np.uint8)
    rc, n, best, qual, row, alt, p = _raw_table_call(gpu_ctx, weights, seen8, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5, count - 1)
    assert rc == _lib.ERR_CAPACITY and n == count
    assert (row == 0x5a5a5a5a).all() and (alt == 0x5a).all() and (p == -7.0).all()
    assert np.array_equal(best, want["best"]) and np.array_equal(qual, want["qual"])
    rc, n, best, qual, row, alt, p = _raw_table_call(gpu_ctx, weights, seen8, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5, count)
    assert rc == n == count and np.array_equal(row[:count], want["call_row"])
    assert_same_variants(gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.5), want)
    # no rows at all
    empty = gpu_ctx.snp_variants_table(np.zeros((0, 4)), np.zeros(0, dtype=np.uint8), np.zeros(0, dtype=np.uint8), NULL_MATRIX, HMM_ERROR_MATRIX, 0.5)
    assert all(a.shape == (0,) for a in empty)


def test_error_returns_leave_every_output_alone(gpu_ctx):
    weights, seen, ref = mixed_table(5, 40)
    seen8 = seen.astype(np.uint8)
    zero = np.array(HMM_ERROR_MATRIX, dtype=np.float64)
    zero[2, 3] = 0.0
    for error, threshold in ((HMM_ERROR_MATRIX, float("nan")), (HMM_ERROR_MATRIX, -0.1), (HMM_ERROR_MATRIX, 1.5), (zero, 0.5)):
        rc, n, best, qual, row, alt, p = _raw_table_call(gpu_ctx, weights, seen8, ref, NULL_MATRIX, error, threshold, 200)
        assert rc == _lib.ERR_INVALID and n == -77
        assert (best == 0x5a).all() and (qual == 0x5a).all() and (row == 0x5a5a5a5a).all() and (alt == 0x5a).all() and (p == -7.0).all()
    with pytest.raises(_lib.NprError) as e:   # ... and through the binding's checked call
        gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 1.5)
    assert e.value.code == _lib.ERR_INVALID and "npr_snp_variants_table" in str(e.value)
    pileup = gpu_ctx.pileup([40])
    try:
        with pytest.raises(_lib.NprError) as e:
            pileup.snp_variants(ref, NULL_MATRIX, zero, 0.5)
        assert e.value.code == _lib.ERR_INVALID
        best, qual, row, alt, p = pileup.snp_variants(ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.0)   # an empty table: nothing callable
        assert (best == 4).all() and (qual == 0).all() and len(row) == 0
    finally:
        pileup.close()


def test_two_runs_give_the_same_bytes(gpu_ctx):
    weights, seen, ref = mixed_table(31, 9 * T + 17, variant_share=0.3)
    first = gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.2)
    second = gpu_ctx.snp_variants_table(weights, seen, ref, NULL_MATRIX, HMM_ERROR_MATRIX, 0.2)
    assert len(first[2]) > 500
    for a, b in zip(first, second):
        assert a.tobytes() == b.tobytes()


def _parse_outputs(out_dir):
    (vcf,) = [f for f in os.listdir(out_dir) if f.endswith("_Consensus.vcf")]
    (fastq,) = [f for f in os.listdir(out_dir) if f.endswith("_Consensus.fastq")]
    assert vcf[:-len("_Consensus.vcf")] == fastq[:-len("_Consensus.fastq")]
    lines = open(os.path.join(out_dir, fastq)).read().split("\n")
    assert lines[-1] == "" and len(lines) % 4 == 1
    records = [(lines[i][1:], lines[i + 1], lines[i + 3]) for i in range(0, len(lines) - 1, 4)]
    assert all(lines[i][0] == "@" and lines[i + 2] == "+" for i in range(0, len(lines) - 1, 4))
    text = open(os.path.join(out_dir, vcf)).read().split("\n")
    head = [ln for ln in text if ln.startswith("#")]
    calls = [ln.split("\t") for ln in text if ln and not ln.startswith("#")]
    return vcf, head, calls, records


def test_consensus_on_the_golden_pileup(tmp_path, gpu_ctx):
    from nanopore_amd import ingest
    from nanopore_amd.analyses.consensus import Consensus
    from nanopore_amd.analyses.pileup import pileup_of_sam
    out = tmp_path / "analysis_Consensus"
    out.mkdir()
    analysis = Consensus(str(tmp_path / "some.reads.fastq"), "2D", GLOBAL_FA, GLOBAL_SAM, str(out))
    analysis.run(ctx=gpu_ctx)
    analysis.cleanup()
    assert Consensus.isFinished(str(out))
    vcf, head, calls, records = _parse_outputs(str(out))
    assert vcf == "some.reads_global_Consensus.vcf"
    # the reference rule on the counts of a pileup of the same file, sequences in the order of the FASTA file
    fasta = ingest.FastaTable(GLOBAL_FA)
    names, lengths, pileup = pileup_of_sam(gpu_ctx, GLOBAL_SAM, GLOBAL_FA)
    try:
        counts = pileup.counts()
    finally:
        pileup.close()
    first = dict(zip(names, np.concatenate([[0], np.cumsum(lengths)]).tolist()))
    order = sorted(names, key=lambda n: fasta.index[n])
    table = np.concatenate([counts[first[n]:first[n] + len(_codes(fasta, n))] for n in order])
    ref = np.concatenate([_codes(fasta, n) for n in order])
    want = guarded_reference(table[:, :4], table[:, :5].sum(axis=1) > 0, ref, HMM_ERROR_MATRIX, Consensus.threshold)
    assert [r[0] for r in records] == order
    assert "".join(r[1] for r in records) == "".join("ACGTN"[b] for b in want["best"])
    assert "".join(r[2] for r in records) == "".join(chr(33 + q) for q in want["qual"])
    assert "N" in records[0][1] + records[1][1] and len(want["call_row"]) > 0
    assert head[0] == "##fileformat=VCFv4.1" and [h for h in head if h.startswith("##contig")] == ["##contig=<ID=%s,length=%d>" % (n, len(_codes(fasta, n))) for n in order]
    assert sum(h.startswith("##INFO=<ID=PP,") for h in head) == 1
    start = np.concatenate([[0], np.cumsum([len(_codes(fasta, n)) for n in order])])
    which = np.searchsorted(start, want["call_row"], side="right") - 1
    assert [(c[0], int(c[1]), c[3], c[4]) for c in calls] == [(order[k], int(r - start[k]) + 1, "ACGTN"[ref[r]], "ACGT"[a])
                                                               for k, r, a in zip(which, want["call_row"], want["call_alt"])]
    assert all(c[2] == "." and c[6] == "." and c[7].startswith("PP=") for c in calls)
    assert np.abs(np.array([float(c[7][3:]) for c in calls]) - want["call_p"]).max() <= 1e-6
    # QUAL = min(93, floor(-10 log10(1 - p))): from the reference's p, none of which lies within 1e-9 of an edge of the floor
    phred = -10 * np.log10(1 - want["call_p"])
    assert np.abs(phred - np.rint(phred)).min() > EDGE
    assert [int(c[5]) for c in calls] == np.minimum(93, np.floor(phred)).astype(int).tolist()


def test_consensus_through_the_pipeline_driver(tmp_path):
    from nanopore_amd import pipeline
    from nanopore_amd.analyses.abstractAnalysis import AbstractAnalysis
    from test_gpu_pipeline_driver import _experiment, _working_dir
    work = _working_dir(tmp_path / "work")
    assert pipeline.main([work, "--mappers", "SeedMapperChain", "--analyses", "Consensus", "--metaAnalyses", ""]) == 0
    out = os.path.join(_experiment(work, "SeedMapperChain"), "analysis_Consensus")
    assert AbstractAnalysis.isFinished(out)
    assert sorted(os.listdir(out)) == ["DONE", "reads.fq_reference_Consensus.fastq", "reads.fq_reference_Consensus.vcf"]   # (the name up to ".fastq": this file ends in .fq)
    assert all(os.path.getsize(os.path.join(out, f)) > 0 for f in os.listdir(out) if f != "DONE")
    name, bases, quals = _parse_outputs(out)[3][0]
    assert name == "HUMAN" and len(bases) == len(quals) > 50000 and set(bases) <= set("ACGTN") and set(bases) != {"N"}

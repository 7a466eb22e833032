"""SNP calls on the device (include/nprealign.h: npr_snp_calls_table, npr_batch_snp_calls, npr_pileup_snp_calls; csrc/npr_snpcall.hip)
against the numpy oracle of snp_calls_reference.py: exact integer equality of every histogram and counter.

Why equality and not a tolerance: the device and numpy differ in `exp` and in the order of a few fp64 sums, about 1e-13 in 100 p; a call
changes its bin only when 100 p lies that close to k + 0.5.  Every case first asserts, on the oracle alone, that no call lies within
1e-9 of such an edge (the seeds below were chosen on the CPU so that this holds); above that distance the bins must agree."""
import ctypes
import random

import numpy as np
import pytest

from nanopore_amd import _lib, bioio
from nanopore_amd import realign as R
from nanopore_amd.analyses.marginAlignSnpCaller import FLAT_ERROR_MATRIX, NULL_MATRIX, errorMatrixOfHmm
from nanopore_amd.analyses.utils import trainedModelPath
from snp_calls_reference import snp_calls_reference

pytestmark = pytest.mark.gpu

EDGE = 1e-9
HMM_ERROR_MATRIX = errorMatrixOfHmm(trainedModelPath("blasr_hmm_20.txt"))
SHARP_ERROR_MATRIX = np.where(np.eye(4, dtype=bool), 0.997, 0.001)   # one dominant base decides: posteriors at both ends of the histogram
MODELS = {1: (FLAT_ERROR_MATRIX,), 2: (FLAT_ERROR_MATRIX, HMM_ERROR_MATRIX)}


def mixed_table(seed, rows, identical=0):
    """A seeded table with every kind of row: never seen; seen with zero total; a reference base outside ACGT; one dominant base (the
    lowest and highest bins an error matrix reaches); near-uniform weights (the middle bins); truth equal to and different from the reference.  identical: that many copies of one
    row in the middle, which all land on the same three bins."""
    rng = np.random.default_rng(seed)
    kind = rng.choice(5, size=rows, p=[0.1, 0.05, 0.05, 0.4, 0.4])
    weights = np.where((kind == 3)[:, None], rng.random((rows, 4)) * 0.5, 8.0 + rng.random((rows, 4)) * rng.choice([0.5, 4.0, 16.0], size=(rows, 1)))
    weights[kind == 3, rng.integers(0, 4, size=int((kind == 3).sum()))] += rng.integers(20, 60, size=int((kind == 3).sum()))
    weights[kind == 1] = 0.0
    weights[(kind == 0) & (rng.random(rows) < 0.5)] = 0.0
    seen = kind != 0
    ref = np.where(kind == 2, 4, rng.integers(0, 4, size=rows)).astype(np.uint8)
    true = np.where(rng.random(rows) < 0.3, rng.integers(0, 5, size=rows), ref).astype(np.uint8)
    if rows == 1:
        weights[0], seen[0], ref[0], true[0] = (1.0, 40.0, 2.0, 0.5), True, 0, 1
    if identical:
        lo = (rows - identical) // 2
        weights[lo:lo + identical], seen[lo:lo + identical], ref[lo:lo + identical], true[lo:lo + identical] = (3.0, 11.0, 0.25, 6.0), True, 2, 1
    return weights, seen, ref, true


def assert_same_calls(got, want):
    assert len(got) == len(want)
    for (g_true, g_false, g_not, g_rows), (w_true, w_false, w_not, w_rows) in zip(got, want):
        assert g_true.dtype == np.int64 and g_true.shape == (101,) and g_false.shape == (101,)
        assert np.array_equal(g_true, w_true), np.flatnonzero(g_true != w_true)
        assert np.array_equal(g_false, w_false), np.flatnonzero(g_false != w_false)
        assert (g_not, g_rows) == (w_not, w_rows)


TABLE_CASES = [(rows, n_models, 0) for rows in (1, 63, 64, 65, 257, 70001) for n_models in (1, 2)] + [(6000, 2, 5000)]


@pytest.mark.parametrize("rows,n_models,identical", TABLE_CASES)
def test_table_calls_equal_the_oracle(gpu_ctx, rows, n_models, identical):
    weights, seen, ref, true = mixed_table(100 + rows, rows, identical)
    want, edge = snp_calls_reference(weights, seen, ref, true, MODELS[n_models])
    assert edge > EDGE
    if rows >= 257:   # every kind of row is there; near-uniform rows fill the middle bins, rows with one dominant base bins 7 and 80:
        total = want[0][0] + want[0][1]   # the flat matrix gives a candidate at most 0.8 / (0.8 + 3 * 0.2 / 3) whatever the evidence
        assert want[0][2] > 0 and 0 < want[0][3] < rows - want[0][2] and want[0][0].sum() > 0
        assert total[5:9].sum() > 0 and total[78:82].sum() > 0 and total[20:60].sum() > 0
    if identical:
        assert max((w[0] + w[1]).max() for w in want) >= identical
    assert_same_calls(gpu_ctx.snp_calls_table(weights, seen, ref, true, NULL_MATRIX, MODELS[n_models]), want)
    if rows == 257:   # no truth given: the truth is the reference, every call is a false positive; and a zero in the evolution matrix
        want, edge = snp_calls_reference(weights, seen, ref, None, MODELS[n_models])
        assert edge > EDGE and all(w[0].sum() == 0 for w in want)
        assert_same_calls(gpu_ctx.snp_calls_table(weights, seen, ref, None, NULL_MATRIX, MODELS[n_models]), want)
        evolution = np.array([[0.97, 0.01, 0.01, 0.01], [0.0, 1.0, 0.0, 0.5], [0.2, 0.2, 0.4, 0.2], [0.01, 0.0, 0.01, 0.98]])
        want, edge = snp_calls_reference(weights, seen, ref, true, MODELS[n_models], evolution)
        assert edge > EDGE
        assert_same_calls(gpu_ctx.snp_calls_table(weights, seen, ref, true, evolution, MODELS[n_models]), want)
        # four models, the most a call takes; the two sharp ones put the dominant rows into bins 0 and 100
        four = MODELS[2] + (SHARP_ERROR_MATRIX, SHARP_ERROR_MATRIX ** 2 / (SHARP_ERROR_MATRIX ** 2).sum(axis=1, keepdims=True))
        want, edge = snp_calls_reference(weights, seen, ref, true, four)
        assert edge > EDGE and all((w[0] + w[1])[0] > 0 and (w[0] + w[1])[100] > 0 for w in want[2:])
        assert_same_calls(gpu_ctx.snp_calls_table(weights, seen, ref, true, NULL_MATRIX, four), want)


def _stage_small_batch(ctx, mode=R.MODE_ALL_POSTERIORS):
    """About 20 reads of about 400 bases from two reference sequences through the mild channel of the pipeline tests, guides = the true
    paths.  -> (batch, ref_lengths, ref_code, true_code): the staged references differ from the reads' source at a few positions."""
    from nanopore_amd import synth
    from nanopore_amd.hmm import Hmm
    from test_gpu_pipeline import _mild_channel
    ctx.set_hmm(Hmm.loadHmm(trainedModelPath("blasr_hmm_0.txt")))
    rng = np.random.default_rng(21)
    sources = [rng.integers(0, 4, size=n).astype(np.uint8) for n in (390, 431)]
    ref_index = np.arange(20) % 2
    T, E = _mild_channel()
    off = np.concatenate([[0], np.cumsum([len(sources[k]) for k in ref_index])]).astype(np.int64)
    rc, roff, cols, coff = synth.error_channel(rng, np.concatenate([sources[k] for k in ref_index]), off, T, E)
    runs, run_off = synth.columns_to_runs(cols, coff)
    staged = [s.copy() for s in sources]
    for s in staged:
        at = rng.choice(len(s), size=6, replace=False)
        s[at] = (s[at] + rng.integers(1, 4, size=6)) % 4
    staged[1][7] = 4   # a reference base outside ACGT
    refs = ["".join("ACGTN"[c] for c in s) for s in staged]
    reads = ["".join("ACGT"[c] for c in rc[roff[i]:roff[i + 1]]) for i in range(20)]
    guides = [[(int(o), int(n)) for o, n in runs[run_off[i]:run_off[i + 1]]] for i in range(20)]
    P = R.make_params(band_mode=R.BAND_ANCHOR, split_threshold=100, mode=mode, max_pairs_per_base=48)
    batch = ctx.stage(P, refs, reads, guides, ref_index=ref_index)
    return batch, [len(s) for s in staged], np.concatenate(staged), np.concatenate(sources)


def test_batch_calls_equal_the_oracle_on_the_fetched_expectations(gpu_ctx):
    batch, ref_lengths, ref_code, true_code = _stage_small_batch(gpu_ctx)
    try:
        batch.run(), batch.finish()
        assert (batch.results()["status"] == 0).all()
        rng = np.random.default_rng(2)
        for use in ((rng.random(20) < 0.5).astype(np.uint8), (np.arange(20) % 2 == 1).astype(np.uint8)):   # (the second: no read of sequence 0)
            expect, seen = batch.base_expectations(ref_lengths, use=use)
            want, edge = snp_calls_reference(expect, seen, ref_code, true_code, MODELS[2])
            assert edge > EDGE and want[0][3] > 300 and want[0][0].sum() > 0
            assert use[::2].any() or want[0][2] >= ref_lengths[0]   # no read of sequence 0: none of its rows is seen
            assert_same_calls(batch.snp_calls(ref_lengths, ref_code, true_code, NULL_MATRIX, MODELS[2], use=use), want)
            again, _ = batch.base_expectations(ref_lengths, use=use)   # the call left the batch as it was
            assert np.array_equal(again, expect)
    finally:
        batch.close()


def test_pileup_calls_equal_the_oracle_on_the_counts(gpu_ctx):
    """About 30 short alignments over two reference sequences, most starting inside them: the row of a position is its sequence's first row
    plus the position."""
    rng = np.random.default_rng(9)
    ref_lengths = [70, 93]
    reads, cigars, ref_index, start = [], [], [], []
    for i in range(30):
        k = int(rng.integers(0, 2))
        x0 = int(rng.integers(0, ref_lengths[k] - 40))
        ops = [(0, int(rng.integers(5, 12))), (int(rng.integers(1, 3)), int(rng.integers(1, 4))), (0, int(rng.integers(5, 12))),
               (int(rng.integers(1, 3)), int(rng.integers(1, 3))), (0, int(rng.integers(3, 9)))]
        assert x0 + sum(n for o, n in ops if o != 1) <= ref_lengths[k]
        reads.append("".join(rng.choice(list("ACGTacgtN"), p=[0.2, 0.2, 0.2, 0.2, 0.04, 0.04, 0.04, 0.04, 0.04]) for _ in range(sum(n for o, n in ops if o != 2))))
        cigars.append(ops), ref_index.append(k), start.append((x0, 0))
    reads.append("N" * 8), cigars.append([(0, 8)]), ref_index.append(1), start.append((85, 0))   # the end of sequence 1 under N alone: seen, no weight
    rows = sum(ref_lengths)
    ref_code = rng.integers(0, 5, size=rows).astype(np.uint8)
    true_code = np.where(rng.random(rows) < 0.3, rng.integers(0, 4, size=rows), ref_code).astype(np.uint8)
    pileup = gpu_ctx.pileup(ref_lengths)
    try:
        assert_same_calls(pileup.snp_calls(ref_code, true_code, NULL_MATRIX, MODELS[1]),   # an empty table: nothing seen, nothing called
                          [(np.zeros(101, dtype=np.int64), np.zeros(101, dtype=np.int64), rows, 0)])
        pileup.add(reads, cigars, ref_index, start=start)
        counts = pileup.counts()
        seen = counts[:, :5].sum(axis=1) > 0
        want, edge = snp_calls_reference(counts[:, :4], seen, ref_code, true_code, MODELS[2])
        assert edge > EDGE and want[0][2] > 0 and want[0][3] > 50 and seen[:70].any() and seen[70:].any()
        assert ((counts[:, :4].sum(axis=1) == 0) & seen).any()   # a position with N alone: seen, but no weight
        assert_same_calls(pileup.snp_calls(ref_code, true_code, NULL_MATRIX, MODELS[2]), want)
        assert np.array_equal(pileup.counts(), counts)
    finally:
        pileup.close()


def test_error_returns_leave_the_output_alone(gpu_ctx):
    L = _lib.load()
    weights, seen, ref, true = mixed_table(5, 40)
    seen8 = seen.astype(np.uint8)
    evolution = np.ascontiguousarray(NULL_MATRIX, dtype=np.float64)

    def refused(call, n_models, errors):
        errors = np.ascontiguousarray(errors, dtype=np.float64)
        out = (_lib.SnpCalls * 5)()
        ctypes.memset(out, 0x5a, ctypes.sizeof(out))
        before = bytes(out)
        rc = call(n_models, _lib.ptr(evolution), _lib.ptr(errors), ctypes.byref(out))
        assert bytes(out) == before
        return rc

    def table(n_models, evolution16, error16, out):
        return L.npr_snp_calls_table(gpu_ctx._h, 40, _lib.ptr(weights), _lib.ptr(seen8), _lib.ptr(ref), _lib.ptr(true), n_models, evolution16, error16, out)

    zero = np.array(MODELS[2], dtype=np.float64)
    zero[1, 2, 3] = 0.0
    assert refused(table, 2, zero) == _lib.ERR_INVALID
    assert refused(table, 5, np.tile(FLAT_ERROR_MATRIX, (5, 1, 1))) == _lib.ERR_INVALID
    assert refused(table, 0, FLAT_ERROR_MATRIX) == _lib.ERR_INVALID
    with pytest.raises(_lib.NprError) as e:   # ... and through the binding's one checked call
        gpu_ctx.snp_calls_table(weights, seen, ref, true, NULL_MATRIX, zero)
    assert e.value.code == _lib.ERR_INVALID and "npr_snp_calls_table" in str(e.value)
    with pytest.raises(_lib.NprError) as e:
        gpu_ctx.snp_calls_table(weights, seen, ref, true, NULL_MATRIX, np.tile(FLAT_ERROR_MATRIX, (5, 1, 1)))
    assert e.value.code == _lib.ERR_INVALID
    pileup = gpu_ctx.pileup([40])
    try:
        assert refused(lambda n, ev, er, out: L.npr_pileup_snp_calls(pileup._h, _lib.ptr(ref), _lib.ptr(true), n, ev, er, out), 2, zero) == _lib.ERR_INVALID
    finally:
        pileup.close()
    # the batch call before npr_batch_finish
    batch, ref_lengths, ref_code, true_code = _stage_small_batch(gpu_ctx)
    try:
        lengths = np.asarray(ref_lengths, dtype=np.int64)
        assert refused(lambda n, ev, er, out: L.npr_batch_snp_calls(batch._h, None, 2, _lib.ptr(lengths), _lib.ptr(ref_code), _lib.ptr(true_code), n, ev, er, out),
                       1, FLAT_ERROR_MATRIX) == _lib.ERR_STATE
        with pytest.raises(_lib.NprError) as e:
            batch.snp_calls(ref_lengths, ref_code, true_code, NULL_MATRIX, MODELS[1])
        assert e.value.code == _lib.ERR_STATE
    finally:
        batch.close()


def test_calls_on_device_write_the_same_xml_and_feed_the_meta_analysis(tmp_path, gpu_ctx):
    """The miniature held-out experiment of test_gpu_pipeline.py, its mutated reference and truth file made by mutateReferenceSequences:
    MarginAlignSnpCaller with callsOnDevice writes what the host path writes, attribute string by attribute string."""
    from nanopore_amd import synth
    from nanopore_amd.analyses.marginAlignSnpCaller import MarginAlignSnpCaller
    from nanopore_amd.analyses.mutate_reference import mutateReferenceSequences
    from nanopore_amd.hmm import Hmm
    from nanopore_amd.metaAnalyses.marginAlignMetaAnalysis import ALL_COLUMNS, MarginAlignMetaAnalysis, fScore
    from test_gpu_pipeline import _mild_channel
    rng = np.random.default_rng(11)
    true = "".join("ACGT"[c] for c in rng.integers(0, 4, size=1500))
    bioio.fastaWrite(str(tmp_path / "ref.fa"), "chr", true)
    fa = mutateReferenceSequences([str(tmp_path / "ref.fa")], rng=random.Random(11))[1]
    assert fa.endswith("ref_1.0_percent_SNPs_0.0_percent_InDels.fasta")
    mutated = dict(bioio.fastaRead(fa))["chr"]
    held = sum(a != b for a, b in zip(true, mutated))
    assert 5 <= held <= 30
    T, E = _mild_channel()
    codes = np.array(["ACGT".index(c) for c in true], dtype=np.uint8)
    n = 40
    rc, roff, cols, coff = synth.error_channel(rng, np.tile(codes, n), np.arange(n + 1, dtype=np.int64) * len(codes), T, E)
    runs, run_off = synth.columns_to_runs(cols, coff)
    fq, samp = tmp_path / "reads.fq", tmp_path / "mapping.sam"
    with open(fq, "w") as fqh, open(samp, "w") as sh:
        sh.write("@SQ\tSN:chr\tLN:%d\n" % len(true))
        for i in range(n):
            read = "".join("ACGT"[c] for c in rc[roff[i]:roff[i + 1]])
            fqh.write("@read%d\n%s\n+\n%s\n" % (i, read, "I" * len(read)))
            cigar = "".join("%d%s" % (l, "MID"[o]) for o, l in runs[run_off[i]:run_off[i + 1]])
            sh.write("\t".join(["read%d" % i, "0", "chr", "1", "255", cigar, "*", "0", "0", read, "*"]) + "\n")
    nodes = {}
    for on_device in (True, False):
        out = tmp_path / ("device" if on_device else "host") / "analysis_MarginAlignSnpCaller"
        out.mkdir(parents=True)
        an = MarginAlignSnpCaller(str(fq), "2D", fa, str(samp), str(out))
        assert MarginAlignSnpCaller.callsOnDevice is False   # the default is not flipped
        an.coverages, an.callsOnDevice = (1000000, 10), on_device
        nodes[on_device] = an.run(ctx=gpu_ctx, seed=5)
        an.cleanup()
    gpu_ctx.set_hmm(Hmm.loadHmm(trainedModelPath("blasr_hmm_0.txt")))
    device, host = list(nodes[True]), list(nodes[False])
    assert len(device) == len(host) == 4 * 4 * (1 + 3)
    for d, h in zip(device, host):
        assert d.tag == h.tag and list(d.attrib) == list(h.attrib)
        for name in h.attrib:
            assert d.attrib[name] == h.attrib[name], (d.tag, d.attrib["coverage"], d.attrib["replicate"], name)
    assert (tmp_path / "device" / "analysis_MarginAlignSnpCaller" / "marginaliseConsensus.xml").read_text() == \
        (tmp_path / "host" / "analysis_MarginAlignSnpCaller" / "marginaliseConsensus.xml").read_text()
    best = [k for k in device if k.tag == "marginAlignMaxExpectedSnpCalls_trained_0" and k.attrib["coverage"] == "1000000"][0]
    assert best.attrib["totalHeldOut"] == str(held) and best.attrib["totalSampledReads"] == "40"
    assert float(best.attrib["actualCoverage"]) > 30
    assert float(best.attrib["recall"]) >= 0.75 and float(best.attrib["precision"]) >= 0.75
    low = [k for k in device if k.tag == "marginAlignMaxExpectedSnpCalls_trained_0" and k.attrib["coverage"] == "10"]
    assert len(low) == 3 and all(int(k.attrib["totalSampledReads"]) < 40 for k in low)

    class SomeMapper(object):
        pass

    meta_dir = tmp_path / "meta"
    meta_dir.mkdir()
    meta = MarginAlignMetaAnalysis(str(meta_dir), [(str(fq), "2D", fa, SomeMapper, [], str(tmp_path / "device"))])
    meta.run()
    meta.cleanup()
    rows = [ln.split("\t") for ln in (meta_dir / "marginAlignAll.txt").read_text().splitlines()]
    assert rows[0] == ALL_COLUMNS
    # coverage 10 is dropped, 1000000 is ALL: one row per call set and hmm type; 1 % of the bases were held out
    assert sorted(r[2] for r in rows[1:]) == sorted(set(k.tag for k in device)) and len(rows) == 1 + 16
    assert all(r[:2] == ["2D", "SomeMapper"] and r[3:5] == ["0.01", "ALL"] for r in rows[1:])
    row = [r for r in rows[1:] if r[2] == best.tag][0]
    assert row[5:] == [str(fScore(best))] * 3 + [str(float(best.attrib["recall"]))] * 3 + [str(float(best.attrib["precision"]))] * 3 + \
        [str(float(best.attrib["totalNoCalls"]) / 1500)] * 3 + [str(float(best.attrib["actualCoverage"]))] * 3

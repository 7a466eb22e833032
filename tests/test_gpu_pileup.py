"""The device pileup (include/nprealign.h: npr_pileup_*; csrc/npr_pileup.hip; nanopore_amd/analyses/pileup.py, metaAnalyses/coverageDepth.py):
every word at every position against what samtools 0.1.19 printed for the fixtures of tests/golden/pileup/ (parser and column counter:
tests/test_pileup_host.py), and against the column counter on random records beyond them.  Counts are integers: every comparison is exact."""
import os
import shutil
import time

import numpy as np
import pytest

from nanopore_amd import _lib
from nanopore_amd.realign import NprError
from test_pileup_host import SETS, WORDS, count_columns, fixture, parse_mpileup, sam_contigs

pytestmark = pytest.mark.gpu

LETTER = "MID"


def _letters(cigar):
    return [(LETTER[op], n) for op, n in cigar]


def _expect(ref_lengths, reads, cigars, ref_index, start=None, use=None):
    """The table of the selected records from the column counter."""
    base = np.concatenate([[0], np.cumsum(ref_lengths)]).astype(np.int64)
    table = np.zeros((int(base[-1]), WORDS), dtype=np.int32)
    for i in range(len(reads)):
        if use is None or use[i]:
            sx, sy = start[i] if start is not None else (0, 0)
            count_columns(table, int(base[ref_index[i]]) + sx, _letters(cigars[i]), reads[i], y=sy)
    return table


def _expect_by_runs(ref_lengths, reads, cigars, ref_index):
    """The same table from run arithmetic in numpy, for records whose reference span is too long to walk: a difference array over the D runs."""
    base = np.concatenate([[0], np.cumsum(ref_lengths)]).astype(np.int64)
    table = np.zeros((int(base[-1]), WORDS), dtype=np.int32)
    diff = np.zeros(int(base[-1]) + 1, dtype=np.int64)
    code = np.full(256, 4, dtype=np.int64)
    for k, ch in enumerate("ACGT"):
        code[ord(ch)] = code[ord(ch.lower())] = k
    for i, cigar in enumerate(cigars):
        x, y, have_column, previous = int(base[ref_index[i]]), 0, False, None
        seq = code[np.frombuffer(reads[i].encode(), dtype=np.uint8)]
        for op, n in cigar:
            if n == 0:
                continue
            if op != 1 and not have_column:
                table[x, 7] += 1
                have_column = True
            if op == 0:
                np.add.at(table, (np.arange(x, x + n), seq[y:y + n]), 1)
            elif op == 2:
                diff[x] += 1
                diff[x + n] -= 1
            elif have_column and previous != 1:
                table[x - 1, 6] += 1
            x, y, previous = x + (n if op != 1 else 0), y + (n if op != 2 else 0), op
    table[:, 5] = np.cumsum(diff)[:-1]
    return table


def _random_seq(rng, n, alphabet="ACGT"):
    return np.frombuffer(alphabet.encode(), dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes().decode()


def _random_cigar(rng, n_m, m_hi=60):
    ops = []
    if rng.integers(0, 4) == 0:
        ops.append((1, int(rng.integers(1, 6))))                       # a leading I
    if rng.integers(0, 4) == 0:
        ops.append((2, int(rng.integers(1, 30))))                      # a leading D (and an I after it, sometimes)
        if rng.integers(0, 2) == 0:
            ops.append((1, int(rng.integers(1, 4))))
    for j in range(n_m):
        if j:
            i_run, d_run = (1, int(rng.integers(1, 6))), (2, int(rng.integers(1, 9)))
            ops += [[i_run], [d_run], [i_run, d_run], [d_run, i_run], [i_run, (0, 0), i_run], [(2, 0)], [i_run, i_run]][int(rng.integers(0, 7))]
        ops.append((0, int(rng.integers(1, m_hi))))
    if rng.integers(0, 4) == 0:
        ops += [[(1, 3)], [(2, 11)], [(2, 4), (1, 2)], [(1, 2), (2, 4)]][int(rng.integers(0, 4))]
    return ops


def _spans(cigar):
    return sum(n for op, n in cigar if op != 1), sum(n for op, n in cigar if op != 2)


@pytest.mark.parametrize("name", SETS)
def test_fixture_sets_equal_samtools(gpu_ctx, name):
    """All eight words at every position equal what `samtools mpileup` printed, and the depth text is `samtools depth`'s byte for byte."""
    from nanopore_amd.analyses.pileup import depth_text, pileup_of_sam
    fx = fixture(name)
    names, lengths, pileup = pileup_of_sam(gpu_ctx, fx["sam_path"], fx["fa_path"])
    try:
        assert (names, [int(v) for v in lengths]) == sam_contigs(fx["sam"])
        want, _ = parse_mpileup(fx["mpileup"], names, lengths)
        got = pileup.counts()
        assert got.dtype == np.int32 and got.shape == want.shape
        assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        depth, covered = pileup.depth()
        assert np.array_equal(depth, want[:, :5].sum(axis=1)) and np.array_equal(covered, want[:, :6].sum(axis=1) != 0)
        assert depth_text(names, lengths, depth, covered) == fx["depth"]
    finally:
        pileup.close()


def test_random_records_over_several_megabases(gpu_ctx):
    """Several thousand records over five sequences of 3 Mb in all: many workgroups, cigars of more than 64 operations, M runs longer than a
    wavefront, zero-length operations, records that touch the first and the last position of neighbouring sequences, window starts, a mask."""
    rng = np.random.default_rng(5)
    ref_lengths = [1500000, 7, 900000, 1, 600003]
    n = 4000
    reads, cigars, ref_index, start = [], [], [], []
    for i in range(n):
        k = int(rng.choice([0, 2, 4], p=[0.5, 0.3, 0.2])) if i % 97 else int(rng.choice([1, 3]))
        if ref_lengths[k] < 100:
            cigar = [(0, ref_lengths[k])] if i % 2 else [(2, ref_lengths[k])]
        else:
            cigar = _random_cigar(rng, int(rng.integers(1, 8)) if i % 50 else 90, 60 if i % 31 else 700)
        x, y = _spans(cigar)
        sx = 0 if i % 11 == 0 else (ref_lengths[k] - x if i % 11 == 1 else int(rng.integers(0, ref_lengths[k] - x + 1)))
        sy = int(rng.integers(0, 9)) if i % 3 == 0 else 0
        reads.append(_random_seq(rng, sy + y + int(rng.integers(0, 5)), "ACGTACGTNacgtn" if i % 4 == 0 else "ACGT"))
        cigars.append(cigar), ref_index.append(k), start.append((sx, sy))
    reads += ["", "ACGT", "ACGT"]
    cigars += [[(2, 5)], [], [(1, 4)]]                                 # a single D run, no operation at all, a single I run
    ref_index += [1, 0, 2]
    start += [(2, 0), (10, 0), (0, 0)]
    use = (rng.random(len(reads)) < 0.8).astype(np.uint8)
    use[n:] = 1
    assert max(len(c) for c in cigars) > 128 and max(ln for c in cigars for op, ln in c if op == 0) > 256
    pl = gpu_ctx.pileup(ref_lengths)
    try:
        assert pl.counts().sum() == 0 and pl.depth()[0].sum() == 0 and not pl.depth()[1].any()
        pl.add([], [], [])                                             # empty input
        assert pl.counts().sum() == 0
        pl.add(reads, cigars, ref_index, start=start, use=use)
        want = _expect(ref_lengths, reads, cigars, ref_index, start, use)
        got = pl.counts()
        assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        assert want[:, 5].sum() > 1000 and want[:, 6].sum() > 1000 and want[:, 4].sum() > 100 and want[:, 7].sum() == int(use.sum()) - 2
        depth, covered = pl.depth()
        assert np.array_equal(depth, want[:, :5].sum(axis=1)) and np.array_equal(covered, want[:, :6].sum(axis=1) != 0)
        # the run arithmetic the next test's expectation is made with, pinned against the column walk on these records
        full = [i for i in range(len(reads)) if use[i] and start[i] == (0, 0)]
        a = _expect_by_runs(ref_lengths, [reads[i] for i in full], [cigars[i] for i in full], [ref_index[i] for i in full])
        b = _expect(ref_lengths, [reads[i] for i in full], [cigars[i] for i in full], [ref_index[i] for i in full])
        assert len(full) > 100 and np.array_equal(a, b)
    finally:
        pl.close()


def test_global_records_cost_their_runs_not_their_span(gpu_ctx):
    """2 000 global records over one 4.6 Mb contig hold about 10^10 deletion columns; the table is right and comes back at once, because a D
    run is two adds into a difference array whatever its length."""
    rng = np.random.default_rng(17)
    length, n = 4600000, 2000
    reads, cigars = [], []
    for i in range(n):
        inner = _random_cigar(rng, int(rng.integers(2, 9)))
        x, y = _spans(inner)
        lead = int(rng.integers(0, length - x + 1)) if i % 9 else 0
        trail = length - x - lead
        cigars.append([(2, lead)] + inner + ([(2, trail)] if i % 2 else [(2, trail), (1, 3)]))
        reads.append(_random_seq(rng, _spans(cigars[-1])[1], "ACGTNacgt"))
    assert sum(ln for c in cigars for op, ln in c if op == 2) > 9 * 10 ** 9
    pl = gpu_ctx.pileup([length])
    try:
        t0 = time.perf_counter()
        pl.add(reads, cigars, [0] * n)
        got = pl.counts()
        seconds = time.perf_counter() - t0
        want = _expect_by_runs([length], reads, cigars, [0] * n)
        assert np.array_equal(got, want), np.argwhere(got != want)[:10]
        assert (got[:, :6].sum(axis=1) == n).all() and got[:, 7].sum() == n   # every record covers every position
        depth, covered = pl.depth()
        assert covered.all() and np.array_equal(depth, want[:, :5].sum(axis=1))
        print("2000 global records over 4.6 Mb: add + counts %.3f s" % seconds)
    finally:
        pl.close()


def test_accumulation_in_parts(gpu_ctx):
    rng = np.random.default_rng(23)
    ref_lengths = [5000, 3000]
    reads, cigars, ref_index, start = [], [], [], []
    for i in range(300):
        k = i % 2
        cigar = _random_cigar(rng, int(rng.integers(1, 6)))
        x, y = _spans(cigar)
        reads.append(_random_seq(rng, y, "ACGTN"))
        cigars.append(cigar), ref_index.append(k), start.append((int(rng.integers(0, ref_lengths[k] - x + 1)), 0))
    whole, parts = gpu_ctx.pileup(ref_lengths), gpu_ctx.pileup(ref_lengths)
    try:
        whole.add(reads, cigars, ref_index, start=start)
        for lo, hi in ((0, 100), (100, 101), (101, 300)):
            parts.add(reads[lo:hi], cigars[lo:hi], ref_index[lo:hi], start=start[lo:hi])
            got = parts.counts()                                       # read in between: the difference array stays what it is
            assert np.array_equal(got, _expect(ref_lengths, reads[:hi], cigars[:hi], ref_index[:hi], start[:hi]))
            assert np.array_equal(parts.depth()[0], got[:, :5].sum(axis=1))
        assert np.array_equal(parts.counts(), whole.counts()) and whole.counts()[:, 5].sum() > 0
    finally:
        whole.close(), parts.close()


def test_add_batch_equals_add_of_the_batch_cigars(gpu_ctx):
    """The table made where a finished batch's cigars lie is the table of those cigars; a read that failed adds nothing."""
    from helpers import MODEL_DIR, load_model_arrays
    from nanopore_amd import realign as R, synth
    from nanopore_amd.hmm import Hmm
    T, E, _ = load_model_arrays()
    n = 64
    w = synth.make_workload(77, n, 1500, T, E, flank=0, length_sigma=0.4, len_min=200, len_max=4000)
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    read = w["read"].copy()
    read[::53] = ord("N")
    guide_ops = w["guide_ops"].reshape(-1, 2).copy()
    last = int(w["guide_off"][6]) - 1                                  # read 5's guide stops short of its sequences: the read fails
    assert guide_ops[last, 1] > 1
    guide_ops[last, 1] -= 1
    ref_lengths = np.diff(w["ref_off"])
    P = R.make_params(band_mode=R.BAND_ANCHOR, constraint_trim=4, split_threshold=100, max_pairs_per_base=40)
    for host_mea in (False, True):
        if host_mea:
            gpu_ctx.set_option(_lib.OPTIONS["host_mea"], 1)
        b = gpu_ctx.stage_csr(P, w["ref"], w["ref_off"], read, w["read_off"], guide_ops, w["guide_off"])
        where, again, masked = gpu_ctx.pileup(ref_lengths), gpu_ctx.pileup(ref_lengths), gpu_ctx.pileup(ref_lengths)
        try:
            with pytest.raises(NprError) as e:
                where.add_batch(b)
            assert e.value.code == _lib.ERR_STATE
            b.run(), b.finish()
            res, (off, ops) = b.results(), b.ops()
            ok = res["status"] == 0
            assert not ok[5] and ok.sum() == n - 1 and res["n_segments"].max() > 1
            where.add_batch(b)
            reads = [bytes(read[w["read_off"][i]:w["read_off"][i + 1]]).decode() for i in range(n)]
            cigars = [[(int(a), int(c)) for a, c in ops[off[i]:off[i + 1]]] for i in range(n)]
            again.add(reads, cigars, np.arange(n), use=ok)
            got, want = where.counts(), again.counts()
            assert np.array_equal(got, want) and got[:, :5].sum() > 10000 and got[:, 5].sum() > 100 and got[:, 6].sum() > 100
            assert np.array_equal(want, _expect(ref_lengths, reads, cigars, list(range(n)), use=ok))
            row5 = int(w["ref_off"][5] - w["ref_off"][0])
            assert got[row5:row5 + int(ref_lengths[5])].sum() == 0     # the failed read's reference: nothing
            use = (np.arange(n) % 3 != 0).astype(np.uint8)
            masked.add_batch(b, use=use)
            assert np.array_equal(masked.counts(), _expect(ref_lengths, reads, cigars, list(range(n)), use=ok & (use != 0)))
        finally:
            where.close(), again.close(), masked.close(), b.close()
            gpu_ctx.set_option(_lib.OPTIONS["host_mea"], 0)


def test_a_cigar_that_overruns_adds_nothing(gpu_ctx):
    ref_lengths = [60, 40]
    reads = ["ACGTACGTACGTACGTACGT", "ACGTACG", "ACGTACGTAC", "ACGTACGTACGTACGTACGTACGTACGTAC", "ACGTAC"]
    cigars = [[(0, 5), (2, 3), (0, 10), (1, 2), (0, 3)],                 # fine
              [(0, 4), (2, 2), (0, 6)],                                  # runs past its read (7 bases, 10 needed) after valid columns
              [(0, 10)],                                                 # fine, ends with its reference
              [(0, 20), (2, 15), (0, 10)],                               # runs past its reference (40 positions, 45 needed)
              [(0, 3), (3, 2), (0, 3)]]                                  # an operation outside M I D
    ref_index, start = [0, 0, 1, 1, 0], [(10, 0), (0, 0), (30, 0), (0, 0), (0, 0)]
    pl = gpu_ctx.pileup(ref_lengths)
    try:
        with pytest.raises(NprError) as e:
            pl.add(reads, cigars, ref_index, start=start)
        assert e.value.code == _lib.ERR_INVALID
        good = np.array([1, 0, 1, 0, 0], dtype=np.uint8)
        want = _expect(ref_lengths, reads, cigars, ref_index, start, good)
        got = pl.counts()
        assert np.array_equal(got, want) and got[:, 7].sum() == 2 and got[:10].sum() == 0
        pl.add(reads, cigars, ref_index, start=start, use=good)           # the bad ones not selected: no error, the good ones twice
        assert np.array_equal(pl.counts(), 2 * want)
        for bad_index, bad_start in ((2, (0, 0)), (-1, (0, 0)), (0, (61, 0)), (0, (0, 21)), (0, (-1, 0))):
            with pytest.raises(NprError):
                pl.add(reads[:1], cigars[:1], [bad_index], start=[bad_start])
        assert np.array_equal(pl.counts(), 2 * want)
    finally:
        pl.close()
    with pytest.raises(NprError):
        gpu_ctx.pileup([10, -1])


def test_coverage_depth_end_to_end(gpu_ctx, tmp_path):
    from nanopore_amd.analyses.utils import getFastaDictionary
    from nanopore_amd.metaAnalyses.coverageDepth import CoverageDepth, coverageStats
    fx = fixture("local")
    results, out = tmp_path / "results" / "experiment_1", tmp_path / "meta"
    results.mkdir(parents=True), out.mkdir()
    shutil.copy(fx["sam_path"], str(results / "mapping.sam"))

    class LastzMapper(object):
        pass

    experiments = [("reads.fq", "2D", fx["fa_path"], LastzMapper, [], str(results)), ("reads.fq", "2D", fx["fa_path"], LastzMapper, [], str(tmp_path / "results" / "absent"))]
    CoverageDepth(str(out), experiments).run(ctx=gpu_ctx)
    depth_file, stats_file = out / "experiment_1_Depth.txt", out / "experiment_1_Stats.out"
    assert depth_file.read_text() == fx["depth"]
    stats = stats_file.read_text()
    assert stats == coverageStats(fx["depth"], getFastaDictionary(fx["fa_path"])) and stats.startswith("Position\tCoverage (mu=4.25761772853X, sd=")
    assert sorted(os.listdir(str(out))) == ["experiment_1_Depth.txt", "experiment_1_Stats.out"]
    stamp = os.stat(str(depth_file)).st_mtime_ns
    stats_file.unlink()
    CoverageDepth(str(out), experiments).run(ctx=gpu_ctx)             # the experiment has its depth file: left alone
    assert os.stat(str(depth_file)).st_mtime_ns == stamp and depth_file.read_text() == fx["depth"] and not stats_file.exists()


def test_context_close_closes_open_pileups():
    from nanopore_amd import realign
    ctx = realign.Context(0)
    pl = ctx.pileup([1000, 10])
    pl.add(["ACGT"], [[(0, 4)]], [1])
    assert pl.counts()[1000:1004, :4].sum() == 4
    ctx.close()
    assert pl._h is None
    pl.close()

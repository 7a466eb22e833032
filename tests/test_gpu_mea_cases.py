"""The device MEA chain (csrc/npr_mea.hip) on the constructed pair lists of tests/mea_cases.py, against the oracle's O(k^2) all-pairs statement
of the rule -- not against the project's own host stage: status, ops, score (the same double expression) and pair count exactly, and the
pairs npr_batch_pairs returns.  The lists replace, through the test hook npr_batch_debug_set_pairs, what the DP pass left for single-segment
reads of the cases' lengths; cases that share gammas share a batch, so the lanes of one k_mea_chain_lanes wavefront hold pieces of different
reads, some handed over to the ring kernel and some not.  npr_batch_debug_finish_stage says which stage finished the batch: a device stage
that gave up on every batch would otherwise pass as "the host stage's results"."""
import numpy as np
import pytest

import mea_cases as mc
from helpers import orc
from nanopore_amd import _lib

pytestmark = pytest.mark.gpu

# name -> (test / bring-up switches, NPR_OPT_OVERLAP)
VARIANTS = {
    "default": ({}, 0),
    "ring_only": (dict(mea_ring_only=1), 0),
    "global_sort": (dict(mea_global_sort=1), 0),
    "ring_only_global_sort": (dict(mea_ring_only=1, mea_global_sort=1), 0),
    "host_mea": (dict(host_mea=1), 0),
    "own_tables": ({}, 2),
}


@pytest.fixture(scope="module")
def brute():
    """name -> (ops, score) of the brute force, computed once for all variants"""
    out = {}
    for name, lX, lY, x, y, p, gg, mg in mc.cases():
        ops, score = orc.mea_cigar(lX, lY, x, y, p.astype(np.float64), gg, mg, brute_force=True)
        out[name] = ([tuple(o) for o in ops], score)
    return out


def _batches():
    """[(gammas + tag, cases)]: the cases that share gammas in one batch; the ones that must reach the host stage in batches of their own"""
    groups = {}
    for c in mc.cases():
        if c[0] not in mc.EXPECT_REFUSED:
            groups.setdefault((c[6], c[7], mc.BATCH_TAG.get(c[0], "")), []).append(c)
    return sorted(groups.items())


def _reads(cases):
    """single-segment reads of the cases' lengths: random bases, the guide one M run and the rest deleted / inserted"""
    rng = np.random.default_rng(5)
    refs, reads, guides = [], [], []
    for _, lX, lY in (c[:3] for c in cases):
        refs.append(bytes(b"ACGT"[v] for v in rng.integers(0, 4, lX)))
        reads.append(bytes(b"ACGT"[v] for v in rng.integers(0, 4, lY)))
        k = min(lX, lY)
        guides.append([(_lib.OP_M, k)] + ([(_lib.OP_D, lX - k)] if lX > k else []) + ([(_lib.OP_I, lY - k)] if lY > k else []))
    return refs, reads, guides


def _finish_batch(ctx, cases, order_seed):
    """run(), every case's list injected in shuffled order, finish() -> per case (status, ops, score, n_pairs, x, y, p), and the stage"""
    from nanopore_amd import realign as R
    rng = np.random.default_rng(order_seed)
    if order_seed:
        cases = [cases[i] for i in rng.permutation(len(cases))]
    per_base = max([6] + [-(-(len(c[3]) - 64) // min(c[1], c[2])) for c in cases])
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=128, gap_gamma=cases[0][6], match_gamma=cases[0][7], max_pairs_per_base=per_base)
    b = ctx.stage(P, *_reads(cases))
    try:
        b.run()
        for r, c in enumerate(cases):
            perm = rng.permutation(len(c[3]))
            b.debug_set_pairs(r, c[3][perm], c[4][perm], c[5][perm])
        b.finish()
        res = b.results()
        off, ops = b.ops()
        poff, x, y, p = b.pairs()
        stage = b.finish_stage()
    finally:
        b.close()
    assert (res["n_segments"] == 1).all()
    out = {}
    for r, c in enumerate(cases):
        s = slice(poff[r], poff[r + 1])
        out[c[0]] = (int(res["status"][r]), [(int(o), int(n)) for o, n in ops[off[r]:off[r + 1]]], float(res["score"][r]), int(res["n_pairs"][r]),
                     x[s].copy(), y[s].copy(), p[s].copy())
    return out, stage


def _check_batch(ctx, key, cases, brute, want_stage):
    for order_seed in (0, 17):  # the reads in two different orders: other lanes, other neighbours
        got, stage = _finish_batch(ctx, cases, order_seed)
        assert stage == want_stage, (key, order_seed, "finished by the %s stage" % ("host", "device")[stage == _lib.FINISH_DEVICE])
        for c in cases:
            name = c[0]
            status, ops, score, n_pairs, x, y, p = got[name]
            assert status == 0, (name, status)
            assert ops == brute[name][0], (name, order_seed)
            assert score == brute[name][1], (name, order_seed)
            assert n_pairs == len(c[3]), name
            srt = np.lexsort((c[4], c[3]))
            assert np.array_equal(x, c[3][srt]) and np.array_equal(y, c[4][srt]) and np.array_equal(p.view(np.uint32), c[5][srt].view(np.uint32)), name


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_constructed_lists_equal_brute_force(gpu_ctx, brute, variant):
    switches, overlap = VARIANTS[variant]
    try:
        gpu_ctx.set_option(_lib.OPT_OVERLAP, overlap)
        with gpu_ctx.options(**switches):
            for key, cases in _batches():
                host = variant == "host_mea" or any(c[0] in mc.EXPECT_HOST for c in cases)
                _check_batch(gpu_ctx, key, cases, brute, _lib.FINISH_HOST if host else _lib.FINISH_DEVICE)
    finally:
        gpu_ctx.set_option(_lib.OPT_OVERLAP, 0)


def test_long_runs_as_whole_words(gpu_ctx, brute):
    """the deleted runs of 16383 (the longest a 16-bit word holds) and 16384, each in its batch, with mea_wide_ops as well"""
    picked = [(key, cases) for key, cases in _batches() if any(c[0] in mc.WIDE_OPS_CASES for c in cases)]
    assert len(picked) == 2
    with gpu_ctx.options(mea_wide_ops=1):
        for key, cases in picked:
            _check_batch(gpu_ctx, key, cases, brute, _lib.FINISH_DEVICE)


def test_gammas_that_are_no_weights_are_refused_at_staging(gpu_ctx):
    """gap_gamma 250, match_gamma -300: the weights would not fit the 32 bits the device keeps them in -- a clean error, no wrapped weight"""
    from nanopore_amd import realign as R
    wild = [c for c in mc.cases() if c[0] in mc.EXPECT_REFUSED]
    assert wild
    for c in wild:
        for gg, mg in ((c[6], c[7]), (c[6], 0.0), (0.5, c[7]), (float("nan"), 0.0), (-0.01, 0.0), (0.5, 1.01)):
            with pytest.raises(R.NprError) as e:
                gpu_ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=128, gap_gamma=gg, match_gamma=mg), *_reads([c]))
            assert e.value.code == _lib.ERR_INVALID
    # the ends of the range are taken
    for gg, mg in ((0.0, -1.0), (1.0, 1.0)):
        gpu_ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=128, gap_gamma=gg, match_gamma=mg), *_reads(wild)).close()

"""The in-LDS sort of the MEA finish (csrc/npr_mea.hip k_mea_sort_lds: one read of the posterior pairs, ranks kept in registers, weights
written beside the sorted pairs) and the k_mea_weigh that reads them, on constructed pair lists: every batch is finished twice from the same
injected lists (npr_batch_debug_set_pairs), by the device stage and by the host stage (NPR_OPT_HOST_MEA), and status, ops and score must be
equal read by read.  The lists aim at what the sort can get wrong: no pairs, one pair, a crowded reference position with equal posteriors,
the first and last positions of both sequences, more pairs than the threads' register budget (1024 x 22, and 512 x 22 in overlap mode),
pairs that are no input (the read ends NPR_ERR_INVALID, its neighbours as if it were not there), and a read beyond the LDS tables beside
reads within them."""
import numpy as np
import pytest

from nanopore_amd import _lib

pytestmark = pytest.mark.gpu

SORT_BUDGET_PAIRS = 1024 * 22  # threads x SORT_BUDGET of k_mea_sort_lds


def _diagonal(rng, L, p_lo=0.3):
    """a usual list over an L x L read: the diagonal with large posteriors, its two neighbours with small ones; no pair twice"""
    d = np.arange(L, dtype=np.int32)
    x = np.concatenate([d, d[:-1], d[1:]])
    y = np.concatenate([d, d[1:], d[:-1]])
    p = np.concatenate([rng.uniform(p_lo, 1.0, L), rng.uniform(0.01, 0.3, 2 * (L - 1))]).astype(np.float32)
    return x, y, p


def _crowded(rng, L):
    """reference positions 50 and L - 7 carry 40 pairs each, most of them with the same posterior; the diagonal elsewhere"""
    x, y, p = _diagonal(rng, L)
    keep = (x != 50) & (x != L - 7)
    xs, ys, ps = [x[keep]], [y[keep]], [p[keep]]
    for gx, y0 in ((50, 30), (L - 7, L - 45)):
        gy = np.arange(y0, y0 + 40, dtype=np.int32)
        gp = np.full(40, 0.3, np.float32)
        gp[::7] = 0.02   # not kept
        gp[3] = gp[17] = 0.85  # two equal leaders
        xs.append(np.full(40, gx, np.int32)), ys.append(gy), ps.append(gp)
    return np.concatenate(xs), np.concatenate(ys), np.concatenate(ps)


def _corners(rng, L):
    """the four corners of the matrix besides a stretch of the diagonal"""
    d = np.arange(5, L - 5, dtype=np.int32)
    x = np.concatenate([d, np.array([0, 0, L - 1, L - 1], np.int32)])
    y = np.concatenate([d, np.array([0, L - 1, 0, L - 1], np.int32)])
    p = np.concatenate([rng.uniform(0.4, 1.0, len(d)), [0.9, 0.6, 0.6, 0.9]]).astype(np.float32)
    return x, y, p


def _dense(rng, L, per_x=12):
    """per_x pairs on every reference position, around the diagonal: more than the sort's threads hold in registers"""
    xs = np.repeat(np.arange(L, dtype=np.int32), per_x)
    ys = xs + np.tile(np.arange(per_x, dtype=np.int32) - per_x // 2, L)
    ok = (ys >= 0) & (ys < L)
    xs, ys = xs[ok], ys[ok]
    p = np.where(xs == ys, rng.uniform(0.5, 1.0, len(xs)), rng.uniform(0.01, 0.08, len(xs))).astype(np.float32)
    return xs, ys, p


def _lists(seed=11):
    """[(name, L, x, y, p, expected status)]"""
    rng = np.random.default_rng(seed)
    none = np.zeros(0, np.int32)
    out = [("usual_a", 700) + _diagonal(rng, 700) + (0,),
           ("no_pairs", 300, none, none, np.zeros(0, np.float32), 0),
           ("one_pair", 200, np.array([117], np.int32), np.array([120], np.int32), np.array([0.75], np.float32), 0),
           ("crowded", 900) + _crowded(rng, 900) + (0,),
           ("corners", 333) + _corners(rng, 333) + (0,),
           ("over_budget", 2000) + _dense(rng, 2000) + (0,)]
    x, y, p = _diagonal(rng, 450)
    x = x.copy()
    x[200] = 450  # one past the last reference position
    out.append(("x_out_of_range", 450, x, y, p, _lib.ERR_INVALID))
    x, y, p = _diagonal(rng, 512)
    p = p.copy()
    p[77] = np.nan
    out.append(("nan_posterior", 512, x, y, p, _lib.ERR_INVALID))
    out.append(("usual_b", 1025) + _diagonal(rng, 1025) + (0,))
    return out


def _finish(ctx, lists, host, max_pairs_per_base=24):
    """stage + run, the lists injected in shuffled order, finish -> ([(status, ops, score)], stage)"""
    from nanopore_amd import realign as R
    rng = np.random.default_rng(3)
    refs = [bytes(b"ACGT"[v] for v in rng.integers(0, 4, c[1])) for c in lists]
    reads = [bytes(b"ACGT"[v] for v in rng.integers(0, 4, c[1])) for c in lists]
    guides = [[(_lib.OP_M, c[1])] for c in lists]
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=128, gap_gamma=0.2, match_gamma=0.0, max_pairs_per_base=max_pairs_per_base)
    with ctx.options(**(dict(host_mea=1) if host else {})):
        b = ctx.stage(P, refs, reads, guides)
        try:
            b.run()
            for r, c in enumerate(lists):
                perm = rng.permutation(len(c[2]))
                b.debug_set_pairs(r, c[2][perm], c[3][perm], c[4][perm])
            b.finish()
            res = b.results()
            off, ops = b.ops()
            stage = b.finish_stage()
        finally:
            b.close()
    assert (res["n_segments"] == 1).all()
    return [(int(res["status"][r]), [(int(o), int(n)) for o, n in ops[off[r]:off[r + 1]]], float(res["score"][r])) for r in range(len(lists))], stage


def _device_equals_host(ctx, lists):
    dev, stage = _finish(ctx, lists, host=False)
    assert stage == _lib.FINISH_DEVICE
    ref, stage = _finish(ctx, lists, host=True)
    assert stage == _lib.FINISH_HOST
    for c, d, h in zip(lists, dev, ref):
        assert d[0] == h[0] == c[5], (c[0], d[0], h[0])
        assert d[1] == h[1], c[0]
        assert d[2] == h[2], c[0]
    return dev


@pytest.fixture(scope="module")
def lists():
    out = _lists()
    assert len(out[5][2]) > SORT_BUDGET_PAIRS  # the over-budget path runs
    assert all(len(np.unique(c[2].astype(np.int64) << 32 | c[3])) == len(c[2]) for c in out)  # (the host stage refuses a pair given twice)
    return out


def test_constructed_lists_equal_host_stage(gpu_ctx, lists):
    dev = _device_equals_host(gpu_ctx, lists)
    by_name = {c[0]: d for c, d in zip(lists, dev)}
    assert sorted(by_name["no_pairs"][1]) == sorted([(_lib.OP_D, 300), (_lib.OP_I, 300)]) and by_name["no_pairs"][2] == 0.0
    assert (_lib.OP_M, 1) in by_name["one_pair"][1]
    # a read that is no input leaves its neighbours alone: the same cigars without it in the batch
    good = [c for c in lists if c[5] == 0]
    alone, _ = _finish(gpu_ctx, good, host=False)
    assert alone == [by_name[c[0]] for c in good]


def test_overlap_mode_sorts_with_512_threads(gpu_ctx, lists):
    """NPR_OPT_OVERLAP 1: workgroups of 512 threads, half the register budget -- more than half of the dense read's pairs lie beyond it"""
    try:
        gpu_ctx.set_option(_lib.OPT_OVERLAP, 1)
        _device_equals_host(gpu_ctx, lists)
    finally:
        gpu_ctx.set_option(_lib.OPT_OVERLAP, 0)


def test_lds_and_global_sorted_reads_share_a_launch(gpu_ctx):
    """one read beyond the 16 k positions the in-LDS tables hold among reads within them"""
    rng = np.random.default_rng(23)
    lists = [("short_a", 800) + _diagonal(rng, 800) + (0,), ("long", 17000) + _diagonal(rng, 17000) + (0,),
             ("crowded", 600) + _crowded(rng, 600) + (0,), ("short_b", 1999) + _diagonal(rng, 1999) + (0,)]
    _device_equals_host(gpu_ctx, lists)

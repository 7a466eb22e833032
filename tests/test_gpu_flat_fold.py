"""The FLAT instances of the frame kernels (k_dp_rs / k_dp_mid_rs, npr_rs.h) fold the gap states' flat emission 2^-2 into the transitions and
compute every row under the band's lane mask.  The table-driven instances still look the emissions up and multiply; with blasr_hmm_0 they read
0.25 from LDS, so the two must agree bit for bit.  The library takes the FLAT instances only when EVERY loaded model is flat: the same batch is
staged in a context that holds blasr_hmm_0 alone (FLAT) and in one whose slot 1 holds a model with base-dependent gap emissions that no read
uses (table-driven)."""
import os

import numpy as np
import pytest

from nanopore_amd import _lib

from helpers import MODEL_DIR, random_pair

pytestmark = pytest.mark.gpu

MID, RS = 12, 15            # first class of k_dp_mid_rs / k_dp_rs; + 0, 1, 2 for 1, 2, 4 slots per lane
SLOT_OF_BAND = {100: 0, 200: 1, 400: 2}


def _models():
    from nanopore_amd.hmm import Hmm
    flat = Hmm.loadHmm(os.path.join(MODEL_DIR, "blasr_hmm_0.txt"))
    bent = Hmm.loadHmm(os.path.join(MODEL_DIR, "blasr_hmm_0.txt"))
    E = np.array(bent.emissions).reshape(5, 4, 4).copy()
    g = np.array([0.4, 0.1, 0.2, 0.3]) / 4
    E[1], E[3] = g[:, None] * np.ones((4, 4)), g[::-1][:, None] * np.ones((4, 4))
    E[2], E[4] = g[None, :] * np.ones((4, 4)), g[::-1][None, :] * np.ones((4, 4))
    bent.emissions = [float(v) for v in E.reshape(-1)]
    return flat, bent


@pytest.fixture(scope="module")
def ctx_pair():
    """(context whose launches are FLAT, context whose launches are table-driven); every read uses slot 0 = blasr_hmm_0 in both."""
    from nanopore_amd import realign as R
    flat, bent = _models()
    a, b = R.Context(0), R.Context(0)
    a.set_hmm(flat, slot=0)
    b.set_hmm(flat, slot=0)
    b.set_hmm(bent, slot=1)
    yield a, b
    a.close()
    b.close()


def _join(parts):
    X = np.concatenate([p[0] for p in parts]).astype(np.uint8)
    Y = np.concatenate([np.asarray(p[1], dtype=np.uint8) for p in parts]).astype(np.uint8)
    ops = [o for p in parts for o in p[2]]
    return X, Y, ops


def _ins(rng, k):
    return np.zeros(0, np.uint8), rng.integers(0, 4, size=k).astype(np.uint8), [(1, k)]


def _del(rng, k):
    return rng.integers(0, 4, size=k).astype(np.uint8), np.zeros(0, np.uint8), [(2, k)]


def _text(codes, n_at=()):
    s = bytearray(b"ACGT"[c] for c in codes)
    for i in n_at:
        s[i] = ord("N")
    return bytes(s)


def _cases(seed):
    """(ref, read, guide): 300-700 bases, odd and even numbers of anti-diagonals, a 30-60 base insertion and a deletion of that size (the band
    moves and the frame rebases either way), N in both sequences, a band that runs along the matrix's edge at both ends, and one read of
    fewer anti-diagonals than k_dp_mid_rs takes (MID_MIN_D = 64)."""
    rng = np.random.default_rng(seed)
    P = lambda n, **kw: random_pair(rng, n, **kw)
    raw = [P(300, indel=0.15, max_indel=6), P(457, indel=0.15, max_indel=6), P(700, indel=0.2, max_indel=12),
           _join([P(220), _ins(rng, 47), P(230)]),
           _join([P(250), _del(rng, 52), P(180)]),
           _join([P(180), _ins(rng, 33), P(150), _del(rng, 58), P(140)]),
           _join([_ins(rng, 40), P(330), _del(rng, 40)]),      # leaves the matrix's corner along an edge, comes back along the other
           _join([_del(rng, 36), P(300), _ins(rng, 31)]),
           P(30, indel=0.0)]                                  # D = 60 < MID_MIN_D: k_dp_rs
    out = []
    for i, (X, Y, ops) in enumerate(raw):
        nx = (5, len(X) // 2, len(X) - 3) if i in (1, 4) else ()
        ny = (0, len(Y) // 3, len(Y) - 1) if i in (1, 5) else ()
        out.append((_text(X, nx), _text(Y, ny), ops))
    par = {(len(x) + len(y)) & 1 for x, y, _ in out}
    assert par == {0, 1}
    return out


def _run(ctx, P, cases, pair_opt):
    ctx.set_option(_lib.OPTIONS["pair"], pair_opt)
    try:
        b = ctx.stage(P, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        tasks, _ = b.class_stats()
        b.run()
        arith = b.segment_arith()[1].copy()
        b.finish()
        out = dict(tasks=tasks.copy(), arith=arith, res=b.results(), pairs=b.pairs(), ops=b.ops())
        b.close()
    finally:
        ctx.set_option(_lib.OPTIONS["pair"], 0)
    return out


@pytest.mark.parametrize("kernel", ["mid", "rs"])
@pytest.mark.parametrize("W", [100, 200, 400])
def test_flat_instance_equals_the_table_instance(ctx_pair, W, kernel):
    from nanopore_amd import realign as R
    flat, table = ctx_pair
    cases = _cases(8100 + W)
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=W)
    got = [_run(c, P, cases, _lib.PAIR_NEVER if kernel == "rs" else 0) for c in (flat, table)]
    for o in got:
        t = o["tasks"]
        assert t.sum() == len(cases) == t[MID:MID + 3].sum() + t[RS:RS + 3].sum(), t      # the frame kernels in row-scaled arithmetic took every read
        assert t[(MID if kernel == "mid" else RS) + SLOT_OF_BAND[W]] >= 8, t               # ... all but the short one in the class the band asks for
        assert t[RS] >= 1 and (kernel == "mid" or t[MID:MID + 3].sum() == 0), t            # the short read is k_dp_rs's in either case
        assert (o["arith"] == 1).all(), o["arith"]                                          # nothing ran again per cell
        assert (o["res"]["status"] == 0).all()
    a, c = got
    assert np.array_equal(a["tasks"], c["tasks"])
    for key in ("status", "cells", "loglik", "loglik_bwd", "score", "n_pairs"):
        assert np.array_equal(a["res"][key], c["res"][key]), key
    for u, v in zip(a["pairs"], c["pairs"]):
        assert np.array_equal(u, v)
    assert a["pairs"][3].size > sum(len(x[0]) for x in cases) // 2
    for u, v in zip(a["ops"], c["ops"]):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("W", [100, 200, 400])
@pytest.mark.parametrize("kind", ["insertion", "deletion"])
def test_forward_rows_stay_exact_when_the_band_jumps(ctx_pair, W, kind):
    """A guide that moves the band by more than its half-width within 50 reference bases: the control words say `moved` on many rows in a row and
    the frame rebases on each.  A slot the band left and that was not cleared would feed the next rows' cells, the rows' common exponent (the
    renormalisation takes the maximum over ALL slots) and the total at the cut; a slot a band entered would start from it.  The hook returns the
    stored forward rows' band cells (it has no access to slots outside the band), every one of which -- not only those above the pair lists'
    0.01 -- and every row exponent must equal the table-driven instance's, which multiplies slots outside the band by 0.
    (This is the test that keeps the fold out of the four-slot kernels: with it, band 400 gave 2 867 of 122 910 cells that differed after the
    insertion and 106 after the deletion, the largest 2.0e-25 -- subnormal intermediates that the renormalisation lifted back among the normal
    numbers once the band had jumped.  Bands 100 and 200 gave none; only the two-slot kernels fold today, npr_rs.h RS_FOLD_R.)"""
    from nanopore_amd import realign as R
    flat, table = ctx_pair
    rng = np.random.default_rng(8200 + W)
    k = W // 2 + 12
    X, Y, ops = _join([random_pair(rng, 150), _ins(rng, k) if kind == "insertion" else _del(rng, k), random_pair(rng, 151)])
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=W)
    (seg,) = R.plan(P, len(X), len(Y), ops)
    cells = seg["cells"]
    rows = []
    for ctx in (flat, table):
        b = ctx.stage(P, [_text(X)], [_text(Y)], [ops])
        tasks, _ = b.class_stats()
        assert tasks[MID + SLOT_OF_BAND[W]] == 1, tasks
        b.run()
        assert list(b.segment_arith()[1]) == [1]
        rows.append(b.rs_forward(0, cells))
        b.close()
    (fv, fe), (tv, te) = rows
    assert fv.size > 150 * (W // 2) and (fv > 0).sum() > fv.size // 2
    assert np.array_equal(fe, te)
    fb, tb = fv.view(np.uint32), tv.view(np.uint32)
    bad = np.nonzero(fb != tb)[0]
    # (what differs, before the verdict: how many cells, the largest of them, by how many units in the last place)
    print("band %d %s: %d of %d cells differ; largest differing value %g (bits %#x), largest difference %d ulp" % (
        W, kind, bad.size, fb.size, float(max(fv[bad].max(), tv[bad].max())) if bad.size else 0.0,
        int(max(fb[bad].max(), tb[bad].max())) if bad.size else 0,
        int(np.abs(fb[bad].astype(np.int64) - tb[bad].astype(np.int64)).max()) if bad.size else 0))
    assert bad.size == 0


def test_two_launches_on_poisoned_scratch_give_the_same_pairs(ctx_pair, monkeypatch):
    """Under the lane mask a lane outside the band writes nothing: a kernel that READ such a register, or a row from the scratch before it is
    written, would see the poison (NPR_POISON) of this launch instead of what the last one left."""
    from nanopore_amd import realign as R
    flat, _ = ctx_pair
    monkeypatch.setenv("NPR_POISON", "0x3f")
    cases = _cases(8300)
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=200)
    first = _run(flat, P, cases, 0)
    assert first["tasks"][MID + 1] == 8 and (first["res"]["status"] == 0).all()
    monkeypatch.setenv("NPR_POISON", "0xc1")
    again = _run(flat, P, cases, 0)
    for key in ("status", "loglik", "loglik_bwd", "score"):
        assert np.array_equal(first["res"][key], again["res"][key]), key
    for u, v in zip(first["pairs"], again["pairs"]):
        assert np.array_equal(u, v)
    for u, v in zip(first["ops"], again["ops"]):
        assert np.array_equal(u, v)

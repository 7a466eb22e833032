"""What npr_batch_create decides for a batch -- every task's kernel class, the class totals, the launch slots -- pinned as literals
for three small batches under every switch that enters the class rules (nanopore_amd/csrc/npr_stage.cpp), and the errors staging
itself returns.  The literals are what the library gave before staging was split into steps (device_bytes included: it came out the
same in fresh processes)."""
import numpy as np
import pytest

from helpers import MODEL_DIR, random_pair

pytestmark = pytest.mark.gpu

WIDTHS = (40, 200, 900)  # BAND_FIXED, one per batch: one-slot frames, four-slot frames and stripes
REALIGN, EM = 0, 3       # NPR_MODE_REALIGN, NPR_MODE_EXPECTATIONS
# name -> (mode, context options, NPR_OPT_OVERLAP)
SETTINGS = {
    "default": (REALIGN, {}, 0),
    "arith=1": (REALIGN, {"arith": 1}, 0),
    "kernel=1": (REALIGN, {"kernel": 1}, 0),
    "no_tile=1": (REALIGN, {"no_tile": 1}, 0),
    "no_tile=1 no_wide=1": (REALIGN, {"no_tile": 1, "no_wide": 1}, 0),
    "tile_rs=2": (REALIGN, {"tile_rs": 2}, 0),
    "pair=1": (REALIGN, {"pair": 1}, 0),
    "pair=2": (REALIGN, {"pair": 2}, 0),
    "overlap": (REALIGN, {}, 1),
    "em": (EM, {}, 0),
    "em em_tile=1": (EM, {"em_tile": 1}, 0),
}
STATS = ("n_tasks", "cells", "diagonals", "max_width", "slots", "kernel_variant", "device_bytes")

# (batch, setting) -> ({class: (tasks, cells)}, STATS)
EXPECT = {
    (0, 'default'): ({12: (20, 689687), 15: (4, 3126)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'arith=1'): ({0: (24, 692813)}, (24, 692813, 34189, 21, 24, 1, 13690396)),
    (0, 'kernel=1'): ({7: (24, 692813)}, (24, 692813, 34189, 21, 24, 0, 13553640)),
    (0, 'no_tile=1'): ({12: (20, 689687), 15: (4, 3126)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'no_tile=1 no_wide=1'): ({12: (20, 689687), 15: (4, 3126)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'tile_rs=2'): ({12: (20, 689687), 15: (4, 3126)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'pair=1'): ({15: (24, 692813)}, (24, 692813, 34189, 21, 24, 1, 13690396)),
    (0, 'pair=2'): ({12: (16, 681045), 15: (8, 11768)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'overlap'): ({12: (20, 689687), 15: (4, 3126)}, (24, 692813, 34189, 21, 24, 1, 7886364)),
    (0, 'em'): ({0: (24, 692813)}, (24, 692813, 34189, 21, 24, 1, 13690396)),
    (0, 'em em_tile=1'): ({0: (24, 692813)}, (24, 692813, 34189, 21, 24, 1, 13690396)),
    (1, 'default'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'arith=1'): ({0: (4, 2775), 1: (20, 2588089)}, (24, 2590864, 27941, 101, 24, 1, 57530756)),
    (1, 'kernel=1'): ({7: (24, 2590864)}, (24, 2590864, 27941, 101, 24, 0, 57418992)),
    (1, 'no_tile=1'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'no_tile=1 no_wide=1'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'tile_rs=2'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'pair=1'): ({15: (4, 2775), 16: (20, 2588089)}, (24, 2590864, 27941, 101, 24, 1, 57530756)),
    (1, 'pair=2'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'overlap'): ({13: (20, 2588089), 15: (4, 2775)}, (24, 2590864, 27941, 101, 24, 1, 24576388)),
    (1, 'em'): ({0: (4, 2775), 1: (20, 2588089)}, (24, 2590864, 27941, 101, 24, 1, 57530756)),
    (1, 'em em_tile=1'): ({0: (4, 2775), 1: (20, 2588089)}, (24, 2590864, 27941, 101, 24, 1, 57530756)),
    (2, 'default'): ({14: (1, 33855), 15: (4, 2906), 18: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 143556572)),
    (2, 'arith=1'): ({0: (4, 2906), 2: (1, 33855), 11: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 179061212)),
    (2, 'kernel=1'): ({7: (24, 11841232)}, (24, 11841232, 35285, 451, 24, 0, 216145032)),
    (2, 'no_tile=1'): ({3: (19, 11804471), 14: (1, 33855), 15: (4, 2906)}, (24, 11841232, 35285, 451, 24, 1, 171828700)),
    (2, 'no_tile=1 no_wide=1'): ({7: (19, 11804471), 14: (1, 33855), 15: (4, 2906)}, (24, 11841232, 35285, 451, 24, 0, 171687560)),
    (2, 'tile_rs=2'): ({11: (19, 11804471), 14: (1, 33855), 15: (4, 2906)}, (24, 11841232, 35285, 451, 24, 2, 143556572)),
    (2, 'pair=1'): ({15: (4, 2906), 17: (1, 33855), 18: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 179061212)),
    (2, 'pair=2'): ({14: (1, 33855), 15: (4, 2906), 18: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 143556572)),
    (2, 'overlap'): ({14: (1, 33855), 15: (4, 2906), 18: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 143556572)),
    (2, 'em'): ({0: (4, 2906), 18: (20, 11838326)}, (24, 11841232, 35285, 451, 24, 2, 170705884)),
    (2, 'em em_tile=1'): ({0: (4, 2906), 2: (1, 33855), 11: (19, 11804471)}, (24, 11841232, 35285, 451, 24, 2, 179061212)),
}


def _ascii(codes):
    return bytes(b"ACGT"[c] for c in codes)


def make_batches():
    """Three batches of 24 reads of 20 to 1500 bases: four of fewer than 32 (tasks of fewer than 64 anti-diagonals stay with k_dp_rs)."""
    rng = np.random.default_rng(20261018)
    out = []
    for _ in WIDTHS:
        lengths = list(rng.integers(20, 32, size=4)) + list(rng.integers(32, 1501, size=20))
        cases = [random_pair(rng, int(n)) for n in lengths]
        out.append(([_ascii(X) for X, _, _ in cases], [_ascii(Y) for _, Y, _ in cases], [g for _, _, g in cases]))
    return out


@pytest.fixture(scope="module")
def batches():
    return make_batches()


def staged(ctx, batches, which, setting):
    """-> (the batch staged under the setting, what it decided in EXPECT's form)"""
    from nanopore_amd import _lib, realign as R
    mode, options, overlap = SETTINGS[setting]
    refs, reads, guides = batches[which]
    ctx.set_option(_lib.OPT_OVERLAP, overlap)
    try:
        with ctx.options(**options):
            b = ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=WIDTHS[which], mode=mode), refs, reads, guides)
    finally:
        ctx.set_option(_lib.OPT_OVERLAP, 0)
    tasks, cells = b.class_stats()
    st = b.stats()
    return b, ({c: (int(tasks[c]), int(cells[c])) for c in range(len(tasks)) if tasks[c]}, tuple(int(st[k]) for k in STATS))


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    from nanopore_amd.hmm import Hmm
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    return gpu_ctx


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("which", range(len(WIDTHS)))
def test_what_staging_decides(ctx, batches, which, setting):
    b, got = staged(ctx, batches, which, setting)
    try:
        print(which, setting, got)
        assert b.plan_check() == 0
        assert got == EXPECT[which, setting]
        if SETTINGS[setting][0] == REALIGN:
            b.run(), b.finish()
            assert not b.results()["status"].any()
    finally:
        b.close()


def test_the_batches_populate_the_scaled_classes(ctx, batches):
    """the two-wavefront frame classes, the one-wavefront row-scaled ones and the column-scaled stripes"""
    seen = set()
    for which in range(len(WIDTHS)):
        seen |= set(EXPECT[which, "default"][0])
    assert seen & {12, 13, 14} and seen & {15, 16, 17} and 18 in seen


def test_without_ref_index_the_references_pair_with_the_reads(ctx):
    from nanopore_amd import _lib, realign as R
    with pytest.raises(_lib.NprError) as err:
        ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=10), [b"ACGTACGT"] * 2, [b"ACGTACGT"] * 3, [[(0, 8)]] * 3)
    assert err.value.code == _lib.ERR_INVALID
    assert ctx.last_error() == "npr_batch_create: without ref_index, n_refs must equal n_reads"


def test_a_read_of_an_unloaded_model_slot_leaves_its_neighbours_alone(ctx):
    from nanopore_amd import _lib, realign as R
    b = ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=10), [b"ACGTACGT"] * 3, [b"ACGTACGT"] * 3, [[(0, 8)]] * 3,
                  model_slot=[0, 7, 0])
    assert b.plan_check() == 0 and b.stats()["n_tasks"] == 2
    b.run(), b.finish()
    assert list(b.results()["status"]) == [0, _lib.ERR_MODEL, 0]
    b.close()


def test_a_batch_of_no_reads_stages(ctx):
    from nanopore_amd import realign as R
    b = ctx.stage(R.make_params(band_mode=R.BAND_FIXED, fixed_width=10), [], [], [])
    assert b.stats()["n_tasks"] == 0 and b.stats()["n_reads"] == 0
    b.close()

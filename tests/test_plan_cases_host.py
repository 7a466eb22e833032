"""Every constructed guide of tests/plan_cases.py is what its name says, shown with the host planner alone (the npr_plan_* functions of
include/nprealign.h, the ones tests/test_host_logic.py pins against the oracle).  No GPU: a family that was emptied or a case that lost its
property fails here, before tests/test_gpu_plan_edges.py stages anything."""
import numpy as np
import pytest

import plan_cases as pc
from nanopore_amd import realign as R


def _D(case):
    return len(case[2]) + len(case[3])


def test_every_guide_is_global_and_no_band_has_an_empty_row():
    for fam in pc.FAMILIES:
        assert pc.cases(fam), fam
        for c in pc.cases(fam):
            assert pc.spans(c[4]) == (len(c[2]), len(c[3])), c[0]
            for seg in pc.host_plan(c):
                assert int(seg["n"].min()) >= 1, c[0]   # (plan_cases.family_e says why no guide can make one)
    names = [c[0] for fam in pc.FAMILIES for c in pc.cases(fam)]
    assert len(set(names)) == len(names)


def test_family_a_lengths_sit_on_the_seams():
    flat = [c for c in pc.cases("a") if c[0].startswith("a_flat")]
    runs = [c for c in pc.cases("a") if c[0].startswith("a_run")]
    assert sorted(_D(c) for c in flat) == sorted(pc.A_LENGTHS)
    assert {_D(c) for c in runs} == {D for D in pc.A_LENGTHS if D >= pc.SCHED_CHUNK - 1}
    for c in flat + runs:
        segs = pc.host_plan(c)
        assert len(segs) == 1 and segs[0]["D"] == _D(c), c[0]
        assert sum(n for o, n in c[4] if o != pc.OP_M) <= (5 if c in runs else 1), c[0]   # (the run of 1 to 3, a one-base indel either side where a parity needs it)
    # every run begins where its name says, and between them the runs begin on every one of the four rows around a chunk edge and around 1024
    seen = set()
    for c in runs:
        edge, off = int(c[0].split("_at")[1].split("_")[0][:-2]), int(c[0].split("_at")[1].split("_")[0][-2:])
        d0 = pc.fixed_points_d0(c[4])
        k = [i for i, (o, n) in enumerate(c[4]) if o != pc.OP_M and d0[i] == edge + off and 1 <= n <= 3]
        assert k, c[0]
        assert edge % pc.SCHED_CHUNK == 0 and edge >= pc.SCHED_CHUNK and edge + off + c[4][k[0]][1] <= _D(c), c[0]
        seen.add((edge == pc.BAND_TILE, off))
    assert seen == {(t, o) for t in (False, True) for o in (-2, -1, 0, 1)}


def test_family_b_rebases_in_the_first_two_rows_of_a_chunk():
    got = set()
    for c in pc.cases("b"):
        cand, shape = pc.host_shape(c)
        assert shape == cand[0] == (int(c[0].split("_R")[1][0]), 1), c[0]   # the class the widths were chosen for, and the host picks it
        heads = pc.chunk_head_rebases(c, shape)
        assert heads, c[0]
        got |= {(shape, d % pc.SCHED_CHUNK, r) for d, r in heads}
    # towards lower x - y before a chunk's first row (even: a Y-step) and towards higher x - y before its second, in every class
    assert got >= {(s, 0, -1) for s in pc.FRAME_CLASSES} | {(s, 1, 1) for s in pc.FRAME_CLASSES}


def test_family_c_piece_density():
    by = {c[0]: c for c in pc.cases("c")}
    per = {k: pc.points_per_tile(c[4]) for k, c in by.items()}
    assert _D(by["c_1I1D"]) >= 2200 and (per["c_1I1D"][:2] == pc.BAND_TILE).all()          # a piece per anti-diagonal: the staging is full
    assert per["c_M500_1I1D"][0] < pc.BAND_TILE and per["c_M500_1I1D"][1] == pc.BAND_TILE   # dense from anti-diagonal 500 on
    assert _D(by["c_1M1I1M1D"]) >= 2200 and per["c_1M1I1M1D"].max() >= 2 * pc.BAND_TILE // 3
    for k in ("c_zero_runs", "c_zero_only_tail"):                                           # more points than a tile stages
        assert per[k].max() > pc.BAND_STAGE and any(n == 0 for o, n in by[k][4]), k
    assert (per["c_zero_runs"] > pc.BAND_STAGE).all() and len(per["c_zero_runs"]) >= 2
    # pieces without an anti-diagonal at the read's first and last one and on the seam between two tiles
    d0 = pc.fixed_points_d0(by["c_zero_runs"][4])
    for d in (0, pc.BAND_TILE, _D(by["c_zero_runs"])):
        assert (d0 == d).sum() > pc.BAND_STAGE, d
    for c in by.values():
        assert len(pc.host_plan(c)) == 1, c[0]


def test_family_e_stripe_counts():
    cs = pc.cases("e")
    assert sorted(len(c[2]) for c in cs) == sorted(pc.E_LENGTHS)
    for c in cs:
        segs = pc.host_plan(c)
        assert len(segs) == 1, c[0]
        st = R.stripes(pc.params_of(c), len(c[2]), len(c[3]), c[4], 2)
        assert len(st["X"]) == pc.E_STRIPES[len(c[2])] == len(c[2]) // pc.STRIPE_COLS + 1, c[0]
        assert (st["dl"] >= st["df"]).all() and st["rows"] == int((st["dl"] - st["df"] + 1).sum()), c[0]
        # no frame class that the case's mode allows admits the band: the task is the stripe kernel's
        limit = 126 if c[1].get("mode") == pc._lib.MODE_EXPECTATIONS else 255
        assert int(segs[0]["n"].max()) > limit, c[0]
        assert not pc.rough(segs[0]), c[0]   # (k_plan_stripes' binary searches; test_no_guide_makes_a_rough_band... says why none takes its general walk)
    assert {pc.E_STRIPES[len(c[2])] for c in cs} == {1, 2, 63, 64, 65, 128, 129}
    assert any(s > pc.STRIPE_TRIP for s in pc.E_STRIPES.values()) and pc.STRIPE_TRIP in pc.E_STRIPES.values()


def test_family_f_reads_have_many_uneven_segments():
    for c in pc.cases("f"):
        assert 3000 <= len(c[2]) <= 6000 and c[1]["split_threshold"] in (5, 40), c[0]
        segs = pc.host_plan(c)
        assert len(segs) >= 3 and len({s["D"] for s in segs}) >= 3, c[0]
    assert {c[1]["split_threshold"] for c in pc.cases("f")} == {5, 40}
    # chunks of the schedule per segment (D / 256 + 1) differ within a read: chunk_off is a prefix over uneven counts
    assert sum(len({s["D"] // pc.SCHED_CHUNK for s in pc.host_plan(c)}) >= 2 for c in pc.cases("f")) >= 2


def test_no_guide_makes_a_rough_band_or_fails_the_first_candidate_class():
    """The search for family D (class fall-through) and for rough bands, kept as a test: plan_cases.search_family states the family and why
    it comes back empty.  2000 seeds, every segment of every plan.  If this test fails the
    planner has changed: the guide it names is the missing D or rough-E case."""
    segments = at_limit = 0
    fitted = set()
    for c, shape in pc.search_family():
        segs = pc.host_plan(c)
        for i, seg in enumerate(segs):
            segments += 1
            assert int(seg["n"].min()) >= 1 and not pc.rough(seg), (c[0], i, "a rough band: a case for family E")
            cand = pc.candidates(seg)
            assert cand, (c[0], i)
            at_limit += int(seg["n"].max()) == pc.FRAME_MAX_WIDTH[cand[0]]
            assert pc.host_schedule(c, cand[0], i) is not None, (c[0], i, cand, "the first candidate fails: a case for family D")
        if max(int(g["n"].max()) for g in segs) == pc.FRAME_MAX_WIDTH[shape]:
            fitted.add((shape, c[1]["band_mode"], c[1].get("constraint_trim", -1)))
    # the search is not empty-handed for lack of trying: most seeds give a plan, and the widest row sits exactly on its class's limit in at
    # least the quarter of the seeds that are fixed-width bands (by construction) -- in every class, fixed and anchored, trimmed and not
    assert segments >= pc.SEARCH_SEEDS // 2 and at_limit >= pc.SEARCH_SEEDS // 4, (segments, at_limit)
    assert {f[0] for f in fitted} == set(pc.FRAME_CLASSES) and {f[1] for f in fitted} == {0, 1} and {f[2] for f in fitted} >= {0, 5, 14}, fitted

"""The device planner (nanopore_amd/csrc/npr_plan.hip) on the constructed guides of tests/plan_cases.py: lengths and indel runs on the seams
of k_plan_bands' tiles (1024 anti-diagonals) and of the schedule's chunks (256), rebases in a chunk's first two rows (the `moved` bits
k_sched_patch carries over), more plan points than a tile stages (pieces without an anti-diagonal: the search in global memory), stripe
tables of one, two and three trips of k_plan_stripes' wavefront, reads of many uneven segments, and a batch with more segments than the
grids of k_plan_bands have workgroups.  tests/test_plan_cases_host.py shows on the CPU that every case is what its name says.

npr_batch_plan_check compares every staged table with the host planner's -- for the class the task was sorted into.  Which class that is it
does not ask, so the class tests here do: a segment must land in the smallest frame the HOST can follow its band with."""
import time

import numpy as np
import pytest

import plan_cases as pc
from helpers import MODEL_DIR
from nanopore_amd import _lib

pytestmark = pytest.mark.gpu

ENVS = ({}, {"no_tile": 1}, {"kernel": 1})   # context options by name (_lib.OPTIONS): default, no stripe kernel, the any-band kernel throughout
assert all(k in _lib.OPTIONS for env in ENVS for k in env)

# class index of npr_batch_class_stats -> frame (R, NW), as include/nprealign.h documents them; the classes without a frame are not listed
SHAPE_OF_CLASS = {0: (1, 1), 1: (2, 1), 2: (4, 1), 3: (2, 4), 4: (2, 8), 5: (4, 8), 6: (4, 12),
                  12: (1, 1), 13: (2, 1), 14: (4, 1), 15: (1, 1), 16: (2, 1), 17: (4, 1)}


@pytest.fixture(scope="module")
def ctx(gpu_ctx):
    from nanopore_amd.hmm import Hmm
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    return gpu_ctx


def _stage(ctx, cases):
    return ctx.stage(pc.params_of(cases[0]), [c[2] for c in cases], [c[3] for c in cases], [c[4] for c in cases])


def _shuffled(cases, seed):
    return [cases[i] for i in np.random.default_rng(seed).permutation(len(cases))]


def _shape_counts(batch):
    """{(R, NW) or None: tasks} of the batch's classes"""
    out = {}
    for c, t in enumerate(batch.class_stats()[0]):
        if t:
            out[SHAPE_OF_CLASS.get(c)] = out.get(SHAPE_OF_CLASS.get(c), 0) + int(t)
    return out


@pytest.mark.parametrize("family", sorted(pc.FAMILIES))
def test_device_plans_equal_host_plans(ctx, family):
    """every case alone, then the family's cases (those that share parameters) in one batch in a shuffled order -- other segment indices,
    other band_off / ctl_off / chunk_off -- under each of ENVS"""
    t0 = time.time()
    staged = 0
    for env in ENVS:
        with ctx.options(**env):
            for group in pc.groups(family):
                for batch in [[c] for c in group] + [_shuffled(group, 31 + len(group))]:
                    b = _stage(ctx, batch)
                    try:
                        assert b.plan_check() == 0, (env, [c[0] for c in batch][:4])
                        assert b.stats()["n_tasks"] == sum(len(pc.host_plan(c)) for c in batch)
                        if family == "e" and not env:   # the stripe kernel takes these
                            assert b.stats()["kernel_variant"] == 2, batch[0][0]
                    finally:
                        b.close()
                    staged += 1
    print("family %s: %d cases, %d batches staged and checked in %.2f s" % (family, len(pc.cases(family)), staged, time.time() - t0))


def test_segments_land_in_the_smallest_frame_the_host_can_follow(ctx):
    """One-segment cases of families A and B, alone and in one shuffled batch per parameter set: the frame (R, NW) of the class that holds the
    task is the smallest candidate for which npr_plan_frame_schedule succeeds.  (A clamp composition in k_sched_compose / k_sched_starts that
    handed a chunk a wrong frame position would make the chunk fail and the segment move to a larger frame, with equal results and a passing
    plan_check.)"""
    t0 = time.time()
    for family in ("a", "b"):
        for group in pc.groups(family):
            want_sum = {}
            for c in group:
                cand, want = pc.host_shape(c)
                assert want is not None and want in cand, c[0]
                b = _stage(ctx, [c])
                try:
                    assert _shape_counts(b) == {want: 1}, c[0]
                finally:
                    b.close()
                want_sum[want] = want_sum.get(want, 0) + 1
            b = _stage(ctx, _shuffled(group, 5))
            try:
                assert _shape_counts(b) == want_sum, family
            finally:
                b.close()
    print("class of every A and B case: %.2f s" % (time.time() - t0))


def _finished(ctx, cases):
    b = _stage(ctx, cases)
    try:
        shapes = _shape_counts(b)
        b.run(), b.finish()
        res = b.results()
        off, ops = b.ops()
        return (res["status"].copy(), res["score"].copy(), off.copy(), ops.copy()), shapes
    finally:
        b.close()


@pytest.mark.parametrize("family", ["a", "b"])
def test_control_words_drive_the_frame_kernels(ctx, family):
    """run() and finish() on the device planner's control words against the same batch on the any-band kernel (NPR_OPT_KERNEL = 1), which reads
    band rows and row offsets only: status, score and cigars exactly (the kernels compute the same bits)."""
    t0 = time.time()
    for group in pc.groups(family):
        # (the reads without a reference base or without a read base, D = 0 and D = 1, are staged and checked above and not run: a DP problem
        # needs a base of each sequence)
        cases = [c for c in _shuffled(group, 9) if len(c[2]) and len(c[3])]
        got, shapes = _finished(ctx, cases)
        with ctx.options(kernel=1):
            want, generic = _finished(ctx, cases)
        # the two runs are two kernels: every task of the first in a frame class (the one the host picks), every task of the second in none
        assert None not in shapes and sum(shapes.values()) == len(cases) and set(shapes) == {pc.host_shape(c)[1] for c in cases}, shapes
        assert set(generic) == {None}, generic
        for g, w, what in zip(got, want, ("status", "score", "ops_off", "ops")):
            assert np.array_equal(g, w), (family, what, [c[0] for c, a, b in zip(cases, g, w) if what != "ops" and a != b][:5])
        assert (got[0] == 0).all()
    print("family %s run on both kernels: %.2f s" % (family, time.time() - t0))


def test_more_segments_than_workgroups(ctx):
    """65 600 one-segment reads of 1 to 3 bases: k_plan_bands' grid is capped at 65 536 workgroups and strides over the rest"""
    from nanopore_amd import realign as R
    n = 65600
    rng = np.random.default_rng(77)
    lens = rng.integers(1, 4, n)
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    seq = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(off[-1]))]
    guide_ops = np.stack([np.full(n, _lib.OP_M), lens], axis=1).astype(np.int32)
    t0 = time.time()
    b = ctx.stage_csr(R.make_params(band_mode=R.BAND_FIXED, fixed_width=10), seq, off, seq, off, guide_ops, np.arange(n + 1, dtype=np.int64))
    try:
        t1 = time.time()
        assert b.stats()["n_tasks"] == n
        assert b.plan_check() == 0
    finally:
        b.close()
    print("65 600 segments: staged in %.2f s, checked in %.2f s" % (t1 - t0, time.time() - t1))

import hashlib

import numpy as np

from helpers import load_model_arrays
from nanopore_amd import synth


def _spans(g):
    return int(g[g[:, 0] != 1, 1].sum()), int(g[g[:, 0] != 2, 1].sum())


def test_workload_is_seeded_and_guides_are_global():
    T, E, _ = load_model_arrays()
    w, W = synth.config_c2(T, E, n_reads=60)
    w2, _ = synth.config_c2(T, E, n_reads=60)
    assert W == 100 and (w["read"] == w2["read"]).all() and (w["guide_ops"] == w2["guide_ops"]).all()
    n = len(w["ref_off"]) - 1
    moved = 0
    for i in range(n):
        g = w["guide_ops"][w["guide_off"][i]:w["guide_off"][i + 1]]
        assert _spans(g) == (w["ref_off"][i + 1] - w["ref_off"][i], w["read_off"][i + 1] - w["read_off"][i])
        assert (g[:, 1] > 0).all() and (g[1:, 0] != g[:-1, 0]).all()
        t = w["true_runs"][w["true_off"][i]:w["true_off"][i + 1]]
        moved += int(len(g) != len(t) or (g != t).any())
    assert moved > n // 2                       # the guide is a degraded version of the truth
    rl = w["read_off"][1:] - w["read_off"][:-1]
    assert 800 < rl.mean() < 1250


def test_north_star_shape_has_50kb_slices():
    T, E, _ = load_model_arrays()
    w, W = synth.config_north_star(T, E, n_reads=8, windowed=False)
    assert W == 200 and ((w["ref_off"][1:] - w["ref_off"][:-1]) == 50000).all()
    g = w["guide_ops"][w["guide_off"][0]:w["guide_off"][1]]
    assert _spans(g)[0] == 50000 and w["guide_start"] is None
    # default: the guide keeps its own span and carries the coordinates of its window inside the slice
    v, _ = synth.config_north_star(T, E, n_reads=8)
    assert ((v["ref_off"][1:] - v["ref_off"][:-1]) == 50000).all() and np.array_equal(v["ref"], w["ref"])
    for i in range(8):
        g = v["guide_ops"][v["guide_off"][i]:v["guide_off"][i + 1]]
        sx, sy = _spans(g)
        assert sx == v["interval_len"][i] and sy == v["read_off"][i + 1] - v["read_off"][i]
        assert v["guide_start"][i, 0] == v["lead"][i] and v["guide_start"][i, 1] == 0
        assert v["guide_start"][i, 0] + sx <= 50000


def test_workloads_stay_what_their_seeds_made_them():
    """The seeded inputs of bench.py and of the tests do not change from build to build (outputs are compared across builds on
    them): digests of two small batches, the windowed north-star shape and the global-guide c2 shape."""
    T, E, _ = load_model_arrays()
    keys = ("ref", "ref_off", "read", "read_off", "guide_ops", "guide_off", "true_runs")
    for (w, _), want in ((synth.config_north_star(T, E, n_reads=16), "88989508bc6c792c996f3b7bc6a349639597347fa60afbac02e8da3874772ba3"),
                         (synth.config_c2(T, E, n_reads=16), "659577ee8b5b91ed70880d85fbd439278db604e305337a3d54f0b78c6c71f481")):
        assert hashlib.sha256(b"".join(np.ascontiguousarray(w[k]).tobytes() for k in keys)).hexdigest() == want

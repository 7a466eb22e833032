"""The second pass of npr_batch_run (nanopore_amd/csrc/npr_run.cpp): a task whose row- / column-scaled kernel (k_dp_rs, k_dp_mid_rs, k_dp_tile_cs)
comes back without its range certificate runs again in the per-cell kernel of its class (k_dp_stair<R>, k_dp_tile<2>) on the first launch's scratch
regions and queue counter, its result replaces the first one on the host and on the device, and the finish reads it there.  Natural refusals are
rare (one read in the rest of the suite), so the test hook npr_batch_debug_refuse marks tasks as refused: every scaled class, several tasks of a
launch at once, several classes of a batch at once, one segment of a read of many, every finish behind it -- against test_gpu_parity's two bars
(bit-exact against the fp32 mirror of the arithmetic each segment reports, 1e-4 against the fp64 oracle) and against the same batch left alone.

Why a refused task must give what it gave before, pair for pair: the per-cell and the row-scaled mirror are two bookkeepings of the same fp32
products and sums, and differ only where a value leaves a row's range -- which the certificate exists to exclude
(test_the_two_mirrors_agree_where_both_hold, on the CPU).  The stripe class's two kernels give the same bits by construction, and
npr_batch_segment_arith reports 0 for both of them: which stripe tasks ran again is read from the run's own report on stderr (NPR_TIMING)."""
import contextlib
import re

import numpy as np
import pytest

from nanopore_amd import _lib

from helpers import oracle_hmm, orc, random_pair
from test_gpu_parity import _hmm_obj, _pairs_dict, _run_case

gpu = pytest.mark.gpu

FRAME_SCALED, STRIPES_SCALED = range(12, 18), 18
INDEL = dict(indel=0.2, max_indel=30)


def _ascii(codes):
    return bytes(b"ACGT"[c] for c in codes)


def _cases(seed, n_reads, lmin, lmax):
    """The reads _run_case draws from default_rng(seed) with INDEL (the same calls in the same order)."""
    rng = np.random.default_rng(seed)
    return [random_pair(rng, int(rng.integers(lmin, lmax + 1)), **INDEL) for _ in range(n_reads)]


def _inputs(cases):
    return [_ascii(X) for X, _, _ in cases], [_ascii(Y) for _, Y, _ in cases], [g for _, _, g in cases]


@contextlib.contextmanager
def refusing(monkeypatch, mark):
    """Every Batch.run() inside the body is preceded by debug_refuse(mark(seg_off, scaled)) -- scaled: what segment_arith says before the run, 1 for
    the segments of the row-scaled frame classes.  Yields the log: one dict(tasks, seg_off, scaled, mark) per run."""
    from nanopore_amd import realign as R
    log, run = [], R.Batch.run

    def run_refused(self):
        off, scaled = self.segment_arith()
        m = np.asarray(mark(off, scaled.copy()), dtype=np.uint8)
        self.debug_refuse(m)
        log.append(dict(tasks=self.class_stats()[0].copy(), seg_off=off, scaled=scaled.copy(), mark=m))
        return run(self)

    with monkeypatch.context() as mp:
        mp.setattr(R.Batch, "run", run_refused)
        yield log


@contextlib.contextmanager
def remembering_oracle(monkeypatch):
    """orc.realign_read answers a question it has been asked before from memory: the patterns of a test ask for the same few mirrors of the same reads."""
    memo, ask = {}, orc.realign_read

    def realign_read(hmm, params, X, Y, guide_ops, precision=0, want_pairs=True, seg_arith=None):
        key = (bytes(hmm), bytes(params), np.asarray(X).tobytes(), np.asarray(Y).tobytes(), repr(guide_ops), precision, want_pairs,
               None if seg_arith is None else tuple(int(a) for a in seg_arith))
        if key not in memo:
            memo[key] = ask(hmm, params, X, Y, guide_ops, precision=precision, want_pairs=want_pairs, seg_arith=seg_arith)
        return memo[key]

    with monkeypatch.context() as mp:
        mp.setattr(orc, "realign_read", realign_read)
        yield memo


def _reruns(capfd):
    """{class: tasks run again} of the runs since the last call, from npr_batch_run's report (NPR_TIMING)."""
    out = {}
    for c, k in re.findall(r"\[npr\] class (\d+): (\d+) of \d+ tasks run again", capfd.readouterr().err):
        out[int(c)] = out.get(int(c), 0) + int(k)
    return out


def _same_answers(u, v, what=""):
    """two results of one read (Context.realign's dicts): the same posteriors bit for bit once sorted, the same cigar, score and totals"""
    ku, kv = np.lexsort((u["y"], u["x"])), np.lexsort((v["y"], v["x"]))
    assert u["status"] == v["status"], what
    assert np.array_equal(u["x"][ku], v["x"][kv]) and np.array_equal(u["y"][ku], v["y"][kv]), what
    assert np.array_equal(u["p"][ku].view(np.uint32), v["p"][kv].view(np.uint32)), what
    assert u["ops"] == v["ops"] and u["score"] == v["score"] and u["n_pairs"] == v["n_pairs"], what
    assert u["loglik"] == v["loglik"] and u["loglik_bwd"] == v["loglik_bwd"], what


def _arith(out):
    return np.array([a for o in out for a in o["seg_arith"]], dtype=np.int32)


# ---- the argument on the CPU ----

def test_the_two_mirrors_agree_where_both_hold():
    """The oracle's per-cell and row-scaled restatements on reads like those below -- fixed widths 40 / 200 / 300, a split anchor band, three random
    reads each: the same pairs (as sets: the two list them in different orders), cigars, scores and totals, bit for bit.  So a task that runs again
    although its certificate held must come back with what it had."""
    h = oracle_hmm()
    rng = np.random.default_rng(5)
    for kw, lo, hi in ((dict(band_mode=1, fixed_width=40), 100, 600), (dict(band_mode=1, fixed_width=200), 100, 600),
                       (dict(band_mode=1, fixed_width=300), 300, 600), (dict(band_mode=0, constraint_trim=2, split_threshold=12), 300, 500)):
        P = orc.make_params(**kw)
        for _ in range(3):
            X, Y, g = random_pair(rng, int(rng.integers(lo, hi + 1)), **INDEL)
            nseg = len(orc.plan(len(X), len(Y), g, P))
            a = orc.realign_read(h, P, X, Y, g, precision=1, seg_arith=[0] * nseg)
            b = orc.realign_read(h, P, X, Y, g, precision=1, seg_arith=[1] * nseg)
            ka, kb = np.lexsort((a["py"], a["px"])), np.lexsort((b["py"], b["px"]))
            assert a["status"] == b["status"] == 0 and a["ops"] == b["ops"] and a["score"] == b["score"] and a["total_ll"] == b["total_ll"]
            assert np.array_equal(a["px"][ka], b["px"][kb]) and np.array_equal(a["py"][ka], b["py"][kb])
            assert np.array_equal(a["pp"][ka].astype(np.float32).view(np.uint32), b["pp"][kb].astype(np.float32).view(np.uint32))


def test_a_second_launch_on_the_first_launch_s_regions_never_outgrows_them():
    """What stage_rerun's addressing rests on, restated: the tasks of a class lie in descending order of the scratch they need, workgroup w of the
    first launch got a region sized for task w, and it takes every later task from a queue that only moves forward -- so everything it runs fits.
    The second launch runs a subset `again` (ascending indices, so descending sizes) on min(len(again), grid) workgroups with the same regions:
    again[j] >= j, so task j of `again` is no larger than the j-th task of the class, whose region workgroup j has, and whatever the queue hands
    out later is smaller still -- whichever workgroup asks first.  Random descending size lists, random subsets, random finishing orders."""
    rng = np.random.default_rng(20261019)
    for _ in range(300):
        n = int(rng.integers(1, 60))
        size = np.sort(rng.integers(1, 1000, size=n))[::-1]          # the class, largest first (ties happen)
        grid = int(rng.integers(1, n + 3))
        region = size[:min(grid, n)]                                  # region w: sized for the task workgroup w starts with
        again = np.nonzero(rng.random(n) < rng.random())[0]
        if not len(again):
            continue
        assert all(again[j] >= j for j in range(len(again)))          # (what npr_batch_run asserts under the hook)
        assert all(size[again[j]] <= size[j] for j in range(len(again)))
        g2 = min(len(again), grid)
        queue, busy = 0, {w: again[w] for w in range(g2)}             # workgroup -> the task it runs
        while busy:
            w = list(busy)[int(rng.integers(len(busy)))]              # any of them finishes first
            assert size[busy[w]] <= region[w]
            t, queue = queue + g2, queue + 1
            if t < len(again):
                busy[w] = again[t]
            else:
                del busy[w]
        # ... and a grid of L.grid workgroups instead (more than there are tasks): the extra ones find nothing and the rest run the same tasks
        assert min(len(again), grid) <= len(region)


# ---- a. every scaled class, several mark patterns ----

PATTERNS = ("none", "all", "every other", "largest", "smallest")


def _pattern(name, cells):
    m = np.zeros(len(cells), dtype=np.uint8)
    order = np.argsort(-np.asarray(cells), kind="stable")  # the order of the tasks of a class: the costliest first
    if name == "all":
        m[:] = 1
    elif name == "every other":
        m[order[::2]] = 1
    elif name == "largest":
        m[order[0]] = 1
    elif name == "smallest":
        m[order[-1]] = 1
    return m


# name -> (band, reads, lmin, lmax, context options, the class that must take them)
CLASSES = {
    "k_dp_rs<1> short": (dict(band_mode=1, fixed_width=40), 16, 5, 26, {}, 15),          # fewer than 64 anti-diagonals
    "k_dp_rs<1>": (dict(band_mode=1, fixed_width=40), 12, 100, 600, {"pair": 1}, 15),
    "k_dp_rs<2>": (dict(band_mode=1, fixed_width=200), 12, 150, 600, {"pair": 1}, 16),
    "k_dp_rs<4>": (dict(band_mode=1, fixed_width=400, max_pairs_per_base=12), 8, 300, 600, {"pair": 1}, 17),
    "k_dp_mid_rs<1>": (dict(band_mode=1, fixed_width=40), 12, 100, 600, {}, 12),
    "k_dp_mid_rs<2>": (dict(band_mode=1, fixed_width=200), 12, 150, 600, {}, 13),
    "k_dp_mid_rs<4> w300": (dict(band_mode=1, fixed_width=300, max_pairs_per_base=12), 8, 300, 600, {}, 14),   # (151 cells per anti-diagonal: still one wavefront's frame)
    "k_dp_mid_rs<4>": (dict(band_mode=1, fixed_width=400, max_pairs_per_base=12), 8, 300, 600, {}, 14),
    "k_dp_tile_cs w520": (dict(band_mode=1, fixed_width=520, max_pairs_per_base=12), 8, 300, 600, {}, 18),     # 261 cells: the narrowest band of the stripe class
    "k_dp_tile_cs w700": (dict(band_mode=1, fixed_width=700, max_pairs_per_base=12), 8, 300, 600, {}, 18),
    "k_dp_tile_cs anchors": (dict(band_mode=0, diagonal_expansion=10, constraint_trim=14, split_threshold=3000, max_pairs_per_base=12), 8, 400, 1000, {}, 18),
}


@gpu
@pytest.mark.parametrize("name", list(CLASSES))
def test_refused_tasks_of_every_scaled_class_come_back_the_same(gpu_ctx, monkeypatch, capfd, name):
    """One batch per scaled kernel class (class_stats says that the class took it); no task, all, every other one in the class's order, the largest
    alone and the smallest alone refused.  Every read passes _run_case's two bars against the mirror of the arithmetic it then reports -- per cell
    exactly on the refused segments of the frame classes --, as many tasks run again as were marked, and every pattern gives the unmarked run's
    pairs, cigars, scores and totals."""
    kw, n, lmin, lmax, options, cls = CLASSES[name]
    seed = 4100 + list(CLASSES).index(name)
    okw = {k: v for k, v in kw.items() if k != "max_pairs_per_base"}
    P = orc.make_params(**okw)
    cases = _cases(seed, n, lmin, lmax)
    plans = [orc.plan(len(X), len(Y), g, P) for X, Y, g in cases]
    assert all(len(p) == 1 for p in plans)
    cells = [p[0]["cells"] for p in plans]
    monkeypatch.setenv("NPR_TIMING", "1")
    base = None
    with remembering_oracle(monkeypatch):
        for pattern in PATTERNS:
            mark = _pattern(pattern, cells)
            capfd.readouterr()
            with gpu_ctx.options(**options), refusing(monkeypatch, lambda off, scaled: mark) as log:
                out = _run_case(gpu_ctx, np.random.default_rng(seed), n, lmin, lmax, kw, **INDEL)
            again = _reruns(capfd)
            assert len(log) == 1 and [o["cells"] for o in out] == cells          # one batch, of the reads the marks were made for
            tasks, scaled = log[0]["tasks"], log[0]["scaled"]
            assert tasks[cls] > 0 and tasks[12:19].sum() == tasks.sum() == n, (name, tasks)
            if cls != STRIPES_SCALED and not name.endswith("short"):  # (an insertion can take a short read past 63 anti-diagonals; anchors make bands of any width)
                assert tasks[cls] == n, (name, tasks)
            else:
                assert tasks[cls] >= n // 2, (name, tasks)
            if base is None:
                assert pattern == "none"
                base, base_again = out, sum(again.values())
                # (a read of a handful of bases may miss its certificate by itself; the stripes report per-cell arithmetic whichever kernel ran them)
                assert (_arith(out) <= scaled).all() and (_arith(out) == scaled).sum() >= n - 2 and base_again <= 2, (name, _arith(out), scaled, again)
            assert np.array_equal(_arith(out), _arith(base) & (1 - mark)), (name, pattern, _arith(out), mark)
            assert mark.sum() <= sum(again.values()) <= mark.sum() + base_again, (name, pattern, again, mark)
            assert set(again) <= set(np.nonzero(tasks)[0].tolist())
            for i, (u, v) in enumerate(zip(out, base)):
                _same_answers(u, v, (name, pattern, i))


@gpu
def test_debug_dumps_of_a_batch_whose_task_ran_again(gpu_ctx):
    """npr_batch_rs_forward and npr_batch_dense launch their own kernel on the task (k_dp_rs, k_dp_generic) and read that kernel's layout: what the
    second pass left in the scratch never reaches them.  The same bytes as from the batch left alone, and no refusal."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    X, Y, g = _cases(4200, 1, 300, 300)[0]
    kw = dict(band_mode=1, fixed_width=100)
    cells = orc.plan(len(X), len(Y), g, orc.make_params(**kw))[0]["cells"]
    got = []
    for mark in (0, 1):
        b = gpu_ctx.stage(R.make_params(**kw), *_inputs([(X, Y, g)]))
        b.debug_refuse([mark])
        b.run()
        assert list(b.segment_arith()[1]) == [1 - mark]
        fwd = b.rs_forward(0, cells)
        b.run()                                     # (the marks are gone with the run that used them)
        assert list(b.segment_arith()[1]) == [1]
        got.append(fwd + b.dense(0, cells))
        b.close()
    assert (got[0][0] > 0).sum() > len(X)
    assert all(np.array_equal(u, v) for u, v in zip(got[0], got[1]))


@gpu
def test_the_hook_refuses_a_mark_list_of_another_length(gpu_ctx):
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    b = gpu_ctx.stage(R.make_params(band_mode=1, fixed_width=40), *_inputs(_cases(4201, 3, 40, 60)))
    for n in (0, 2, 4):
        with pytest.raises(_lib.NprError) as err:
            b.debug_refuse(np.ones(n, np.uint8))
        assert err.value.code == _lib.ERR_INVALID
    b.debug_refuse([0, 1, 0])
    b.run()
    assert list(b.segment_arith()[1]) == [1, 0, 1]
    b.close()


# ---- b. one refused segment inside a read of many ----

@gpu
@pytest.mark.parametrize("which", ["middle", "first", "last"])
def test_one_refused_segment_of_a_read_of_many(gpu_ctx, monkeypatch, which):
    """Reads cut into 5 to 13 segments (anchor band, matrix splits every dozen cells); one segment of each read refused -- a middle one, the first,
    the last (ragged at one end only).  The mirror called with the mixed list of arithmetics reproduces every read, and the cigars are those of
    the batch left alone."""
    kw = dict(band_mode=0, diagonal_expansion=10, constraint_trim=2, split_threshold=12)
    seed, n = 4300, 8

    def mark(off, scaled):
        m = np.zeros(int(off[-1]), dtype=np.uint8)
        for r in range(len(off) - 1):
            k = int(off[r + 1] - off[r])
            m[int(off[r]) + {"middle": k // 2, "first": 0, "last": k - 1}[which]] = 1
        return m

    runs = []
    for fn in (lambda off, scaled: np.zeros(int(off[-1]), np.uint8), mark):
        with refusing(monkeypatch, fn) as log:
            runs.append((_run_case(gpu_ctx, np.random.default_rng(seed), n, 300, 500, kw, **INDEL), log[0]))
    (base, lb), (out, lo) = runs
    nseg = np.diff(lo["seg_off"])
    assert nseg.min() >= 5 and nseg.max() >= 8 and lo["tasks"][12:19].sum() == lo["tasks"].sum(), (nseg, lo["tasks"])
    assert lo["scaled"].all() and _arith(base).sum() >= len(_arith(base)) - 2
    assert lo["mark"].sum() == n and np.array_equal(_arith(out), _arith(base) & (1 - lo["mark"]))
    for i, (u, v) in enumerate(zip(out, base)):
        _same_answers(u, v, (which, i))


# ---- c, d. all classes of one batch refused at once; every finish behind the second pass ----

MIXED_KW = dict(band_mode=1, fixed_width=900)


def _mixed_cases():
    """One band of 451 cells, reads of 20 to 700 bases: the short ones' bands end at their corners, so the batch has tasks of fewer than 64
    anti-diagonals (k_dp_rs<1>), of one, two and four slots per lane (k_dp_mid_rs<1|2|4>) and stripes (k_dp_tile_cs)."""
    rng = np.random.default_rng(4400)
    lengths = [20, 24, 27, 30, 40, 46, 52, 58, 80, 95, 110, 120, 150, 180, 210, 240, 300, 380, 460, 540, 620, 700]
    return [random_pair(rng, n, indel=0.2, max_indel=8) for n in lengths]


def _fetch(b, pairs=True):
    res = b.results().copy()
    off, ops = b.ops()
    out = dict(res=res, ops_off=off, ops=ops, arith=b.segment_arith()[1].copy(), stage=b.finish_stage())
    if pairs:
        out["pairs"] = b.pairs()
    return out


def _same_batch(u, v, what=""):
    for key in ("status", "loglik", "loglik_bwd", "score", "n_pairs", "cells"):
        assert np.array_equal(u["res"][key], v["res"][key]), (what, key)
    assert np.array_equal(u["ops_off"], v["ops_off"]) and np.array_equal(u["ops"], v["ops"]), what
    if "pairs" in u and "pairs" in v:
        for a, c in zip(u["pairs"], v["pairs"]):
            assert np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, c.view(np.uint32) if c.dtype == np.float32 else c), what


def _every_other_of_every_class(cells):
    """tasks of a class lie in descending order of cost: every other read by cells marks about every other task of each class"""
    return _pattern("every other", cells)


@gpu
def test_every_class_of_a_batch_refused_at_once_on_poisoned_scratch(gpu_ctx, monkeypatch, capfd):
    """A short k_dp_rs class, three k_dp_mid_rs classes and the stripe class in one batch, every other task of each of them refused: five second
    launches one after the other, each on its class's regions and counter, while the buffers are handed out filled with a poison byte (NPR_POISON)
    -- a second pass that read anything the first left in scratch, or another class's region, would differ from run to run or from the batch left
    alone.  Three times; identical to the unmarked run and to the run with every task refused."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    monkeypatch.setenv("NPR_POISON", "0x3f")
    monkeypatch.setenv("NPR_TIMING", "1")
    cases = _mixed_cases()
    P = R.make_params(**MIXED_KW)
    cells = [orc.plan(len(X), len(Y), g, orc.make_params(**MIXED_KW))[0]["cells"] for X, Y, g in cases]
    alt = _every_other_of_every_class(cells)
    got = {}
    for what, mark, reps in (("none", np.zeros(len(cases), np.uint8), 1), ("every other", alt, 3), ("all", np.ones(len(cases), np.uint8), 1)):
        for rep in range(reps):
            b = gpu_ctx.stage(P, *_inputs(cases))
            tasks, _ = b.class_stats()
            assert tasks[15] > 0 and (tasks[12:15] > 0).sum() >= 2 and tasks[18] > 0 and tasks[12:19].sum() == tasks.sum() == len(cases), tasks
            scaled = b.segment_arith()[1].copy()
            b.debug_refuse(mark)
            capfd.readouterr()
            b.run(), b.finish()
            again = _reruns(capfd)
            out = _fetch(b)
            b.close()
            assert not out["res"]["status"].any() and out["stage"] == _lib.FINISH_DEVICE
            if what == "none":
                natural, natural_again = scaled & (1 - out["arith"]), sum(again.values())
                assert natural.sum() <= natural_again <= 2, (natural, again)
            else:
                assert np.array_equal(out["arith"], scaled & (1 - mark) & (1 - natural)), (what, rep)
                assert mark.sum() <= sum(again.values()) <= mark.sum() + natural_again, (what, again)
                # every class of the batch had its second launch
                assert set(again) == set(np.nonzero(tasks)[0].tolist()), (what, again, tasks)
                _same_batch(out, got["none"], (what, rep))
            got[what] = out
    # ... and the unmarked batch against the two bars, so that "the same" is also "right"
    h = oracle_hmm()
    PO = orc.make_params(**MIXED_KW)
    poff, px, py, pp = got["every other"]["pairs"]
    off, ops = got["every other"]["ops_off"], got["every other"]["ops"]
    for i, (X, Y, g) in enumerate(cases):
        m32 = orc.realign_read(h, PO, X, Y, g, precision=1, seg_arith=[int(got["every other"]["arith"][i])])
        m64 = orc.realign_read(h, PO, X, Y, g, precision=0)
        s = slice(poff[i], poff[i + 1])
        gp, mp, dp = _pairs_dict(px[s], py[s], pp[s]), _pairs_dict(m32["px"], m32["py"], m32["pp"].astype(np.float32)), _pairs_dict(m64["px"], m64["py"], m64["pp"])
        assert gp.keys() == mp.keys() and all(np.float32(gp[k]) == np.float32(mp[k]) for k in gp), i
        assert [tuple(int(v) for v in r) for r in ops[off[i]:off[i + 1]]] == m32["ops"], i
        for k in set(gp) | set(dp):
            a, c = gp.get(k), dp.get(k)
            assert abs((a if a is not None else 0.01) - (c if c is not None else 0.01)) < 1e-4
        assert got["every other"]["res"]["loglik"][i] == pytest.approx(m64["total_ll"], rel=2e-6)


@gpu
@pytest.mark.parametrize("mode", ["realign", "rescore", "all_posteriors"])
def test_every_finish_reads_the_second_pass_s_results(gpu_ctx, mode):
    """The mixed batch with every other task of every class refused, finished on the device and (NPR_OPT_HOST_MEA) on the host, in the three modes
    that finish: the same ops, scores, pair counts and pairs, each from the stage that was asked; the statistics of the cigars where they lie and
    the cigars as text (NPR_OPT_FINISH_TEXT) are those of the batch left alone; a rescored guide's score is the oracle's sum over the pairs."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    cases = _mixed_cases()
    P = R.make_params(mode={"realign": R.MODE_REALIGN, "rescore": R.MODE_RESCORE_ORIGINAL, "all_posteriors": R.MODE_ALL_POSTERIORS}[mode], **MIXED_KW)
    cells = [orc.plan(len(X), len(Y), g, orc.make_params(**MIXED_KW))[0]["cells"] for X, Y, g in cases]
    alt = _every_other_of_every_class(cells)

    def run(mark, **options):
        with gpu_ctx.options(**options):
            b = gpu_ctx.stage(P, *_inputs(cases))
            scaled = b.segment_arith()[1].copy()
            b.debug_refuse(mark)
            b.run(), b.finish()
            stats = b.align_stats()
            text, toff = b.cigar_text()
            out = _fetch(b)
            b.close()
        out.update(stats=stats, text=bytes(text), text_off=toff, scaled=scaled)
        return out

    base = run(np.zeros(len(cases), np.uint8))
    dev, host, text = run(alt), run(alt, host_mea=1), run(alt, finish_text=1)
    assert not dev["res"]["status"].any()
    assert base["stage"] == dev["stage"] == text["stage"] == _lib.FINISH_DEVICE and host["stage"] == _lib.FINISH_HOST
    for o in (dev, host, text):
        assert np.array_equal(o["arith"], base["arith"] & (1 - alt)) and (o["scaled"] & alt).sum() >= 5
        _same_batch(o, base, mode)
        assert np.array_equal(o["stats"], base["stats"]), mode
        assert o["text"] == base["text"] and np.array_equal(o["text_off"], base["text_off"]), mode
    assert (dev["stats"][:, 3] > 0).all() and len(dev["text"]) > len(cases)
    if mode == "rescore":
        poff, px, py, pp = dev["pairs"]
        for i, (X, Y, g) in enumerate(cases):
            s = slice(poff[i], poff[i + 1])
            assert dev["res"]["score"][i] == orc.rescore(np.asarray(g, dtype=np.int32), px[s], py[s], pp[s]), i
            o = dev["ops"][dev["ops_off"][i]:dev["ops_off"][i + 1]]
            assert [tuple(int(v) for v in r) for r in o] == [(op, k) for op, k in g if k > 0]


# ---- e. a pair list that overflows in the second pass ----

@gpu
def test_a_pair_list_that_overflows_in_the_second_pass(gpu_ctx, monkeypatch):
    """One pair per base of capacity against the ~1.8 a read of 600 bases has, every task refused: k_dp_stair reports the overflow as the first pass
    did -- NPR_ERR_CAPACITY per read at the C ABI, no batch error --, the short reads beside them (whose lists fit in the 64 spare entries) are
    untouched, and Context.realign, every run of which is refused again, ends with the answer of a roomy run."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    rng = np.random.default_rng(4500)
    cases = [random_pair(rng, n) for n in (600, 30, 600, 45, 600, 25)]
    inp = _inputs(cases)
    tight = R.make_params(band_mode=1, fixed_width=100, max_pairs_per_base=1)
    roomy = gpu_ctx.realign(R.make_params(band_mode=1, fixed_width=100), *inp, want_pairs=True)
    assert all(o["status"] == 0 and o["seg_arith"] == [1] for o in roomy)
    b = gpu_ctx.stage(tight, *inp)
    b.debug_refuse(np.ones(len(cases), np.uint8))
    b.run(), b.finish()
    out = _fetch(b, pairs=False)
    b.close()
    assert list(out["res"]["status"]) == [_lib.ERR_CAPACITY, 0] * 3 and not out["arith"].any()
    for i in (1, 3, 5):
        assert [tuple(int(v) for v in r) for r in out["ops"][out["ops_off"][i]:out["ops_off"][i + 1]]] == roomy[i]["ops"]
        assert out["res"]["loglik"][i] == roomy[i]["loglik"] and out["res"]["score"][i] == roomy[i]["score"]
    with refusing(monkeypatch, lambda off, scaled: np.ones(int(off[-1]), np.uint8)) as log:
        again = gpu_ctx.realign(tight, *inp, want_pairs=True)
    assert len(log) >= 2 and all(e["mark"].all() for e in log)      # the reads that overflowed were staged again, and refused again
    for i, (u, v) in enumerate(zip(again, roomy)):
        assert u["seg_arith"] == [0]
        _same_answers(u, v, i)


# ---- the work queue of the second launch ----

@gpu
def test_more_refused_tasks_than_the_second_launch_has_workgroups(gpu_ctx, capfd, monkeypatch):
    """A class of more tasks than its launch has workgroups (k_dp_mid_rs<1>: 12 per compute unit), most of them refused: the second launch is as
    wide as the first, and what its workgroups do not start with they take from the first launch's queue counter, which must count from zero
    again.  Against the batch left alone."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    monkeypatch.setenv("NPR_TIMING", "1")
    n = 4096                                                          # (256 compute units: 3072 workgroups; staging says below how many it is)
    rng = np.random.default_rng(4600)
    cases = [random_pair(rng, int(L)) for L in rng.integers(36, 56, size=n)]
    inp = _inputs(cases)
    mark = (rng.random(n) < 0.9).astype(np.uint8)
    P = R.make_params(band_mode=1, fixed_width=40)
    got, natural = [], 0
    for m in (np.zeros(n, np.uint8), mark):
        capfd.readouterr()
        b = gpu_ctx.stage(P, *inp)
        grid = int(re.search(r"\[npr\] class 12 \(.*\): \d+ tasks, .* grid (\d+) x", capfd.readouterr().err).group(1))
        tasks, _ = b.class_stats()
        assert tasks[12] >= grid + grid // 4 and tasks[12] + tasks[15] == n, (tasks, grid)   # (a read that lost a dozen bases has fewer than 64 anti-diagonals)
        b.debug_refuse(m)
        capfd.readouterr()
        b.run(), b.finish()
        again = _reruns(capfd)
        got.append(_fetch(b))
        b.close()
        assert not got[-1]["res"]["status"].any()
        assert m.sum() <= sum(again.values()) <= m.sum() + natural and set(again) <= {12, 15}, (again, m.sum(), natural)
        if not m.any():
            natural = sum(again.values())
            assert natural <= 8
    assert again[12] > grid + 64                                      # more than one task per workgroup of the second launch
    assert (got[1]["arith"][mark == 1] == 0).all() and (got[1]["arith"] == 0).sum() <= mark.sum() + natural
    _same_batch(got[1], got[0])


# ---- f. the stripe class's own exits ----

@gpu
def test_a_stripe_band_without_probability_is_reported_by_the_per_cell_kernel(gpu_ctx, capfd, monkeypatch):
    """test_band_without_probability_is_reported_by_the_per_cell_kernel on the stripe class (a band of 261 cells): a column-scaled task whose forward
    sweep ends with nothing leaves by k_dp_tile_cs's `!alive` exit, runs again in k_dp_tile, and NPR_ERR_ZERO_PROB comes from there; its twin
    without the substitution aligns in the first pass.  (Both report arithmetic 0, as every stripe does: the run's report says which one ran again.)"""
    from nanopore_amd import realign as R
    from nanopore_amd.hmm import Hmm
    T = np.zeros(25)
    T[0] = 1.0                                   # match -> match only
    E = np.zeros(80)
    for s in range(5):
        for c in range(4):
            E[16 * s + 5 * c] = 0.25             # every state emits identical bases only
    hm = Hmm()
    hm.transitions, hm.emissions = [float(v) for v in T], [float(v) for v in E]
    gpu_ctx.set_hmm(hm)
    monkeypatch.setenv("NPR_TIMING", "1")
    try:
        X = np.random.default_rng(4700).integers(0, 4, size=400).astype(np.uint8)
        Y = X.copy()
        Y[200] = (Y[200] + 1) % 4
        for reads, want in (([Y, X], 1), ([X, X], 0)):
            b = gpu_ctx.stage(R.make_params(band_mode=1, fixed_width=520), [_ascii(X)] * 2, [_ascii(r) for r in reads], [[(0, 400)]] * 2)
            assert b.class_stats()[0][18] == 2
            capfd.readouterr()
            b.run(), b.finish()
            again = _reruns(capfd)
            out = _fetch(b, pairs=False)
            b.close()
            assert again == ({18: 1} if want else {}), again
            assert list(out["res"]["status"]) == [_lib.ERR_ZERO_PROB if want else 0, 0] and list(out["arith"]) == [0, 0]
            assert [tuple(int(v) for v in r) for r in out["ops"][out["ops_off"][1]:out["ops_off"][2]]] == [(0, 400)]
    finally:
        gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))


def _indel_pair(rng, gap):
    """a reference with `gap` bases the read lacks and, 400 bases on, a read with `gap` bases the reference lacks, under a guide that knows of neither
    (the construction of test_row_scaled_task_without_its_range_certificate_runs_again_per_cell)"""
    core = rng.integers(0, 4, size=1200).astype(np.uint8)
    X = np.concatenate([core[:400], rng.integers(0, 4, size=gap).astype(np.uint8), core[400:]])
    Y = np.concatenate([core[:800], rng.integers(0, 4, size=gap).astype(np.uint8), core[800:]])
    return X, Y, [(0, len(X))]


CERTIFICATE_GAPS = (100, 200, 300, 450)


@gpu
def test_stripe_tasks_with_long_indels_and_their_certificate(gpu_ctx, capfd, monkeypatch):
    """Reads with a deletion and, 400 bases on, an insertion of the same length that the guide knows nothing of, 100 / 200 / 300 / 450 bases, in a
    band of 501 cells: the construction that costs the frame classes their certificate from 235 bases on.  Every read matches the mirror of the
    arithmetic it reports and the fp64 oracle to 1e-4, and the realigned cigar has both indels.
    This test does NOT require that one of them runs again.  On the MI355X k_dp_tile_cs kept its certificate on every length tried: 50 to 450 in
    steps of 50 in this band, and 600, 800, 1000, 1200 and 1500 in a band of 1601 cells -- no task came back TASK_RERUN, so there is no refused
    length and no certificate value to record (the run reports the value of refused tasks only; forward and backward totals agreed to 2e-9
    relative throughout).  One exponent per lane follows a long gap where one per anti-diagonal row cannot.  The stripe class's second pass is
    therefore covered by the hook (the tests above) and by the `!alive` exit (test_a_stripe_band_without_probability_...); the line printed here
    shows a refusal if a later kernel change produces one."""
    from nanopore_amd import realign as R
    gpu_ctx.set_hmm(_hmm_obj("blasr_hmm_0.txt"))
    monkeypatch.setenv("NPR_TIMING", "1")
    h = oracle_hmm()
    rng = np.random.default_rng(4800)
    cases = [_indel_pair(rng, gap) for gap in CERTIFICATE_GAPS]
    kw = dict(band_mode=1, fixed_width=1000)
    b = gpu_ctx.stage(R.make_params(**kw), *_inputs(cases))
    assert b.class_stats()[0][18] == len(cases)
    b.close()
    capfd.readouterr()
    out = gpu_ctx.realign(R.make_params(**kw), *_inputs(cases), want_pairs=True)
    err = capfd.readouterr().err
    refused = re.findall(r"\[npr\] task (\d+) \(D (\d+)\) runs again.*its certificate value\) (-?\d+)", err)
    print("tasks without their certificate (task, D, certificate value):", refused)
    P = orc.make_params(**kw)
    for (X, Y, g), o, gap in zip(cases, out, CERTIFICATE_GAPS):
        assert o["seg_arith"] == [0]
        m32 = orc.realign_read(h, P, X, Y, g, precision=1, seg_arith=o["seg_arith"])
        m64 = orc.realign_read(h, P, X, Y, g, precision=0)
        assert o["status"] == 0 and o["ops"] == m32["ops"], gap
        gp, mp, dp = _pairs_dict(o["x"], o["y"], o["p"]), _pairs_dict(m32["px"], m32["py"], m32["pp"].astype(np.float32)), _pairs_dict(m64["px"], m64["py"], m64["pp"])
        assert gp.keys() == mp.keys() and all(np.float32(gp[k]) == np.float32(mp[k]) for k in gp), gap
        for k in set(gp) | set(dp):
            a, c = gp.get(k), dp.get(k)
            assert abs((a if a is not None else 0.01) - (c if c is not None else 0.01)) < 1e-4
        assert o["loglik"] == pytest.approx(m64["total_ll"], rel=2e-6)
        assert any(op == 2 and n >= gap - 5 for op, n in o["ops"]) and any(op == 1 and n >= gap - 5 for op, n in o["ops"]), (gap, o["ops"])

"""SAM CIGAR text made on the device (csrc/npr_cigtext.hip; include/nprealign.h: npr_cigar_text_packed, npr_batch_cigar_text,
NPR_OPT_FINISH_TEXT; job.realign_sam_file(device_text=True)) against the host formatter npr_format_cigars_packed / npr_sam_splice, and for
the seeded lists against a restatement of the grammar in the test ("%d%s" per operation, "*" for none: what realignSamFile3TargetFn's
`aR.cigar = ...` makes pysam print, nanopore/analyses/utils.py:597-605).  Equality is exact: bytes and offsets."""
import os

import numpy as np
import pytest

from helpers import MODEL_DIR, load_model_arrays
from nanopore_amd import _lib
from nanopore_amd._lib import NprError, ptr

pytestmark = pytest.mark.gpu

LIST_SIZES = [0, 1, 63, 64, 65, 4096, 200003]
LENGTHS = [0, 1, 9, 10, 99, 100, 999, 1000, 9999, 10000, 99999, 100000, 999999, 1000000, 9999999, 10000000, 99999999, 100000000,
           999999999, 1000000000, (1 << 30) - 1]


def _seeded_lists(seed=11):
    """(word_off, n_ops, words): the sizes of LIST_SIZES and 250 small lists, placed in `words` in a shuffled order with gaps between them."""
    rng = np.random.default_rng(seed)
    nops = np.array(LIST_SIZES + [int(k) for k in rng.integers(0, 300, size=250)], dtype=np.int64)
    nops = nops[rng.permutation(len(nops))]
    n = len(nops)
    woff = np.zeros(n, dtype=np.int64)
    at = 5
    for i in rng.permutation(n):
        woff[i] = at
        at += int(nops[i]) + int(rng.integers(0, 4))
    words = np.full(at + 3, 0xffffffff, dtype=np.uint32)  # (the gaps hold an operation code no list may have)
    lens = np.array(LENGTHS, dtype=np.uint32)
    for i in range(n):
        k = int(nops[i])
        # mostly short runs, as a realigned read's are; every length of LENGTHS somewhere
        ln = np.where(rng.random(k) < 0.7, rng.integers(1, 30, size=k), lens[rng.integers(0, len(lens), size=k)]).astype(np.uint32)
        words[woff[i]:woff[i] + k] = (ln << 2) | rng.integers(0, 3, size=k).astype(np.uint32)
    return woff, nops, words


def _restated(woff, nops, words, i):
    return "".join("%d%s" % (int(w) >> 2, "MID"[int(w) & 3]) for w in words[woff[i]:woff[i] + nops[i]]) or "*"


def _raw(ctx, woff, nops, words, out, cap):
    str_off = np.full(len(nops) + 1, -7, dtype=np.int64)
    rc = _lib.load().npr_cigar_text_packed(ctx._h, len(nops), ptr(woff), ptr(nops), ptr(words), ptr(str_off), ptr(out), cap)
    return rc, str_off


def test_seeded_lists_equal_the_host_formatter(gpu_ctx):
    from nanopore_amd import realign as R
    woff, nops, words = _seeded_lists()
    n = len(nops)
    # what the lists contain
    used = np.concatenate([words[woff[i]:woff[i] + nops[i]] for i in range(n)])
    assert {len(str(int(w) >> 2)) for w in used} == set(range(1, 11))
    assert {int(w) >> 2 for w in used} >= set(LENGTHS) and {int(w) & 3 for w in used} == {0, 1, 2}
    assert set(LIST_SIZES) <= {int(k) for k in nops} and nops.max() >= 200000
    order = np.argsort(woff, kind="stable")
    assert (np.diff(woff) < 0).any()                                                 # out of order
    assert (woff[order][1:] > (woff + nops)[order][:-1]).any() and woff.min() > 0    # gaps
    want, want_off = R.format_cigars_packed(woff, nops, words)
    assert want_off[-1] > 64 * 1024
    got, got_off = R.cigar_text_packed(gpu_ctx, woff, nops, words)
    assert np.array_equal(got_off, want_off)
    assert bytes(got) == bytes(want)
    for i in list(range(0, n, 17)) + [int(np.argmax(nops)), int(np.argmin(nops))]:
        assert bytes(got[got_off[i]:got_off[i + 1]]).decode() == _restated(woff, nops, words, i), i
    # a second call: the same bytes
    again, again_off = R.cigar_text_packed(gpu_ctx, woff, nops, words)
    assert bytes(again) == bytes(got) and np.array_equal(again_off, got_off)
    # out == NULL: the host's offsets; one byte short: NPR_ERR_CAPACITY, nothing written
    total = int(want_off[-1])
    rc, off = _raw(gpu_ctx, woff, nops, words, None, 0)
    assert rc == total and np.array_equal(off, want_off)
    buf = np.full(total + 9, 0xa5, dtype=np.uint8)
    rc, off = _raw(gpu_ctx, woff, nops, words, buf, total - 1)
    assert rc == _lib.ERR_CAPACITY and (buf == 0xa5).all() and np.array_equal(off, want_off)
    rc, off = _raw(gpu_ctx, woff, nops, words, buf, total)
    assert rc == total and bytes(buf[:total]) == bytes(want) and (buf[total:] == 0xa5).all()


def test_empty_input_and_malformed_lists(gpu_ctx):
    from nanopore_amd import realign as R
    L = _lib.load()
    off = np.full(1, -7, dtype=np.int64)
    z64, z32 = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.uint32)
    assert L.npr_cigar_text_packed(gpu_ctx._h, 0, ptr(z64), ptr(z64), ptr(z32), ptr(off), None, 0) == 0 and off[0] == 0
    assert L.npr_cigar_text_packed(gpu_ctx._h, -1, ptr(z64), ptr(z64), ptr(z32), ptr(off), None, 0) == _lib.ERR_INVALID
    # only empty lists
    got, got_off = R.cigar_text_packed(gpu_ctx, np.zeros(5, dtype=np.int64), np.zeros(5, dtype=np.int64), z32)
    assert bytes(got) == b"*****" and list(got_off) == [0, 1, 2, 3, 4, 5]
    # an operation code 3 in one list: NPR_ERR_INVALID and the output untouched, from the host formatter too
    woff, nops, words = _seeded_lists(12)
    good, good_off = R.format_cigars_packed(woff, nops, words)
    i = int(np.argmax(nops))
    was = words[woff[i] + 150000]
    words[woff[i] + 150000] |= 3
    with pytest.raises(NprError) as e:
        R.format_cigars_packed(woff, nops, words)
    assert e.value.code == _lib.ERR_INVALID
    buf = np.full(len(good) + 4, 0xa5, dtype=np.uint8)
    rc, _ = _raw(gpu_ctx, woff, nops, words, buf, buf.nbytes)
    assert rc == _lib.ERR_INVALID and (buf == 0xa5).all()
    rc, _ = _raw(gpu_ctx, woff, nops, words, None, 0)
    assert rc == _lib.ERR_INVALID
    # a negative count
    words[woff[i] + 150000] = was
    nops2 = nops.copy()
    nops2[3] = -1
    rc, _ = _raw(gpu_ctx, woff, nops2, words, buf, buf.nbytes)
    assert rc == _lib.ERR_INVALID and (buf == 0xa5).all()
    # ... and the context is as good as before
    got, got_off = R.cigar_text_packed(gpu_ctx, woff, nops, words)
    assert bytes(got) == bytes(good) and np.array_equal(got_off, good_off)


def _workload():
    """64 reads of ~1.5 kb; the guide of read 5 stops one base short of its sequences (not global: the read fails)."""
    from nanopore_amd import synth
    T, E, _ = load_model_arrays()
    w = synth.make_workload(77, 64, 1500, T, E, flank=0, length_sigma=0.4, len_min=200, len_max=4000)
    guide_ops = w["guide_ops"].reshape(-1, 2).copy()
    last = int(w["guide_off"][6]) - 1
    assert guide_ops[last, 1] > 1
    guide_ops[last, 1] -= 1
    return w, guide_ops


def _bands(R, mode):
    """The frame kernels' band (fixed width) and the reference's own (anchors, trimmed, split)."""
    return (R.make_params(band_mode=R.BAND_FIXED, fixed_width=100, mode=mode),
            R.make_params(band_mode=R.BAND_ANCHOR, constraint_trim=4, split_threshold=60, max_pairs_per_base=40, mode=mode))


def _finished(ctx, P, w, guide_ops):
    b = ctx.stage_csr(P, w["ref"], w["ref_off"], w["read"], w["read_off"], guide_ops, w["guide_off"])
    b.run(), b.finish()
    return b


def _check_text_of(b, R):
    """cigar_text() of a finished batch against the host formatter over its ops_packed(); -> (text bytes, offsets, results)."""
    off, words = b.ops_packed()
    want, want_off = R.format_cigars_packed(off[:-1], np.diff(off), words)
    text, str_off = b.cigar_text()
    assert np.array_equal(str_off, want_off) and bytes(text) == bytes(want)
    res = b.results()
    assert res["status"][5] != 0 and (np.delete(res["status"], 5) == 0).all()
    assert bytes(text[str_off[5]:str_off[6]]) == b"*" and off[6] == off[5]
    assert (np.diff(off)[res["status"] == 0] > 0).all() and len(text) > 1000
    return bytes(text), str_off, res


@pytest.mark.parametrize("mode", ["realign", "rescore_original", "all_posteriors"])
def test_batch_text_equals_the_formatted_packed_cigars(gpu_ctx, mode):
    from nanopore_amd import realign as R
    from nanopore_amd.hmm import Hmm
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    w, guide_ops = _workload()
    mode = dict(realign=R.MODE_REALIGN, rescore_original=R.MODE_RESCORE_ORIGINAL, all_posteriors=R.MODE_ALL_POSTERIORS)[mode]
    for P in _bands(R, mode):
        first = gpu_ctx.stage_csr(P, w["ref"], w["ref_off"], w["read"], w["read_off"], guide_ops, w["guide_off"])
        second = None
        try:
            with pytest.raises(NprError) as e:
                first.cigar_text()
            assert e.value.code == _lib.ERR_STATE
            first.run(), first.finish()
            # a second batch runs and finishes on the same context before the first is asked for its text: what the first left on the device
            # is stale and its host form goes up; the second's words are formatted where they lie
            second = _finished(gpu_ctx, P, w, guide_ops)
            t1, o1, r1 = _check_text_of(first, R)
            t2, o2, r2 = _check_text_of(second, R)
            assert t1 == t2 and np.array_equal(o1, o2)
            # asked again: the same
            again, again_off = first.cigar_text()
            assert bytes(again) == t1 and np.array_equal(again_off, o1)
        finally:
            first.close()
            if second is not None:
                second.close()
        # ... and one that is asked right after its own finish
        b = _finished(gpu_ctx, P, w, guide_ops)
        try:
            t3, o3, _ = _check_text_of(b, R)
            assert t3 == t1 and np.array_equal(o3, o1)
        finally:
            b.close()


@pytest.mark.parametrize("mode", ["realign", "all_posteriors"])
def test_finish_text_option(gpu_ctx, mode):
    """NPR_OPT_FINISH_TEXT = 1: the text crosses PCIe instead of the words.  The same text, the same results, the same words on demand
    while they are on the device -- and a clear NPR_ERR_STATE once another batch's finish has overwritten them."""
    from nanopore_amd import realign as R
    from nanopore_amd.hmm import Hmm
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    w, guide_ops = _workload()
    mode = dict(realign=R.MODE_REALIGN, all_posteriors=R.MODE_ALL_POSTERIORS)[mode]
    for P in _bands(R, mode):
        b = _finished(gpu_ctx, P, w, guide_ops)
        try:
            want_text, want_off, want_res = _check_text_of(b, R)
            want_ops_off, want_words = b.ops_packed()
            want_pairs = b.ops()
        finally:
            b.close()
        with gpu_ctx.options(finish_text=1):
            b = _finished(gpu_ctx, P, w, guide_ops)
            other = None
            try:
                off, words = b.ops_packed()                      # right after finish: fetched from the device
                assert np.array_equal(off, want_ops_off) and np.array_equal(words, want_words)
                res = b.results()
                for k in ("status", "score", "n_ops", "n_pairs", "loglik", "cells"):
                    assert np.array_equal(res[k], want_res[k]), k
                text, str_off = b.cigar_text()
                assert bytes(text) == want_text and np.array_equal(str_off, want_off)
                got_pairs = b.ops()
                assert np.array_equal(got_pairs[0], want_pairs[0]) and np.array_equal(got_pairs[1], want_pairs[1])
                b.close()
                # a batch that is not asked for its words before the next one has finished: the text is there, the words are gone
                b = _finished(gpu_ctx, P, w, guide_ops)
                other = _finished(gpu_ctx, P, w, guide_ops)
                text, str_off = b.cigar_text()
                assert bytes(text) == want_text and np.array_equal(str_off, want_off)
                with pytest.raises(NprError) as e:
                    b.ops_packed()
                assert e.value.code == _lib.ERR_STATE and "NPR_OPT_FINISH_TEXT" in str(e.value)
                with pytest.raises(NprError) as e:
                    b.ops()
                assert e.value.code == _lib.ERR_STATE
                off, words = other.ops_packed()
                assert np.array_equal(off, want_ops_off) and np.array_equal(words, want_words)
            finally:
                b.close()
                if other is not None:
                    other.close()
        # the host stage is not affected by the option
        with gpu_ctx.options(finish_text=1, host_mea=1):
            b = _finished(gpu_ctx, P, w, guide_ops)
            try:
                t, o, _ = _check_text_of(b, R)
                assert t == want_text and np.array_equal(o, want_off)
            finally:
                b.close()


def _noisy_batch(seed, n_reads, lmin, lmax, indel, max_indel=3, sub=0.1):
    """CSR buffers for Context.stage_csr: references of lmin .. lmax random bases and noisy copies of them (helpers.random_pair's channel,
    drawn with numpy: thousands of reads in a second), the true alignments as global guides."""
    rng = np.random.default_rng(seed)
    ascii_of = np.frombuffer(b"ACGT", dtype=np.uint8)
    refs, reads, guides = [], [], []
    for _ in range(n_reads):
        L = int(rng.integers(lmin, lmax + 1))
        r = rng.random(L)                                     # at most L events consume L reference bases
        kind = np.where(r < indel / 2, 2, np.where(r < indel, 1, 0)).astype(np.int32)
        klen = np.where(kind == 0, 1, rng.integers(1, max_indel + 1, size=L)).astype(np.int32)
        m = int(np.searchsorted(np.cumsum(np.where(kind != 1, klen, 0)), L)) + 1   # the events up to the one that reaches L reference bases
        kind, klen = kind[:m], klen[:m]
        x_adv, y_adv = np.where(kind != 1, klen, 0), np.where(kind != 2, klen, 0)
        X = rng.integers(0, 4, size=int(x_adv.sum())).astype(np.uint8)
        Y = rng.integers(0, 4, size=int(y_adv.sum())).astype(np.uint8)
        match = kind == 0
        copied = X[(np.cumsum(x_adv) - x_adv)[match]]
        copied = np.where(rng.random(copied.size) < sub, (copied + rng.integers(1, 4, size=copied.size)) % 4, copied)
        Y[(np.cumsum(y_adv) - y_adv)[match]] = copied
        first = np.flatnonzero(np.concatenate([[True], kind[1:] != kind[:-1]]))   # runs of the same operation, merged
        refs.append(ascii_of[X]), reads.append(ascii_of[Y])
        guides.append(np.stack([kind[first], np.add.reduceat(klen, first)], axis=1))
    off = lambda parts: np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return (np.concatenate(refs), off(refs), np.concatenate(reads), off(reads), np.concatenate(guides).astype(np.int32), off(guides))


def test_hand_over_in_several_pieces(gpu_ctx):
    """A batch whose cigars cross PCIe in more than one piece of the pinned staging, the last piece partial, in the three forms the device
    MEA stage hands them over in: 16-bit words (the default), whole words (mea_wide_ops), text (finish_text, the words fetched from the device
    afterwards).  The same words as the host stage's, and the text the host formatter makes of them."""
    from nanopore_amd import realign as R
    from nanopore_amd.hmm import Hmm
    gpu_ctx.set_hmm(Hmm.loadHmm(MODEL_DIR + "/blasr_hmm_0.txt"))
    csr = _noisy_batch(41, 3600, 2000, 3000, indel=0.3)
    P = R.make_params(band_mode=R.BAND_FIXED, fixed_width=100)
    got = {}
    for name, opts in (("narrow", {}), ("wide", dict(mea_wide_ops=1)), ("text", dict(finish_text=1)), ("host", dict(host_mea=1))):
        with gpu_ctx.options(**opts):
            b = gpu_ctx.stage_csr(P, *csr)
            try:
                b.run(), b.finish()
                text = b.cigar_text() if name == "text" else None   # (made by the finish: asked for before the words come over)
                got[name] = b.ops_packed() + (b.results()["status"].copy(), text)
            finally:
                b.close()
    off, words, status, _ = got["host"]
    assert (status == 0).all()
    assert off[-1] > 2 ** 21 and off[-1] % (1 << 20) != 0   # two pieces or more of 2^20 words, the last one partial
    for name in ("narrow", "wide", "text"):
        assert np.array_equal(got[name][0], off) and np.array_equal(got[name][1], words) and np.array_equal(got[name][2], status), name
    want, want_off = R.format_cigars_packed(off[:-1], np.diff(off), words)
    assert want_off[-1] > 4 << 20                           # two pieces or more of 4 MiB
    text, str_off = got["text"][3]
    assert np.array_equal(str_off, want_off) and bytes(text) == bytes(want)


def test_job_with_device_text_writes_the_same_file(tmp_path, monkeypatch):
    from test_gpu_job import HMM0, _c3_files
    from nanopore_amd import job
    n = 768
    w, sam, fa, fq = _c3_files(str(tmp_path), n, True)
    monkeypatch.setattr(job, "CHUNK_BASES", 700000)             # ~8 chunks on three contexts
    words_out, text_out = str(tmp_path / "words.sam"), str(tmp_path / "text.sam")
    try:
        a = job.realign_sam_file(sam, words_out, fa, hmm=HMM0)
        b = job.realign_sam_file(sam, text_out, fa, hmm=HMM0, device_text=True)
        want = open(words_out, "rb").read()
        assert open(text_out, "rb").read() == want and want.count(b"\n") == n + len(w["ref_off"])
        assert a["timings"]["chunks"] > 3 and b["timings"]["chunks"] == a["timings"]["chunks"]
        for k in ("status", "score", "n_ops", "loglik", "cells"):
            assert np.array_equal(a["results"][k], b["results"][k]), k
        assert np.array_equal(a["n_ops"], b["n_ops"]) and (a["results"]["status"] == 0).all()
        # the contexts are left as they were found: the next job ships words again
        c = job.realign_sam_file(sam, text_out, fa, hmm=HMM0)
        assert open(text_out, "rb").read() == want and np.array_equal(c["n_ops"], a["n_ops"])
        # one chunk, one worker
        monkeypatch.setattr(job, "CHUNK_BASES", 1 << 40)
        monkeypatch.setattr(job, "WORKERS", 1)
        job.realign_sam_file(sam, text_out, fa, hmm=HMM0, device_text=True)
        assert open(text_out, "rb").read() == want
        with pytest.raises(ValueError):
            job.realign_sam_file(sam, text_out, fa, hmm=HMM0, device_text=True, want_stats=True)
    finally:
        for pool in job._ctx_pool.values():   # (the job keeps its contexts; the tests after this one want the memory)
            for c in pool:
                if getattr(c, "_h", None):
                    c.release_scratch()


def test_sharded_job_refuses_device_text(tmp_path):
    import torch.distributed as dist
    from test_gpu_job import HMM0, _c3_files
    from nanopore_amd import job
    w, sam, fa, fq = _c3_files(str(tmp_path), 24, True, seed_genome=60000)
    out = str(tmp_path / "o.sam")
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        with pytest.raises(ValueError) as e:
            job.realign_sam_file(sam, out, fa, hmm=HMM0, device_text=True)
        assert "device_text" in str(e.value) and not os.path.exists(out)
    finally:
        dist.destroy_process_group()

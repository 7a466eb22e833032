"""Batched realignment API over the C ABI (libnprealign.so).

`Context.realign()` is the in-process replacement of the reference's per-read fan-out
(nanopore/analyses/utils.py:557-609: one jobTree job + one `cactus_realign` process per SAM record):
all reads of a SAM file go to the GPU in one call.  Device work only -- no CPU fallback.
"""
import contextlib
import ctypes as C
import weakref

import numpy as np

from . import _lib
from ._lib import (BAND_ANCHOR, BAND_FIXED, ERR_CAPACITY, ERR_NOMEM, MODE_ALL_POSTERIORS, MODE_EXPECTATIONS, MODE_REALIGN, MODE_RESCORE_ORIGINAL, NprError,
                   Params, _sized, check, ptr)


def make_params(band_mode=BAND_ANCHOR, diagonal_expansion=10, constraint_trim=14, split_threshold=3000,
                fixed_width=0, gap_gamma=0.5, match_gamma=0.0, posterior_threshold=0.01, mode=MODE_REALIGN,
                max_pairs_per_base=0):
    """Defaults are the realign call string of nanopore/analyses/utils.py:587 and
    AbstractMapper.realignSamFile's gammas (nanopore/mappers/abstractMapper.py:25)."""
    return Params(band_mode, diagonal_expansion, constraint_trim, split_threshold, fixed_width, gap_gamma,
                  match_gamma, posterior_threshold, mode, max_pairs_per_base)


def _arr(x, dtype, cols=None):
    """None for None, else x as a contiguous array of `dtype`, as rows of `cols` when that is given."""
    if x is None:
        return None
    a = np.ascontiguousarray(x, dtype=dtype)
    return a if cols is None else a.reshape(-1, cols)


def _csr(items, pad=False):
    """list of bytes / str / uint8 arrays -> (uint8 buffer, int64 offsets[n + 1]).  pad: a buffer without bytes becomes one zero byte,
    for the entry points that refuse a null pointer."""
    items = [s.encode("ascii") if isinstance(s, str) else s.astype(np.uint8).tobytes() if isinstance(s, np.ndarray) else s for s in items]
    off = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum(np.fromiter(map(len, items), dtype=np.int64, count=len(items)), out=off[1:])
    return np.frombuffer(b"".join(items) or (b"\0" if pad else b""), dtype=np.uint8), off


def _ragged(items):
    return _csr(items, pad=True)


class ReadQuality(object):
    """The six int64 tables of npr_read_quality (include/nprealign.h defines them), first axis = group: pos_qual [G, 336, 95],
    pos_base [G, 336, 5], len_hist [G, 336], meanq_hist [G, 95], gc_hist [G, 102], totals [G, 8]."""
    FIELDS = ("pos_qual", "pos_base", "len_hist", "meanq_hist", "gc_hist", "totals")
    TILE = _lib.RQ_TILE  # positions of one read a workgroup of the kernel takes per step

    def __init__(self, pos_qual, pos_base, len_hist, meanq_hist, gc_hist, totals):
        self.pos_qual, self.pos_base, self.len_hist, self.meanq_hist, self.gc_hist, self.totals = pos_qual, pos_base, len_hist, meanq_hist, gc_hist, totals

    @classmethod
    def zeros(cls, n_groups):
        B, Q = _lib.RQ_POS_BINS, _lib.RQ_QUAL_COLS
        return cls(*[np.zeros((n_groups,) + shape, dtype=np.int64) for shape in ((B, Q), (B, 5), (B,), (Q,), (_lib.RQ_GC_COLS,), (_lib.RQ_TOTALS,))])

    def arrays(self):
        return [getattr(self, f) for f in self.FIELDS]

    def group(self, g):
        """The tables of one group (no group axis), as fastqc.writeFastqcData takes them."""
        return ReadQuality(*[a[g] for a in self.arrays()])


class _Tables(object):
    """A set of int64 tables an entry point fills: FIELDS names them, in the order of its signature."""
    FIELDS = ()

    def __init__(self, *arrays):
        if len(arrays) != len(self.FIELDS):
            raise ValueError("one array per field: %s" % ", ".join(self.FIELDS))
        for f, a in zip(self.FIELDS, arrays):
            setattr(self, f, a)

    def arrays(self):
        return [getattr(self, f) for f in self.FIELDS]


class Coverage(_Tables):
    """The four int64 tables of npr_pileup_coverage (include/nprealign.h defines them): win [W, 8], depth_hist [336], start_hist [336],
    totals [8]."""
    FIELDS = ("win", "depth_hist", "start_hist", "totals")
    TILE = _lib.AQ_TILE  # consecutive rows a workgroup of the kernel takes

    @classmethod
    def zeros(cls, n_windows):
        B = _lib.RQ_POS_BINS
        return cls(*[np.zeros(shape, dtype=np.int64) for shape in ((n_windows, _lib.AQ_WIN_WORDS), (B,), (B,), (_lib.AQ_TOTALS,))])


class AlignQuality(_Tables):
    """The eight int64 tables of npr_align_quality (include/nprealign.h defines them): mapq_hist [256], win_mapq [W, 2], pos_base [336, 5],
    clip_hist [336], gc_hist [102], indel [2, 5], indel_len [2, 336], totals [8].  `invalid`: some record was malformed or ran past its
    sequences and was left out (only a call with allow_invalid hands such tables back)."""
    FIELDS = ("mapq_hist", "win_mapq", "pos_base", "clip_hist", "gc_hist", "indel", "indel_len", "totals")
    invalid = False

    @classmethod
    def zeros(cls, n_windows):
        B = _lib.RQ_POS_BINS
        return cls(*[np.zeros(shape, dtype=np.int64) for shape in ((256,), (n_windows, 2), (B, 5), (B,), (_lib.RQ_GC_COLS,), (2, 5), (2, B), (_lib.AQ_TOTALS,))])


def _csr_ops(guides):
    lens = np.fromiter((len(g) for g in guides), dtype=np.int64, count=len(guides))
    off = np.zeros(len(guides) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ops = np.zeros((int(off[-1]), 2), dtype=np.int32)
    for i, g in enumerate(guides):
        if len(g):
            ops[off[i]:off[i + 1]] = np.asarray(g, dtype=np.int32).reshape(-1, 2)
    return ops, off


def _host_alignments(refs, reads, cigars, ref_index, start):
    """Alignments given on the host, as npr_align_stats and npr_align_indel_kmers take them: (n_reads, n_refs, the eight arrays from
    `ref` to `start` in the order of both signatures)."""
    ref, ref_off = _csr(refs)
    read, read_off = _csr(reads)
    ops, ops_off = _csr_ops(cigars)
    return len(read_off) - 1, len(ref_off) - 1, (ref, ref_off, _arr(ref_index, np.int32), read, read_off, ops, ops_off, _arr(start, np.int64, 2))


def _packed_cigars(word_off, n_ops, words):
    """Packed cigars (one uint32 per op, length << 2 | op; list i at words[word_off[i] .. + n_ops[i])) as the library takes them."""
    return _arr(word_off, np.int64), _arr(n_ops, np.int64), _arr(words, np.uint32)


def _read_spans(text, name_span, begin, end):
    """Reads and their names as spans of one text (FastqTable.text / .name_span / .seq_span) as the library takes them."""
    return _arr(text, np.uint8), _arr(name_span, np.int64, 2), _arr(begin, np.int64), _arr(end, np.int64)


def _snp_calls(fn, where, ctx, head, rows, ref_code, true_code, evolution, errors):
    """The call the three SNP-call entry points share (include/nprealign.h: npr_snp_calls_table): fn(*head, ref_code, true_code, n_models,
    evolution16, error16, out) with one 4 x 4 error matrix [candidate, observed] per model in `errors` and the 4 x 4 `evolution`
    [reference, candidate], both as probabilities.  -> per model (true_pos int64[101], false_pos int64[101], not_called, rows_called)."""
    ref_code, true_code = _arr(ref_code, np.uint8), _arr(true_code, np.uint8)
    if ref_code is None or ref_code.shape != (rows,) or (true_code is not None and true_code.shape != (rows,)):
        raise ValueError("one reference base code (and one true base code) per table row")
    evolution, errors = _arr(evolution, np.float64), _arr(errors, np.float64)
    if evolution.size != 16 or errors.size % 16:
        raise ValueError("evolution is one 4 x 4 matrix, errors a list of 4 x 4 matrices")
    n_models = errors.size // 16
    out = (_lib.SnpCalls * max(n_models, 1))()
    check(fn(*head, ptr(ref_code), ptr(true_code), n_models, ptr(evolution), ptr(errors), C.byref(out)), where, ctx)
    return [(np.array(o.true_pos, dtype=np.int64), np.array(o.false_pos, dtype=np.int64), int(o.not_called), int(o.rows_called)) for o in out[:n_models]]


def _snp_variants(fn, where, ctx, head, rows, ref_code, evolution, error, threshold):
    """The call the three SNP-variant entry points share (include/nprealign.h: npr_snp_variants_table): fn(*head, ref_code, evolution16,
    error16, threshold, best, qual, call_row, call_alt, call_p, cap, n_calls) with the 4 x 4 `error` [candidate, observed] and `evolution`
    [reference, candidate], both as probabilities.  -> (best uint8[rows]: base code, 4 = no call possible; qual uint8[rows]: 0..93;
    call_row int64[n], call_alt uint8[n], call_p float64[n]: the calls in ascending (row, candidate) order).  Room for one call in
    sixteen rows is offered first; when there are more the library says how many and the call is made once more with that room."""
    ref_code = _arr(ref_code, np.uint8)
    if ref_code is None or ref_code.shape != (rows,):
        raise ValueError("one reference base code per table row")
    evolution, error = _arr(evolution, np.float64), _arr(error, np.float64)
    if evolution.size != 16 or error.size != 16:
        raise ValueError("evolution and error are one 4 x 4 matrix each")
    best, qual = np.empty(rows, dtype=np.uint8), np.empty(rows, dtype=np.uint8)
    n = C.c_int64(0)

    def call(cap):
        row, alt, p = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.uint8), np.empty(cap, dtype=np.float64)
        rc = fn(*head, ptr(ref_code), ptr(evolution), ptr(error), float(threshold), ptr(best), ptr(qual), ptr(row), ptr(alt), ptr(p), cap, C.byref(n))
        return rc, row, alt, p

    rc, row, alt, p = call(rows // 16 + 64)
    if rc == ERR_CAPACITY:
        rc, row, alt, p = call(n.value)
    count = int(check(rc, where, ctx))
    return best, qual, row[:count], alt[:count], p[:count]


class _Handle(object):
    """An object of the library that belongs to a Context (Batch, Pileup, SeedIndex, SeedMap): destroyed once, by close(), by the context's
    close() or when it is collected, whichever comes first."""
    _destroy = None  # the entry point that destroys the handle

    def _create(self, ctx, create, where, *args, made_from=None):
        """self._h = the handle `create`(ctx, *args, &handle) makes -- or `create`(made_from, *args, &handle), for an object the library
        makes from another handle of the same context."""
        self._L, self.ctx, self._h = _lib.load(), ctx, None
        h = C.c_void_p()
        check(getattr(self._L, create)((made_from or ctx)._h, *args, C.byref(h)), where, ctx)
        self._h = h
        ctx._open.add(self)

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch(_Handle):
    """A staged batch: inputs resident in HBM after construction."""
    _destroy = "npr_batch_destroy"

    def __init__(self, ctx, params, ref, ref_off, read, read_off, guide_ops, guide_off, model_slot=None,
                 ref_index=None, guide_start=None, read_end=None):
        model_slot, ref_index, guide_start = _arr(model_slot, np.int32), _arr(ref_index, np.int32), _arr(guide_start, np.int64, 2)
        n_refs = len(ref_off) - 1
        self._keep = (ref, ref_off, read, read_off, guide_ops, guide_off, model_slot, ref_index, guide_start, read_end)
        if read_end is not None:  # reads scattered in `read` (the SEQ fields of a mapped SAM text): read_off = their starts
            self.n_reads = len(read_off)
            self._create(ctx, "npr_batch_create_spans", "npr_batch_create", C.byref(params), self.n_reads, n_refs, ptr(ref), ptr(ref_off),
                         ptr(ref_index), ptr(read), ptr(read_off), ptr(read_end), ptr(guide_ops), ptr(guide_off), ptr(guide_start),
                         ptr(model_slot))
        else:
            self.n_reads = len(read_off) - 1
            self._create(ctx, "npr_batch_create_at", "npr_batch_create", C.byref(params), self.n_reads, n_refs, ptr(ref), ptr(ref_off),
                         ptr(ref_index), ptr(read), ptr(read_off), ptr(guide_ops), ptr(guide_off), ptr(guide_start), ptr(model_slot))

    def class_stats(self):
        """(tasks, cells) per kernel class (include/nprealign.h: npr_batch_class_stats)."""
        t = np.zeros(32, dtype=np.int64)
        c = np.zeros(32, dtype=np.int64)
        k = check(self._L.npr_batch_class_stats(self._h, ptr(t), ptr(c), 32), "npr_batch_class_stats", self.ctx)
        return t[:k], c[:k]

    def segment_arith(self):
        """-> (seg_off[n+1], arith): per segment of every read, in read order, the device arithmetic it ran in (0: one
        exponent per cell, 1: one per anti-diagonal row; include/nprealign.h: npr_batch_segment_arith)."""
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        check(self._L.npr_batch_segment_arith(self._h, ptr(off), None, 0), "npr_batch_segment_arith", self.ctx)
        ar = np.zeros(max(int(off[-1]), 1), dtype=np.int32)
        check(self._L.npr_batch_segment_arith(self._h, ptr(off), ptr(ar), len(ar)), "npr_batch_segment_arith", self.ctx)
        return off, ar[:int(off[-1])]

    def stats(self):
        st = _lib.BatchStats()
        check(self._L.npr_batch_get_stats(self._h, C.byref(st)), "npr_batch_get_stats", self.ctx)
        return {k: getattr(st, k) for k, _ in st._fields_}

    def run(self):
        """Device DP pass (forward + backward + posterior extraction).  Returns kernel milliseconds
        measured with HIP events on the library's stream."""
        ms = C.c_float(0)
        check(self._L.npr_batch_run(self._h, C.byref(ms)), "npr_batch_run", self.ctx)
        return ms.value

    def finish(self):
        check(self._L.npr_batch_finish(self._h), "npr_batch_finish", self.ctx)

    def results(self):
        out = np.zeros(self.n_reads, dtype=_lib.RESULT_DTYPE)
        assert out.dtype.itemsize == C.sizeof(_lib.ReadResult)
        check(self._L.npr_batch_results(self._h, ptr(out)), "npr_batch_results", self.ctx)
        return out

    def ops(self):
        """-> (ops_off[n+1], ops[k,2]) CSR of output cigars."""
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        check(self._L.npr_batch_ops(self._h, ptr(off), None, 0), "npr_batch_ops", self.ctx)
        ops = np.zeros((int(off[-1]), 2), dtype=np.int32)
        check(self._L.npr_batch_ops(self._h, ptr(off), ptr(ops), len(ops)), "npr_batch_ops", self.ctx)
        return off, ops

    def ops_packed(self):
        """Output cigars, one uint32 per op (length << 2 | op): (offsets[n+1], words)."""
        off, words, _ = self.ops_packed_into(None, slack=False)
        return off, words

    def ops_packed_into(self, buffer, slack=True):
        """ops_packed for a caller that fetches batch after batch: -> (offsets, words, buffer) -- the words are a view of `buffer`
        (a uint32 array or None) when it is large enough, else of a new, larger one, which is returned for the next call."""
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        check(self._L.npr_batch_ops_packed(self._h, ptr(off), None, 0), "npr_batch_ops_packed", self.ctx)
        total = int(off[-1])
        if buffer is None or buffer.size < max(total, 1):
            buffer = np.empty(max(total + (total // 4 if slack else 0), 1), dtype=np.uint32)  # (filled by the call: no memset first)
        check(self._L.npr_batch_ops_packed(self._h, ptr(off), ptr(buffer), total), "npr_batch_ops_packed", self.ctx)
        return off, buffer[:total], buffer

    def cigar_text(self, buffer=None):
        """Output cigars as SAM CIGAR text, formatted on the device (include/nprealign.h: npr_batch_cigar_text): (uint8 buffer, offsets[n+1]);
        string i = buffer[offsets[i]:offsets[i + 1]], "*" for a read that failed.  `buffer`: a uint8 array the text may be written into (a view
        of it is returned when it is large enough)."""
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        return _sized(self._L.npr_batch_cigar_text, "npr_batch_cigar_text", [self._h, ptr(off)], self.ctx, buffer), off

    def debug_set_pairs(self, read, x, y, p, task_status=0):
        """TEST HOOK (include/nprealign.h npr_batch_debug_set_pairs): replaces on the device the posterior pairs the DP pass left for `read`."""
        x, y, p = _arr(x, np.int32), _arr(y, np.int32), _arr(p, np.float32)
        check(self._L.npr_batch_debug_set_pairs(self._h, int(read), ptr(x), ptr(y), ptr(p), len(x), int(task_status)), "npr_batch_debug_set_pairs", self.ctx)

    def finish_stage(self):
        """TEST HOOK (include/nprealign.h npr_batch_debug_finish_stage): the stage the last finish() took, FINISH_DEVICE (0) or FINISH_HOST (1)."""
        return int(check(self._L.npr_batch_debug_finish_stage(self._h), "npr_batch_debug_finish_stage", self.ctx))

    def debug_refuse(self, mark):
        """TEST HOOK (include/nprealign.h npr_batch_debug_refuse): the next run() takes the scaled tasks of the marked segments (one entry per
        segment, in segment_arith()'s order) as refused by their range certificate and runs them again per cell."""
        mark = _arr(np.asarray(mark) != 0, np.uint8)
        check(self._L.npr_batch_debug_refuse(self._h, ptr(mark), len(mark)), "npr_batch_debug_refuse", self.ctx)

    def pairs(self):
        """-> (pair_off[n+1], x, y, p) sparse posterior match probabilities sorted by (x, y)."""
        off = np.zeros(self.n_reads + 1, dtype=np.int64)
        check(self._L.npr_batch_pairs(self._h, ptr(off), None, None, None, 0), "npr_batch_pairs", self.ctx)
        k = int(off[-1])
        x = np.zeros(k, dtype=np.int32)
        y = np.zeros(k, dtype=np.int32)
        p = np.zeros(k, dtype=np.float32)
        check(self._L.npr_batch_pairs(self._h, ptr(off), ptr(x), ptr(y), ptr(p), k), "npr_batch_pairs", self.ctx)
        return off, x, y, p

    def base_expectations(self, ref_lengths, use=None):
        """Posterior-weighted base counts per reference position of the (selected) reads, scattered on the device
        (include/nprealign.h: npr_batch_base_expectations): (expect[sum(ref_lengths), 4], seen[sum(ref_lengths)])."""
        ref_lengths = _arr(ref_lengths, np.int64)
        rows = int(ref_lengths.sum())
        expect = np.zeros((rows, 4), dtype=np.float64)
        seen = np.zeros(rows, dtype=np.uint8)
        u = _arr(use, np.uint8)
        check(self._L.npr_batch_base_expectations(self._h, ptr(u), len(ref_lengths), ptr(ref_lengths), ptr(expect), ptr(seen)),
              "npr_batch_base_expectations", self.ctx)
        return expect, seen.astype(bool)

    def snp_calls(self, ref_lengths, ref_code, true_code, evolution, errors, use=None):
        """SNP calls from the posterior-weighted base counts of the (selected) reads, made where k_base_expectations leaves the table: only
        the histograms leave the device (include/nprealign.h: npr_batch_snp_calls; _snp_calls for the matrices and what comes back)."""
        ref_lengths, u = _arr(ref_lengths, np.int64), _arr(use, np.uint8)
        if u is not None and len(u) != self.n_reads:
            raise ValueError("use must have one entry per read of the batch")
        return _snp_calls(self._L.npr_batch_snp_calls, "npr_batch_snp_calls", self.ctx, (self._h, ptr(u), len(ref_lengths), ptr(ref_lengths)),
                          int(ref_lengths.sum()), ref_code, true_code, evolution, errors)

    def snp_variants(self, ref_lengths, ref_code, evolution, error, threshold, use=None):
        """The SNP calls themselves and a best base with its quality per position, from the posterior-weighted base counts of the (selected)
        reads where k_base_expectations leaves them (include/nprealign.h: npr_batch_snp_variants; _snp_variants for what comes back)."""
        ref_lengths, u = _arr(ref_lengths, np.int64), _arr(use, np.uint8)
        if u is not None and len(u) != self.n_reads:
            raise ValueError("use must have one entry per read of the batch")
        return _snp_variants(self._L.npr_batch_snp_variants, "npr_batch_snp_variants", self.ctx, (self._h, ptr(u), len(ref_lengths), ptr(ref_lengths)),
                             int(ref_lengths.sum()), ref_code, evolution, error, threshold)

    def plan_check(self):
        """Tasks whose device-made band rows / schedules / stripe tables differ from the host planner's (test aid;
        include/nprealign.h: npr_batch_plan_check)."""
        return int(check(self._L.npr_batch_plan_check(self._h, ptr(self._keep[4])), "npr_batch_plan_check", self.ctx))

    def align_stats(self):
        """Per-read reductions over the aligned pairs of the cigars finish() produced, computed where they lie
        (include/nprealign.h: npr_batch_align_stats): int32 array [n_reads, STATS_WORDS]."""
        out = np.zeros((self.n_reads, _lib.STATS_WORDS), dtype=np.int32)
        check(self._L.npr_batch_align_stats(self._h, ptr(out)), "npr_batch_align_stats", self.ctx)
        return out

    def indel_kmers(self, k=5):
        """The k-mers that straddle a gap of the cigars finish() produced, counted where they lie (include/nprealign.h:
        npr_batch_indel_kmers): (read-side table, reference-side table), int64 [4^k + 1] each."""
        nb = 4 ** k + 1 if 1 <= k <= _lib.KMER_MAX_K else 1
        rd, rf = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
        check(self._L.npr_batch_indel_kmers(self._h, int(k), ptr(rd), ptr(rf)), "npr_batch_indel_kmers", self.ctx)
        return rd, rf

    def expectations(self):
        """Baum-Welch E-step with the installed models: (T_exp[slots,25], E_exp[slots,80], loglik[slots], kernel ms)."""
        T = np.zeros((_lib.MAX_MODELS, 25))
        E = np.zeros((_lib.MAX_MODELS, 80))
        ll = np.zeros(_lib.MAX_MODELS)
        ms = C.c_float(0)
        check(self._L.npr_batch_expectations(self._h, ptr(T), ptr(E), ptr(ll), C.byref(ms)), "npr_batch_expectations", self.ctx)
        return T, E, ll, ms.value

    def dense(self, read_index, cells):
        fv = np.zeros(cells, dtype=np.float32)
        fe = np.zeros(cells, dtype=np.int32)
        bv = np.zeros(cells, dtype=np.float32)
        be = np.zeros(cells, dtype=np.int32)
        check(self._L.npr_batch_dense(self._h, read_index, ptr(fv), ptr(fe), ptr(bv), ptr(be), cells), "npr_batch_dense", self.ctx)
        return fv, fe, bv, be

    def rs_forward(self, read_index, cells):
        """include/nprealign.h: npr_batch_rs_forward -- the forward match rows k_dp_rs stores, (value, row exponent) in band order."""
        fv = np.zeros(cells, dtype=np.float32)
        fe = np.zeros(cells, dtype=np.int32)
        check(self._L.npr_batch_rs_forward(self._h, read_index, ptr(fv), ptr(fe), cells), "npr_batch_rs_forward", self.ctx)
        return fv, fe


class Pileup(_Handle):
    """A per-position table on the device (include/nprealign.h: npr_pileup_*; csrc/npr_pileup.hip): PILEUP_WORDS int32 counters per
    position of the reference sequences whose lengths it was made with, rows in their order.  It accumulates over add_batch() / add()
    calls -- a file realigned in several chunks is one table -- and may be read in between."""
    _destroy = "npr_pileup_destroy"

    def __init__(self, ctx, ref_lengths):
        self.ref_lengths = _arr(ref_lengths, np.int64).reshape(-1)
        self.rows = int(self.ref_lengths.sum())
        self._create(ctx, "npr_pileup_create", "npr_pileup_create", len(self.ref_lengths), ptr(self.ref_lengths))

    def add_batch(self, batch, use=None):
        """The alignments batch.finish() just produced, where they lie; use[i] != 0 selects read i (None: all); reads that failed add
        nothing."""
        u = _arr(use, np.uint8)
        if u is not None and len(u) != batch.n_reads:
            raise ValueError("use must have one entry per read of the batch")
        check(self._L.npr_pileup_add_batch(self._h, batch._h, ptr(u)), "npr_pileup_add_batch", self.ctx)

    def add(self, reads, cigars, ref_index, start=None, use=None):
        """Any alignments: reads = ASCII sequences, cigars = [(op, len)] lists with ops M/I/D (0/1/2), ref_index[i] = the reference
        sequence of record i, start[i] = (first reference position, first read position) of cigar i (None: 0, 0)."""
        read, read_off = _csr(reads)
        ops, ops_off = _csr_ops(cigars)
        self.add_csr(read, read_off, None, ops, ops_off, ref_index, start, use)

    def add_csr(self, read, read_begin, read_end, ops, ops_off, ref_index, start=None, use=None):
        """add() on arrays: read i = read[read_begin[i] : read_end[i]] (read_end None: read_begin has n + 1 entries, the reads lie back
        to back), cigar i = ops[ops_off[i] : ops_off[i + 1]] (rows of (op, len))."""
        read, read_begin, read_end = _arr(read, np.uint8), _arr(read_begin, np.int64), _arr(read_end, np.int64)
        ops, ops_off = _arr(ops, np.int32, 2), _arr(ops_off, np.int64)
        n = len(ops_off) - 1
        ri, st, u = _arr(ref_index, np.int32), _arr(start, np.int64, 2), _arr(use, np.uint8)
        if len(ri) != n or len(read_begin) != (n + 1 if read_end is None else n) or (read_end is not None and len(read_end) != n) or \
                (st is not None and len(st) != n) or (u is not None and len(u) != n):
            raise ValueError("one reference index, read, start and use entry per cigar")
        check(self._L.npr_pileup_add(self._h, n, ptr(ri), ptr(read), ptr(read_begin), ptr(read_end), ptr(ops), ptr(ops_off), ptr(st), ptr(u)),
              "npr_pileup_add", self.ctx)

    def add_bam(self, stream, flag_mask=0x4 | 0x100 | 0x200 | 0x400):
        """The records of a BamStream (Context.bam_open) where they lie on the device (include/nprealign.h: npr_pileup_add_bam, which states
        what is selected, which cigar applies and what is refused): no SAM text, nothing parsed on the host.  flag_mask: records with one of
        these FLAG bits are left out (default: samtools' pileup mask, analyses/pileup.py FLAG_MASK).  -> {"records", "selected", "added",
        "refused"}, kept in self.last_bam_counts too.  A refused record adds nothing and raises NprError (ERR_INVALID) as add_csr does, after
        the other records were counted; a file whose reference sequences are not the pileup's raises too, and nothing is added."""
        out = np.zeros(4, dtype=np.int64)
        rc = self._L.npr_pileup_add_bam(self._h, stream._h, int(flag_mask), ptr(out))
        self.last_bam_counts = dict(zip(("records", "selected", "added", "refused"), (int(v) for v in out)))
        check(rc, "npr_pileup_add_bam", self.ctx)
        return self.last_bam_counts

    def counts(self):
        """The table so far: int32 [rows, PILEUP_WORDS]."""
        out = np.zeros((self.rows, _lib.PILEUP_WORDS), dtype=np.int32)
        check(self._L.npr_pileup_counts(self._h, ptr(out)), "npr_pileup_counts", self.ctx)
        return out

    def snp_calls(self, ref_code, true_code, evolution, errors):
        """SNP calls from the aligned-base frequencies of the table so far (words 0-3; a row is seen when words 0-4 are not all zero), made
        on the device (include/nprealign.h: npr_pileup_snp_calls; _snp_calls for the matrices and what comes back)."""
        return _snp_calls(self._L.npr_pileup_snp_calls, "npr_pileup_snp_calls", self.ctx, (self._h,), self.rows, ref_code, true_code, evolution, errors)

    def snp_variants(self, ref_code, evolution, error, threshold):
        """The SNP calls themselves and a best base with its quality per position, from the aligned-base frequencies of the table so far
        (include/nprealign.h: npr_pileup_snp_variants; _snp_variants for what comes back)."""
        return _snp_variants(self._L.npr_pileup_snp_variants, "npr_pileup_snp_variants", self.ctx, (self._h,), self.rows, ref_code, evolution, error, threshold)

    def depth(self):
        """(depth int32 [rows], covered bool [rows]): what `samtools depth` prints (M columns) and which positions it prints a line for
        (M or deletion columns), summed on the device."""
        depth = np.zeros(self.rows, dtype=np.int32)
        covered = np.zeros(self.rows, dtype=np.uint8)
        check(self._L.npr_pileup_depth(self._h, ptr(depth), ptr(covered)), "npr_pileup_depth", self.ctx)
        return depth, covered.astype(bool)

    def coverage(self, ref_text, ref_off, n_windows=400, out=None):
        """The table so far reduced on the device to windows of the concatenated reference, a depth histogram, the histogram of record
        starts per position and totals (include/nprealign.h: npr_pileup_coverage, which defines every word).  ref_text / ref_off: the ASCII
        reference sequences in the pileup's order, sequence k = ref_text[ref_off[k]:ref_off[k + 1]] (FastaTable.seq / .off when the file
        holds them in that order).  -> Coverage; `out`: a Coverage to fill."""
        ref_text, ref_off = _arr(ref_text, np.uint8), _arr(ref_off, np.int64)
        if len(ref_off) != len(self.ref_lengths) + 1 or (len(ref_off) and (int(ref_off[0]) < 0 or int(ref_off[-1]) > len(ref_text))):
            raise NprError(_lib.ERR_INVALID, "npr_pileup_coverage", "one offset per sequence and the end, inside the reference text")
        if out is None:
            out = Coverage.zeros(n_windows if 1 <= n_windows <= _lib.AQ_MAX_WINDOWS else 1)
        check(self._L.npr_pileup_coverage(self._h, ptr(ref_text), ptr(ref_off), int(n_windows), *map(ptr, out.arrays())), "npr_pileup_coverage", self.ctx)
        return out


def parse_region(references, lengths, region):
    """A region of a file with these reference names and lengths -> (tid, beg, end), 0-based and half-open.  `region`: (name or tid, beg,
    end), 0-based and half-open as it stands, or a samtools string: "name" is the whole sequence, "name:a-b" positions a to b, 1-based and
    inclusive ("name:a": from a to the sequence's end; commas in the numbers are skipped).  A string that is wholly a reference name wins
    over splitting it at its last colon."""
    def tid_of(name):
        if isinstance(name, (int, np.integer)):
            if not 0 <= int(name) < len(references):
                raise ValueError("region %r: the file has %d reference sequences" % (region, len(references)))
            return int(name)
        if name not in references:
            raise KeyError("region %r: no reference sequence %r" % (region, name))
        return list(references).index(name)
    if not isinstance(region, str):
        name, beg, end = region
        return tid_of(name), int(beg), int(end)
    if region in references or ":" not in region:
        tid = tid_of(region)
        return tid, 0, int(lengths[tid])
    name, _, span = region.rpartition(":")
    tid = tid_of(name)
    a, dash, b = span.replace(",", "").partition("-")
    try:
        return tid, int(a) - 1, int(b) if dash else int(lengths[tid])
    except ValueError:
        raise ValueError("region %r: not name, name:a or name:a-b" % (region,))


class BamStream(_Handle):
    """A BAM file image inflated and walked on the device (include/nprealign.h: npr_bam_open): the uncompressed stream and the table of its
    records' offsets stay there until close(); .references / .lengths are the header's names and l_ref values, .n_records the records,
    .l_text the header text's length, .stream_bytes the stream's.  `data`: bytes or a uint8 array.  A file that is not BGZF, a block that
    does not inflate, a bad BAM magic or a malformed record raises, and there is no object.  Pileup.add_bam takes it; it may be added any
    number of times, to any pileup of its context.  A context manager: closed on exit."""
    _destroy = "npr_bam_close"

    def __init__(self, ctx, data, index=None, region=None):
        """index, region: Context.bam_open."""
        data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
        if index is not None and region is None:
            raise ValueError("an index serves a region: give one, or leave the index out")
        if index is not None:
            from . import bam
            index = np.frombuffer(bytes(index), dtype=np.uint8) if isinstance(index, (bytes, bytearray)) else _arr(index, np.uint8)
            tid, beg, end = parse_region(*bam.bam_references(data), region)
            self._create(ctx, "npr_bam_open_region", "npr_bam_open_region", ptr(data), len(data), ptr(index), len(index), tid, beg, end)
        else:
            self._create(ctx, "npr_bam_open", "npr_bam_open", ptr(data), len(data))
        info = np.zeros(4, dtype=np.int64)
        check(self._L.npr_bam_stream_info(self._h, ptr(info)), "npr_bam_stream_info", ctx)
        self.n_records, n_ref, self.l_text, self.stream_bytes = (int(v) for v in info)
        total = int(check(self._L.npr_bam_stream_refs(self._h, None, None, None, 0), "npr_bam_stream_refs", ctx))
        self.lengths, name_off, names = np.zeros(n_ref, dtype=np.int64), np.zeros(n_ref + 1, dtype=np.int64), np.zeros(max(total, 1), dtype=np.uint8)
        check(self._L.npr_bam_stream_refs(self._h, ptr(self.lengths), ptr(name_off), ptr(names), len(names)), "npr_bam_stream_refs", ctx)
        text = names.tobytes()
        self.references = [text[name_off[k]:name_off[k + 1]].decode() for k in range(n_ref)]
        self._image, self._header_text = data, None   # (the file image is kept until header_text() has read the header from it, or close())
        if region is not None and index is None:
            try:
                self.restrict(region)
            except Exception:
                self.close()
                raise

    def restrict(self, region):
        """Narrows the object to the records that overlap `region` (Context.bam_open says how one is written; include/nprealign.h:
        npr_bam_stream_restrict, which states when a record overlaps), order preserved, on the device: no index, a file in any order.
        Restricting twice gives the intersection.  -> the number of records left, .n_records too."""
        tid, beg, end = parse_region(self.references, self.lengths, region)
        self.n_records = int(check(self._L.npr_bam_stream_restrict(self._h, tid, beg, end), "npr_bam_stream_restrict", self.ctx))
        return self.n_records

    def sam_text(self):
        """The header text and one line per record of the object, the lines Context.bam_to_sam writes (include/nprealign.h:
        npr_bam_stream_sam): a uint8 array.  After a region query: `samtools view -h x.bam region`."""
        out = np.empty(6 * self.stream_bytes + 64, dtype=np.uint8)   # a bound instead of a sizing call, as bam.bam_sam's
        n = C.c_int64(0)
        total = int(check(self._L.npr_bam_stream_sam(self._h, ptr(out), len(out), C.byref(n)), "npr_bam_stream_sam", self.ctx))
        return out[:total]

    def header_text(self):
        """The header text alone (the first l_text bytes of sam_text()), read on the host from the file image the first time it is
        asked for (bam.bam_head)."""
        if self._header_text is None:
            from . import bam
            self._header_text, self._image = bam.bam_head(self._image)[0], None
        return self._header_text

    def close(self):
        self._image = None
        _Handle.close(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


class SeedIndex(_Handle):
    """The exact-match seed index of a set of reference sequences on the device (include/nprealign.h: npr_seed_*; csrc/npr_seed.hip):
    built once, asked for the maximal exact matches of any number of reads."""
    _destroy = "npr_seed_index_destroy"

    def __init__(self, ctx, ref, ref_off, k=16):
        self.k = int(k)
        ref, ref_off = _arr(ref, np.uint8), _arr(ref_off, np.int64)
        self.n_refs = len(ref_off) - 1
        self._create(ctx, "npr_seed_index_create", "npr_seed_index_create", self.k, self.n_refs, ptr(ref), ptr(ref_off))

    @staticmethod
    def _chunks(where, text, begin, end, chunk_bases):
        """The reads as the library takes them, and how they go to the device: (text, begin, end, [(lo, hi), ...]) with reads lo .. hi of a
        chunk staying within chunk_bases bases (one read at least); one empty chunk when there are no reads."""
        text, begin, end = _arr(text, np.uint8), _arr(begin, np.int64), _arr(end, np.int64)
        n = len(begin)
        if len(end) != n or (n and (int(begin.min()) < 0 or int(end.max()) > len(text))):
            raise NprError(_lib.ERR_INVALID, where, "begin and end differ in number, or a span lies outside the text")
        first = np.zeros(n + 1, dtype=np.int64)  # bases before read i
        np.cumsum(end - begin, out=first[1:])
        chunks = []
        while not chunks or chunks[-1][1] < n:
            lo = chunks[-1][1] if chunks else 0
            chunks.append((lo, min(n, max(int(np.searchsorted(first, first[lo] + chunk_bases, side="right")) - 1, lo + 1))))
        return text, begin, end, chunks

    def map(self, text, begin, end, min_len=20, strands=3, max_gap=200, chunk_bases=1 << 26, rows=False):
        """matches() followed by Context.seed_chains() on its rows, in one call per chunk of reads and with the rows never leaving the
        device (include/nprealign.h: npr_seed_map_*; csrc/npr_seedmap.hip): (chain_off, chains, ops_off, ops) as seed_chains returns them
        for read lengths end - begin and the index's own sequence lengths, and with rows=True (hit_off, hits, chain_off, chains, ops_off,
        ops), the first two as matches returns them.  Chunks as matches cuts them; their arrays are joined with the offsets rebased."""
        text, begin, end, chunks = self._chunks("npr_seed_map_create", text, begin, end, chunk_bases)
        n = len(begin)
        hit_off, chain_off = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        hits, chains, ops_off, ops = [], [], [np.zeros(1, dtype=np.int64)], []
        n_ops = 0
        for lo, hi in chunks:
            m = SeedMap(self, text, begin[lo:hi], end[lo:hi], min_len, strands, max_gap)
            try:
                part = m.fetch(rows)
            finally:
                m.close()
            if rows:
                hit_off[lo + 1:hi + 1] = hit_off[lo] + part[0][1:]
                hits.append(part[1])
            chain_off[lo + 1:hi + 1] = chain_off[lo] + part[-4][1:]
            chains.append(part[-3])
            ops_off.append(n_ops + part[-2][1:])
            ops.append(part[-1])
            n_ops += len(part[-1])
        out = (chain_off, np.concatenate(chains), np.concatenate(ops_off), np.concatenate(ops))
        return (hit_off, np.concatenate(hits)) + out if rows else out

    def matches(self, text, begin, end, min_len=20, strands=3, chunk_bases=1 << 26):
        """All maximal exact matches of at least min_len bases of the reads text[begin[i]:end[i]] (spans inside a larger uint8 text, e.g.
        FastqTable.text / .seq_span) on the strands asked for (1 forward, 2 reverse, 3 both): (hit_off int64 [n + 1], hits int32 [m, 4]) --
        the rows of read i are hits[hit_off[i]:hit_off[i + 1]], each (reference index, a, b | strand << 31, L), sorted by (strand,
        reference index, a, b).  The reads go to the device in chunks of about chunk_bases bases, each counted first and then fetched
        into a buffer of exactly its size."""
        text, begin, end, chunks = self._chunks("npr_seed_matches", text, begin, end, chunk_bases)
        hit_off = np.zeros(len(begin) + 1, dtype=np.int64)
        parts = []
        for lo, hi in chunks:
            off = np.zeros(hi - lo + 1, dtype=np.int64)
            args = [self._h, int(min_len), int(strands), hi - lo, ptr(text), ptr(begin[lo:hi]), ptr(end[lo:hi]), ptr(off)]
            total = self._L.npr_seed_matches(*args, None, 0)
            if total == ERR_CAPACITY:  # (there are matches: the offsets say how many)
                rows = np.empty((int(off[-1]), 4), dtype=np.int32)
                total = check(self._L.npr_seed_matches(*args, ptr(rows), len(rows)), "npr_seed_matches", self.ctx)
                parts.append(rows)
            check(total, "npr_seed_matches", self.ctx)
            hit_off[lo + 1:hi + 1] = hit_off[lo] + off[1:]
        return hit_off, (np.concatenate(parts) if parts else np.zeros((0, 4), dtype=np.int32))


class SeedMap(_Handle):
    """The rows, chains and guides of one call's reads on the device (include/nprealign.h: npr_seed_map_*): made by one call on a
    SeedIndex, fetched as often as wanted, destroyed like every other object of its context (it does not need its index any more)."""
    _destroy = "npr_seed_map_destroy"

    def __init__(self, index, text, begin, end, min_len=20, strands=3, max_gap=200):
        begin, end = _arr(begin, np.int64), _arr(end, np.int64)
        self.n_reads = len(begin)
        self._create(index.ctx, "npr_seed_map_create", "npr_seed_map_create", int(min_len), int(strands), int(max_gap), self.n_reads,
                     ptr(_arr(text, np.uint8)), ptr(begin), ptr(end), made_from=index)

    def counts(self):
        """(rows, chains, guide op pairs)"""
        c = np.zeros(3, dtype=np.int64)
        check(self._L.npr_seed_map_counts(self._h, ptr(c)), "npr_seed_map_counts", self.ctx)
        return tuple(int(v) for v in c)

    def fetch(self, rows=True):
        """(hit_off, hits, chain_off, chains, ops_off, ops), the first two only with rows=True."""
        n_rows, n_chains, n_pairs = self.counts()
        hit_off, hits = (np.zeros(self.n_reads + 1, dtype=np.int64), np.empty((n_rows, 4), dtype=np.int32)) if rows else (None, None)
        chain_off, chains = np.zeros(self.n_reads + 1, dtype=np.int64), np.empty((n_chains, 4), dtype=np.int32)
        ops_off, ops = np.zeros(n_chains + 1, dtype=np.int64), np.empty((n_pairs, 2), dtype=np.int32)
        out = (hit_off, hits, chain_off, chains, ops_off, ops)
        check(self._L.npr_seed_map_fetch(self._h, *map(ptr, out)), "npr_seed_map_fetch", self.ctx)
        return out if rows else out[2:]


class Context(object):
    """One realigner context = one GPU + one HIP stream.  Raises if no gfx950 device is usable."""

    def __init__(self, device=0):
        self._L = _lib.load()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        rc = self._L.npr_create(device, C.byref(h), err, 512)
        if rc != _lib.OK:
            raise NprError(rc, "npr_create", err.value.decode(errors="replace"))
        self._h = h
        self.device = device
        self._models = {}  # slot -> (T, E) or None, as installed: what another context on the same GPU copies
        self._open = weakref.WeakSet()  # the batches staged and the pileups made on this context and not closed yet: close() closes them first

    def set_option(self, option, value):
        """include/nprealign.h: npr_ctx_option (e.g. _lib.OPT_OVERLAP for a context of a pipelined job)."""
        check(self._L.npr_ctx_option(self._h, option, int(value)), "npr_ctx_option", self)

    def release_scratch(self):
        """NPR_OPT_RELEASE_SCRATCH: the device's forward scratch and this context's cached buffers go back to the driver."""
        self.set_option(_lib.OPT_RELEASE_SCRATCH, 1)

    @contextlib.contextmanager
    def options(self, **kw):
        """The test / bring-up switches of include/nprealign.h by name (_lib.OPTIONS), set for the body and back to 0 after it:
        `with ctx.options(arith=_lib.ARITH_CELL): ...`.  None changes a result."""
        for k, v in kw.items():
            self.set_option(_lib.OPTIONS[k], v)
        try:
            yield self
        finally:
            for k in kw:
                self.set_option(_lib.OPTIONS[k], 0)

    def copy_models_from(self, other):
        """Installs the models `other` holds (a second context of a pipelined job runs the same ones)."""
        for slot, m in other._models.items():
            self._set(slot, m)

    def _set(self, slot, m):
        T, E = (None, None) if m is None else m
        check(self._L.npr_set_hmm(self._h, slot, ptr(T), ptr(E)), "npr_set_hmm", self)
        self._models[slot] = m

    def last_error(self):
        return self._L.npr_last_error(self._h).decode(errors="replace")

    def set_hmm(self, hmm=None, slot=0):
        """hmm: object with .transitions (25) and .emissions (80) (nanopore_amd.hmm.Hmm), or None for
        the stock model used when the reference passes no --loadHmm."""
        if hmm is None:
            return self._set(slot, None)
        T, E = _arr(hmm.transitions, np.float64), _arr(hmm.emissions, np.float64)
        if T.size != 25 or E.size != 80:
            raise ValueError("HMM must have 25 transitions and 80 emissions")
        self._set(slot, (T, E))

    def stage(self, params, refs, reads, guides, model_slot=None, ref_index=None, guide_start=None):
        """refs/reads: lists of ASCII sequences (str/bytes); guides: list of [(op,len),...].
        ref_index[i] = which entry of `refs` read i aligns to (None: read i <-> refs[i]).
        guide_start[i] = (first reference position, first read position) of guide i -- the coordinates of the
        exonerate cigar line cactus_realign reads; None: every guide is global over both sequences."""
        return Batch(self, params, *_csr(refs), *_csr(reads), *_csr_ops(guides), model_slot, ref_index, guide_start)

    def stage_csr(self, params, ref, ref_off, read, read_off, guide_ops, guide_off, model_slot=None,
                  ref_index=None, guide_start=None):
        return Batch(self, params, _arr(ref, np.uint8), _arr(ref_off, np.int64), _arr(read, np.uint8), _arr(read_off, np.int64),
                     _arr(guide_ops, np.int32, 2), _arr(guide_off, np.int64), model_slot, ref_index, guide_start)

    def stage_spans(self, params, ref, ref_off, text, read_begin, read_end, guide_ops, guide_off, model_slot=None,
                    ref_index=None, guide_start=None):
        """Stages reads that lie scattered in `text` (uint8): read i = text[read_begin[i] : read_end[i]]
        (include/nprealign.h: npr_batch_create_spans).  guide_off may be a slice of a longer CSR: its values index guide_ops."""
        return Batch(self, params, ref, _arr(ref_off, np.int64), text, _arr(read_begin, np.int64), _arr(guide_ops, np.int32, 2),
                     _arr(guide_off, np.int64), model_slot, ref_index, guide_start, read_end=_arr(read_end, np.int64))

    def align_stats(self, refs, reads, cigars, ref_index=None, start=None):
        """Per-read reductions over the aligned pairs of arbitrary alignments (a mapper's SAM records) on the device
        (include/nprealign.h: npr_align_stats).  refs / reads: ASCII sequences; cigars: [(op, len)] lists with ops M/I/D
        (0/1/2); start[i] = (first reference position, first read position) of cigar i.  int32 [n, STATS_WORDS]."""
        n, n_refs, arrays = _host_alignments(refs, reads, cigars, ref_index, start)
        out = np.zeros((n, _lib.STATS_WORDS), dtype=np.int32)
        check(self._L.npr_align_stats(self._h, n, n_refs, *map(ptr, arrays), ptr(out)), "npr_align_stats", self)
        return out

    def kmer_counts(self, seqs, k=5):
        """All windows s[i - k : i], i in k .. len(s) - 1, of the ASCII sequences `seqs`, forward strand, counted on the device
        (include/nprealign.h: npr_kmer_counts): int64 [4^k + 1]; bin = base-4 number of the k-mer (A C G T = 0..3, first base
        most significant), the last bin for k-mers with a base outside ACGT."""
        seq, off = _csr(seqs)
        out = np.zeros(4 ** k + 1 if 1 <= k <= _lib.KMER_MAX_K else 1, dtype=np.int64)
        check(self._L.npr_kmer_counts(self._h, int(k), len(off) - 1, ptr(seq), ptr(off), ptr(out)), "npr_kmer_counts", self)
        return out

    def kmer_counts_groups(self, text, begin, end, group, n_groups, k=5):
        """kmer_counts into one table per group in one pass (include/nprealign.h: npr_kmer_counts_groups): sequence i is
        text[begin[i]:end[i]] -- spans inside a larger uint8 text, e.g. FastqTable.text / .seq_span --, group[i] in 0 .. n_groups - 1 picks
        its table and -1 leaves it out: int64 [n_groups, 4^k + 1]."""
        text, begin, end, group = _arr(text, np.uint8), _arr(begin, np.int64), _arr(end, np.int64), _arr(group, np.int32)
        if not (len(begin) == len(end) == len(group)) or (len(begin) and (int(begin.min()) < 0 or int(end.max()) > len(text))):
            raise NprError(_lib.ERR_INVALID, "npr_kmer_counts_groups", "spans and groups differ in number, or a span lies outside the text")
        ok = 1 <= k <= _lib.KMER_MAX_K and 1 <= n_groups <= _lib.KMER_MAX_GROUPS
        out = np.zeros((n_groups, 4 ** k + 1) if ok else (1, 1), dtype=np.int64)
        check(self._L.npr_kmer_counts_groups(self._h, int(k), len(begin), ptr(text), ptr(begin), ptr(end), ptr(group), int(n_groups), ptr(out)),
              "npr_kmer_counts_groups", self)
        return out

    def read_quality(self, text, seq_span, qual_span, group, n_groups):
        """The read-quality tables of the FastQC analysis, counted on the device in one pass (include/nprealign.h: npr_read_quality, which
        defines every table): read i has the bases text[seq_span[i, 0]:seq_span[i, 1]] and the quality bytes
        text[qual_span[i, 0]:qual_span[i, 1]] -- FastqTable.text / .seq_span / .qual_span as they are --, group[i] in 0 .. n_groups - 1
        picks its tables and -1 leaves it out.  -> ReadQuality."""
        text, group = _arr(text, np.uint8), _arr(group, np.int32)
        seq_span, qual_span = _arr(seq_span, np.int64).reshape(-1, 2), _arr(qual_span, np.int64).reshape(-1, 2)
        n = len(group)
        if not (len(seq_span) == len(qual_span) == n) or (n and (min(int(seq_span.min()), int(qual_span.min())) < 0 or
                                                                 max(int(seq_span.max()), int(qual_span.max())) > len(text))):
            raise NprError(_lib.ERR_INVALID, "npr_read_quality", "spans and groups differ in number, or a span lies outside the text")
        out = ReadQuality.zeros(n_groups if 1 <= n_groups <= _lib.RQ_MAX_GROUPS else 1)
        cols = [np.ascontiguousarray(a) for a in (seq_span[:, 0], seq_span[:, 1], qual_span[:, 0], qual_span[:, 1])]
        check(self._L.npr_read_quality(self._h, n, ptr(text), *map(ptr, cols), ptr(group), int(n_groups), *map(ptr, out.arrays())), "npr_read_quality", self)
        return out

    def align_quality(self, read, read_begin, read_end, ops, ops_off, ref_index, mapq, clip, ref_text, ref_off, start=None, use=None, n_windows=400,
                      out=None, allow_invalid=False):
        """The per-record alignment-quality tables of the QualiMap analysis, counted on the device in one pass over the records
        (include/nprealign.h: npr_align_quality, which defines every table).  The records as Pileup.add_csr takes them; mapq[i] = MAPQ of
        record i, clip[i] = (soft-clipped bases before, after read[read_begin[i]:read_end[i]]); ref_text / ref_off = the ASCII reference
        sequences ref_index points into.  A record that is malformed or runs past its sequences is left out and raises NprError, unless
        allow_invalid: then the tables of the other records come back with .invalid set.  -> AlignQuality; `out`: an AlignQuality to fill."""
        read, read_begin, read_end = _arr(read, np.uint8), _arr(read_begin, np.int64), _arr(read_end, np.int64)
        ops, ops_off = _arr(ops, np.int32, 2), _arr(ops_off, np.int64)
        n = len(ops_off) - 1
        ri, st, u = _arr(ref_index, np.int32), _arr(start, np.int64, 2), _arr(use, np.uint8)
        mq, cl = _arr(mapq, np.int32), _arr(clip, np.int64, 2)
        ref_text, ref_off = _arr(ref_text, np.uint8), _arr(ref_off, np.int64)
        if n < 0 or len(ri) != n or len(read_begin) != (n + 1 if read_end is None else n) or (read_end is not None and len(read_end) != n) or \
                (st is not None and len(st) != n) or (u is not None and len(u) != n) or len(mq) != n or len(cl) != n:
            raise ValueError("one reference index, read, start, use, mapq and clip entry per cigar")
        if len(ref_off) < 1 or int(ref_off[0]) < 0 or int(ref_off[-1]) > len(ref_text):
            raise NprError(_lib.ERR_INVALID, "npr_align_quality", "the reference offsets lie outside the reference text")
        if out is None:
            out = AlignQuality.zeros(n_windows if 1 <= n_windows <= _lib.AQ_MAX_WINDOWS else 1)
        rc = self._L.npr_align_quality(self._h, n, ptr(ri), ptr(read), ptr(read_begin), ptr(read_end), ptr(ops), ptr(ops_off), ptr(st), ptr(u), ptr(mq),
                                       ptr(cl), len(ref_off) - 1, ptr(ref_text), ptr(ref_off), int(n_windows), *map(ptr, out.arrays()))
        out.invalid = rc == _lib.ERR_INVALID
        if not (allow_invalid and out.invalid):
            check(rc, "npr_align_quality", self)
        return out

    def sam_to_bam(self, samFile, bamFile, sort=True, index=True, compress=False):
        """samFile as a BAM file made on the device (include/nprealign.h: npr_sam_bam; nanopore_amd/bam.py): coordinate-sorted, with
        bamFile + ".bai" beside it when index is set, or in the file's order without an index (sort=False).  BGZF with stored blocks (the
        file is about the size of the uncompressed stream), or with compress=True with blocks compressed on the device
        (npr_sam_bam_deflate).  -> the counts (records, references, bytes, no_coordinate, mapped, unmapped; with compress stream_bytes)."""
        from . import bam
        return bam.sam_to_bam(self, samFile, bamFile, sort=sort, index=index, compress=compress)

    def bam_to_sam(self, bamFile, samFile):
        """bamFile as SAM text in samFile, inflated, walked and written on the device (include/nprealign.h: npr_bam_sam; nanopore_amd/bam.py).
        -> the counts (records, references, bytes, stream_bytes, blocks).  A malformed file raises and leaves no file."""
        from . import bam
        return bam.bam_to_sam(self, bamFile, samFile)

    def bam_open(self, data, index=None, region=None):
        """A BAM file image (bytes or a uint8 array) inflated and walked on the device, kept there (BamStream; include/nprealign.h:
        npr_bam_open): what Pileup.add_bam takes.  region: only the records that overlap it -- (name or tid, beg, end), 0-based and
        half-open, or a samtools string ("name", "name:a-b" 1-based and inclusive; parse_region).  With `index` (the bytes of the file's
        .bai) only the blocks the index names for the region are inflated and walked (npr_bam_open_region: the file must be the sorted one
        the index was made of); without it the file is opened whole and restricted (BamStream.restrict)."""
        return BamStream(self, data, index=index, region=region)

    def bam_merge(self, streams, sort=True, index=True, compress=False):
        """The records of BamStreams of this context -- as they stand, after any region query or restrict -- as one BAM file image made on
        the device without SAM text (include/nprealign.h: npr_bam_streams_bam; csrc/npr_bammerge.hip): coordinate-sorted (stable: ties keep
        the order of `streams`, then the file's) or, with sort=False, one stream after the other (`samtools cat`).  Every record's bytes pass
        as they stand but for its bin, which is measured.  The header is stream 0's text through bam.bam_header(text, sort=sort); all
        streams must have stream 0's reference sequences.  compress: the BGZF blocks are compressed on the device.
        -> (the image as a uint8 array, the BAI file's bytes (bam.bai_write) or None without sort and index)."""
        from . import bam
        streams = list(streams)
        if not streams:
            raise _lib.NprError(_lib.ERR_INVALID, "npr_bam_streams_bam", "no stream")
        first = streams[0]
        header, ref_len = bam.bam_header(first.header_text(), sort=sort)
        n, n_refs = sum(s.n_records for s in streams), len(ref_len)
        want_index = bool(sort and index)
        handles = (C.c_void_p * len(streams))(*[s._h for s in streams])
        run_tid, run_bin = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32)
        run_beg, run_end = np.zeros(max(n, 1), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint64)
        linear, meta = np.zeros(max(int(bam.linear_windows(ref_len)[-1]), 1), dtype=np.uint64), np.zeros((max(n_refs, 1), 4), dtype=np.uint64)
        n_runs, n_no_coor, n_records = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        # a bound instead of a sizing call (pages nobody touches cost nothing): the records are bytes of the streams
        stream = len(header) + sum(s.stream_bytes for s in streams)
        room = stream + 31 * (stream // _lib.BGZF_PAYLOAD + 1) + 28
        out = np.empty(room, dtype=np.uint8)
        total = int(check(self._L.npr_bam_streams_bam(self._h, handles, len(streams), ptr(header), len(header), int(bool(sort)), int(bool(compress)), ptr(out),
                                                      room, C.byref(n_records), C.byref(n_runs), ptr(run_tid), ptr(run_bin),
                                                      ptr(run_beg), ptr(run_end), ptr(linear), ptr(meta), C.byref(n_no_coor)), "npr_bam_streams_bam", self))
        r = n_runs.value
        bai = bam.bai_write(ref_len, run_tid[:r], run_bin[:r], run_beg[:r], run_end[:r], linear, meta[:n_refs], n_no_coor.value) if want_index else None
        return out[:total], bai

    def bam_merge_last(self):
        """Of the last image bam_merge wrote (npr_bam_merge_last): {"records", "stream_bytes", "gather_bytes": what the gather kernel moved,
        "gather_ns": its time between two events}."""
        out = np.zeros(4, dtype=np.int64)
        check(self._L.npr_bam_merge_last(self._h, ptr(out)), "npr_bam_merge_last", self)
        return dict(zip(("records", "stream_bytes", "gather_bytes", "gather_ns"), (int(v) for v in out)))

    def bam_index(self, data):
        """The BAI file's bytes for a coordinate-sorted BAM file image of any writer, made on the device from the file as it stands
        (include/nprealign.h: npr_bam_index): `samtools index`.  A file whose records are out of order raises NprError (ERR_INVALID)."""
        from . import bam
        data = np.frombuffer(bytes(data), dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else _arr(data, np.uint8)
        _, lengths = bam.bam_references(data)
        _, stream_off = bam.bgzf_scan(data)
        n_refs, windows = len(lengths), int(bam.linear_windows(np.maximum(lengths, 1))[-1])
        room = int(stream_off[-1]) // 36 + 1   # a record has 36 bytes and more; pages nobody touches cost nothing
        ref_len, meta, linear = np.zeros(max(n_refs, 1), dtype=np.int64), np.zeros((max(n_refs, 1), 4), dtype=np.uint64), np.zeros(max(windows, 1), dtype=np.uint64)
        run_tid, run_bin, run_beg, run_end = np.empty(room, dtype=np.int32), np.empty(room, dtype=np.uint32), np.empty(room, dtype=np.uint64), np.empty(room, dtype=np.uint64)
        got_refs, n_runs, n_no_coor = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        check(self._L.npr_bam_index(self._h, ptr(data), len(data), C.byref(got_refs), ptr(ref_len), n_refs, C.byref(n_runs), ptr(run_tid), ptr(run_bin), ptr(run_beg),
                                    ptr(run_end), room, ptr(linear), windows, ptr(meta), C.byref(n_no_coor)), "npr_bam_index", self)
        r = n_runs.value
        return bam.bai_write(ref_len[:n_refs], run_tid[:r], run_bin[:r], run_beg[:r], run_end[:r], linear, meta[:n_refs], n_no_coor.value)

    def align_indel_kmers(self, refs, reads, cigars, k=5, ref_index=None, start=None):
        """The k-mers that straddle a gap of arbitrary alignments (arguments as for align_stats), counted on the device
        (include/nprealign.h: npr_align_indel_kmers): (read-side table, reference-side table), int64 [4^k + 1] each."""
        n, n_refs, arrays = _host_alignments(refs, reads, cigars, ref_index, start)
        nb = 4 ** k + 1 if 1 <= k <= _lib.KMER_MAX_K else 1
        rd, rf = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
        check(self._L.npr_align_indel_kmers(self._h, int(k), n, n_refs, *map(ptr, arrays), ptr(rd), ptr(rf)), "npr_align_indel_kmers", self)
        return rd, rf

    def pileup(self, ref_lengths):
        """A zeroed per-position table for reference sequences of these lengths (Pileup; include/nprealign.h: npr_pileup_create)."""
        return Pileup(self, ref_lengths)

    def snp_calls_table(self, weights, seen, ref_code, true_code, evolution, errors):
        """SNP calls from any table of four non-negative base weights per row, uploaded and called on the device (include/nprealign.h:
        npr_snp_calls_table; _snp_calls for the matrices and what comes back)."""
        weights, seen = _arr(weights, np.float64, 4), _arr(seen, np.uint8)
        if seen.shape != (len(weights),):
            raise ValueError("one seen flag per table row")
        return _snp_calls(self._L.npr_snp_calls_table, "npr_snp_calls_table", self, (self._h, len(weights), ptr(weights), ptr(seen)), len(weights),
                          ref_code, true_code, evolution, errors)

    def snp_variants_table(self, weights, seen, ref_code, evolution, error, threshold):
        """The SNP calls themselves and a best base with its quality per row of any table of four non-negative base weights, uploaded and
        called on the device (include/nprealign.h: npr_snp_variants_table; _snp_variants for what comes back)."""
        weights, seen = _arr(weights, np.float64, 4), _arr(seen, np.uint8)
        if seen.shape != (len(weights),):
            raise ValueError("one seen flag per table row")
        return _snp_variants(self._L.npr_snp_variants_table, "npr_snp_variants_table", self, (self._h, len(weights), ptr(weights), ptr(seen)),
                             len(weights), ref_code, evolution, error, threshold)

    def seed_index(self, refs, k=16):
        """The exact-match seed index of the ASCII sequences `refs` (SeedIndex; include/nprealign.h: npr_seed_index_create)."""
        return SeedIndex(self, *_csr(refs), k)

    def seed_index_csr(self, ref, ref_off, k=16):
        """seed_index on arrays: sequence i = ref[ref_off[i]:ref_off[i + 1]] (FastaTable.seq / .off fit directly)."""
        return SeedIndex(self, ref, ref_off, k)

    def seed_chains(self, read_len, ref_len, hit_off, hits, max_gap=200):
        """The co-linear chains of the rows SeedIndex.matches returned, one per (read, reference) that has rows, as guide alignments made
        on the device (include/nprealign.h: npr_seed_chains; csrc/npr_seedchain.hip): (chain_off int64 [n + 1], chains int32 [m, 4],
        ops_off int64 [m + 1], ops int32 [p, 2]).  The chains of read i are chains[chain_off[i]:chain_off[i + 1]] in ascending reference
        index, each (reference index, strand, score, rows in the chain); chain c's guide over ref_len x read_len is
        ops[ops_off[c]:ops_off[c + 1]] -- what stage_csr and stage_spans take as guide_off and guide_ops."""
        read_len, ref_len, hit_off, hits = _arr(read_len, np.int64), _arr(ref_len, np.int64), _arr(hit_off, np.int64), _arr(hits, np.int32, 4)
        n = len(read_len)
        if len(hit_off) != n + 1 or int(hit_off[-1]) != len(hits):
            raise NprError(_lib.ERR_INVALID, "npr_seed_chains", "one length per read, hit_off[n + 1], one row per match")
        chain_off = np.zeros(n + 1, dtype=np.int64)
        head = [self._h, int(max_gap), n, ptr(read_len), len(ref_len), ptr(ref_len), ptr(hit_off), ptr(hits), ptr(chain_off)]
        m = self._L.npr_seed_chains(*head, None, 0, None, None, 0)  # (nothing runs on the device: the offsets say how many chains)
        if m == ERR_CAPACITY:
            m = int(chain_off[-1])
            chains, ops_off = np.empty((m, 4), dtype=np.int32), np.zeros(m + 1, dtype=np.int64)
            ops = np.empty((3 * len(hits) + 2 * m, 2), dtype=np.int32)  # a chain of k rows has at most 3 k + 2 pairs
            check(self._L.npr_seed_chains(*head, ptr(chains), m, ptr(ops_off), ptr(ops), len(ops)), "npr_seed_chains", self)
            return chain_off, chains, ops_off, ops[:int(ops_off[-1])].copy()
        check(m, "npr_seed_chains", self)
        return chain_off, np.zeros((0, 4), dtype=np.int32), np.zeros(1, dtype=np.int64), np.zeros((0, 2), dtype=np.int32)

    def _realign_once(self, params, refs, reads, guides, model_slot, want_pairs, ref_index, guide_start=None):
        b = self.stage(params, refs, reads, guides, model_slot, ref_index, guide_start)
        try:
            b.run()
            b.finish()
            res = b.results()
            off, ops = b.ops()
            out = []
            aoff, arith = b.segment_arith()
            stage = b.finish_stage()
            if want_pairs:
                poff, x, y, p = b.pairs()
            for i in range(b.n_reads):
                d = dict(status=int(res["status"][i]), score=float(res["score"][i]), loglik=float(res["loglik"][i]),
                         loglik_bwd=float(res["loglik_bwd"][i]), cells=int(res["cells"][i]),
                         n_segments=int(res["n_segments"][i]), n_pairs=int(res["n_pairs"][i]),
                         ops=[(int(a), int(c)) for a, c in ops[off[i]:off[i + 1]]],
                         seg_arith=[int(v) for v in arith[aoff[i]:aoff[i + 1]]], finish_stage=stage)
                if want_pairs:
                    d["x"] = x[poff[i]:poff[i + 1]].copy()
                    d["y"] = y[poff[i]:poff[i + 1]].copy()
                    d["p"] = p[poff[i]:poff[i + 1]].copy()
                out.append(d)
            return out
        finally:
            b.close()

    def realign(self, params, refs, reads, guides, model_slot=None, want_pairs=False, ref_index=None, guide_start=None):
        """One batched call: returns list of dicts (status, score, loglik, cells, ops[, x, y, p]).

        Reads whose sparse posterior list overflowed its capacity (NPR_ERR_CAPACITY: a diffuse model can put up to
        1/threshold pairs on a base) are re-run with a four times larger `max_pairs_per_base` until they fit."""
        out = self._realign_once(params, refs, reads, guides, model_slot, want_pairs, ref_index, guide_start)
        per_base = params.max_pairs_per_base if params.max_pairs_per_base > 0 else 6
        limit = int(1.0 / max(params.posterior_threshold, 1e-6)) + 1
        while per_base < limit:
            again = [i for i, o in enumerate(out) if o["status"] == _lib.ERR_CAPACITY]
            if not again:
                break
            per_base = min(4 * per_base, limit)
            p2 = Params.from_buffer_copy(params)
            p2.max_pairs_per_base = per_base
            if ref_index is None:
                sub_refs, sub_index = [refs[i] for i in again], None
            else:
                sub_refs, sub_index = refs, [ref_index[i] for i in again]
            sub = self._realign_once(p2, sub_refs, [reads[i] for i in again], [guides[i] for i in again],
                                     None if model_slot is None else [model_slot[i] for i in again], want_pairs, sub_index,
                                     None if guide_start is None else [guide_start[i] for i in again])
            for i, o in zip(again, sub):
                out[i] = o
        return out

    def close(self):
        if getattr(self, "_h", None):
            # a batch or pileup that outlives its context (a test that failed with one open, at interpreter exit) would hand
            # npr_batch_destroy / npr_pileup_destroy an object whose context is gone: the library has no way to know
            for b in list(getattr(self, "_open", ())):
                b.close()
            self._L.npr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- host logic (no GPU needed) ----

@contextlib.contextmanager
def _plan(params, lX, lY, guide):
    """`with _plan(...) as (L, h)`: the library and the npr_plan handle of one read's band plan, destroyed when the body ends."""
    L = _lib.load()
    g = _arr(guide, np.int32, 2)
    h = C.c_void_p()
    check(L.npr_plan_create(C.byref(params), lX, lY, ptr(g), len(g), C.byref(h)), "npr_plan_create")
    try:
        yield L, h
    finally:
        L.npr_plan_destroy(h)


def plan(params, lX, lY, guide):
    out = []
    with _plan(params, lX, lY, guide) as (L, h):
        for s in range(check(L.npr_plan_segments(h), "npr_plan_segments")):
            info = np.zeros(8, dtype=np.int64)
            check(L.npr_plan_segment_info(h, s, ptr(info)), "npr_plan_segment_info")
            D = int(info[6])
            lo = np.zeros(D + 1, dtype=np.int32)
            n = np.zeros(D + 1, dtype=np.int32)
            check(L.npr_plan_segment_band(h, s, ptr(lo), ptr(n)), "npr_plan_segment_band")
            out.append(dict(xs=int(info[0]), ys=int(info[1]), xe=int(info[2]), ye=int(info[3]),
                            ragged_start=int(info[4]), ragged_end=int(info[5]), D=D, cells=int(info[7]), lo=lo,
                            n=n))
    return out


def frame_schedule(params, lX, lY, guide, slots, slots_per_lane, segment=0):
    """Frame schedule of the register kernels for one segment of the plan (host logic, no GPU needed):
    dict(jlo, rebase, row_off, cells) or None when a frame of `slots` slots cannot follow the band
    (include/nprealign.h: npr_plan_frame_schedule)."""
    with _plan(params, lX, lY, guide) as (L, h):
        info = np.zeros(8, dtype=np.int64)
        check(L.npr_plan_segment_info(h, segment, ptr(info)), "npr_plan_segment_info")
        D = int(info[6])
        jlo = np.zeros(D + 1, dtype=np.int32)
        reb = np.zeros(D + 1, dtype=np.int32)
        off = np.zeros(D + 1, dtype=np.uint32)
        cells = np.zeros(1, dtype=np.int64)
        rc = L.npr_plan_frame_schedule(h, segment, slots, slots_per_lane, ptr(jlo), ptr(reb), ptr(off), ptr(cells))
        if rc == _lib.ERR_BAND_TOO_WIDE:
            return None
        check(rc, "npr_plan_frame_schedule")
        return dict(jlo=jlo, rebase=reb, row_off=off, cells=int(cells[0]))


def stripes(params, lX, lY, guide, slots_per_lane=2, segment=0):
    """Stripe table of the wide-band kernel for one segment of the plan (host logic, no GPU needed):
    dict(X, K, df, dl, row0 -- arrays per stripe --, rows) (include/nprealign.h: npr_plan_stripes)."""
    with _plan(params, lX, lY, guide) as (L, h):
        S = check(L.npr_plan_stripes(h, segment, slots_per_lane, None, 0, None), "npr_plan_stripes")
        tab = np.zeros((S, 5), dtype=np.int32)
        rows = np.zeros(1, dtype=np.int64)
        check(L.npr_plan_stripes(h, segment, slots_per_lane, ptr(tab), S, ptr(rows)), "npr_plan_stripes")
        return dict(X=tab[:, 0].copy(), K=tab[:, 1].copy(), df=tab[:, 2].copy(), dl=tab[:, 3].copy(),
                    row0=tab[:, 4].copy(), rows=int(rows[0]))


def format_cigars(ops_off, ops):
    """SAM CIGAR text of every op list of a CSR pair as Batch.ops() returns it: (bytes buffer, offsets[n+1])
    (include/nprealign.h: npr_format_cigars)."""
    L = _lib.load()
    ops_off, ops = _arr(ops_off, np.int64), _arr(ops, np.int32, 2)
    n = len(ops_off) - 1
    str_off = np.zeros(n + 1, dtype=np.int64)
    return _sized(L.npr_format_cigars, "npr_format_cigars", [n, ptr(ops_off), ptr(ops), ptr(str_off)]), str_off


def format_cigars_packed(word_off, n_ops, words):
    """SAM CIGAR text from packed cigars (one uint32 per op, length << 2 | op), list i at words[word_off[i] .. + n_ops[i]):
    (bytes buffer, offsets[n+1]) (include/nprealign.h: npr_format_cigars_packed)."""
    L = _lib.load()
    packed = _packed_cigars(word_off, n_ops, words)
    n = len(packed[1])
    str_off = np.zeros(n + 1, dtype=np.int64)
    return _sized(L.npr_format_cigars_packed, "npr_format_cigars_packed", [n, *map(ptr, packed), ptr(str_off)]), str_off


def cigar_text_packed(ctx, word_off, n_ops, words):
    """format_cigars_packed with the text made on the device of `ctx` (include/nprealign.h: npr_cigar_text_packed; the kernels of
    csrc/npr_cigtext.hip on lists given on the host): (bytes buffer, offsets[n+1])."""
    L = _lib.load()
    packed = _packed_cigars(word_off, n_ops, words)
    n = len(packed[1])
    str_off = np.zeros(n + 1, dtype=np.int64)
    return _sized(L.npr_cigar_text_packed, "npr_cigar_text_packed", [ctx._h, n, *map(ptr, packed), ptr(str_off)], ctx), str_off


def format_sam_records(qnames, ref_names, ref_index, pos, word_off, n_ops, words, seq, seq_off, flag=None, mapq=None):
    """The realigned SAM records as one uint8 array + offsets[n+1] (include/nprealign.h: npr_format_sam_records).  qnames /
    ref_names: lists of bytes; pos 1-based; cigars packed as for format_cigars_packed; seq: uint8 array of read bases with
    CSR offsets seq_off (relative to seq[0])."""
    L = _lib.load()
    n = len(qnames)
    qn, qoff = _ragged(qnames)
    rn, roff = _ragged(ref_names)
    ref_index, pos = _arr(ref_index, np.int32), _arr(pos, np.int64)
    packed = _packed_cigars(word_off, n_ops, words)
    seq, seq_off = _arr(seq, np.uint8), _arr(seq_off, np.int64)
    flag, mapq = _arr(flag, np.int32), _arr(mapq, np.int32)
    rec_off = np.zeros(n + 1, dtype=np.int64)
    args = [n, ptr(qn), ptr(qoff), ptr(flag), ptr(rn), ptr(roff), ptr(ref_index), ptr(pos), ptr(mapq), *map(ptr, packed), ptr(seq),
            ptr(seq_off), ptr(rec_off)]
    return _sized(L.npr_format_sam_records, "npr_format_sam_records", args), rec_off


def seed_sam_text(text, name_span, begin, end, ref_names, hit_off, hits):
    """The matches SeedIndex.matches returned as the SAM records of a base mapper, one per match (include/nprealign.h:
    npr_seed_sam_text; host code, no device needed): (uint8 array, offsets[m + 1]).  Read i is text[begin[i]:end[i]] and is named
    text[name_span[i, 0]:name_span[i, 1]] (FastqTable.text / .seq_span / .name_span); ref_names: list of bytes."""
    L = _lib.load()
    text, name_span, begin, end = spans = _read_spans(text, name_span, begin, end)
    hit_off, hits = _arr(hit_off, np.int64), _arr(hits, np.int32, 4)
    n = len(begin)
    if not (len(end) == len(name_span) == n and len(hit_off) == n + 1 and int(hit_off[-1]) == len(hits)):
        raise NprError(_lib.ERR_INVALID, "npr_seed_sam_text", "one name, begin and end per read, hit_off[n + 1], one row per match")
    rn, roff = _ragged(ref_names)
    rec_off = np.zeros(len(hits) + 1, dtype=np.int64)
    args = [n, *map(ptr, spans), ptr(rn), ptr(roff), len(ref_names), ptr(hit_off), ptr(hits), ptr(rec_off)]
    return _sized(L.npr_seed_sam_text, "npr_seed_sam_text", args), rec_off


def seed_chain_sam_text(text, name_span, begin, end, ref_names, chain_off, chains, ops_off, ops):
    """The chains Context.seed_chains returned as the records chainSamFile writes, one per chain, sorted by (reference index, read name)
    (include/nprealign.h: npr_seed_chain_sam_text; host code, no device needed): (uint8 array, offsets[m + 1]).  Reads and names as
    seed_sam_text takes them; read names must be unique."""
    L = _lib.load()
    text, name_span, begin, end = spans = _read_spans(text, name_span, begin, end)
    chain_off, chains, ops_off, ops = _arr(chain_off, np.int64), _arr(chains, np.int32, 4), _arr(ops_off, np.int64), _arr(ops, np.int32, 2)
    n = len(begin)
    if not (len(end) == len(name_span) == n and len(chain_off) == n + 1 and int(chain_off[-1]) == len(chains) and len(ops_off) == len(chains) + 1
            and int(ops_off[-1]) == len(ops)):
        raise NprError(_lib.ERR_INVALID, "npr_seed_chain_sam_text", "one name, begin and end per read, chain_off[n + 1], one row per chain, ops_off[m + 1], one pair per op")
    rn, roff = _ragged(ref_names)
    rec_off = np.zeros(len(chains) + 1, dtype=np.int64)
    args = [n, *map(ptr, spans), ptr(rn), ptr(roff), len(ref_names), ptr(chain_off), ptr(chains), ptr(ops_off), ptr(ops), ptr(rec_off)]
    return _sized(L.npr_seed_chain_sam_text, "npr_seed_chain_sam_text", args), rec_off


def mea_cigar(lX, lY, x, y, p, gap_gamma=0.5, match_gamma=0.0):
    L = _lib.load()
    x, y, p = _arr(x, np.int32), _arr(y, np.int32), _arr(p, np.float32)
    cap = 2 * len(x) + 8
    ops = np.zeros((cap, 2), dtype=np.int32)
    score = C.c_double(0)
    k = check(L.npr_mea_cigar(lX, lY, ptr(x), ptr(y), ptr(p), len(x), gap_gamma, match_gamma, ptr(ops), cap, C.byref(score)), "npr_mea_cigar")
    return [(int(a), int(c)) for a, c in ops[:k]], score.value


def rescore(guide, x, y, p):
    L = _lib.load()
    g, x, y, p = _arr(guide, np.int32, 2), _arr(x, np.int32), _arr(y, np.int32), _arr(p, np.float32)
    score = C.c_double(0)
    check(L.npr_rescore(ptr(g), len(g), ptr(x), ptr(y), ptr(p), len(x), C.byref(score)), "npr_rescore")
    return score.value


def names_mark(names_text, name_span, sam_text, span, fields, mark):
    """Which names a SAM file maps (include/nprealign.h: npr_names_mark; host code, no device needed): sets mark[i] = 1 for every
    name i = names_text[name_span[i, 0]:name_span[i, 1]] that is the QNAME of an alignment line with a reference and without
    FLAG 4 -- span / fields as SamText.span / SamText.parse() give them; marks already set stay set.  `mark`: uint8 [n],
    written in place.  Returns the number of such lines whose QNAME is none of the names."""
    names_text, sam_text = _arr(names_text, np.uint8), _arr(sam_text, np.uint8)
    name_span, span, fields = _arr(name_span, np.int64, 2), _arr(span, np.int64, 2), _arr(fields, np.int64, _lib.SAM_COLS)
    if not (isinstance(mark, np.ndarray) and mark.dtype == np.uint8 and mark.flags.c_contiguous and mark.shape == (len(name_span),)) or len(span) != len(fields):
        raise NprError(_lib.ERR_INVALID, "npr_names_mark", "mark must be a contiguous uint8 array with one entry per name, span and fields one row per line")
    return int(check(_lib.load().npr_names_mark(ptr(names_text), ptr(name_span), len(name_span), ptr(sam_text), ptr(span), ptr(fields), len(span), ptr(mark)),
                     "npr_names_mark"))


def encode(seq):
    L = _lib.load()
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    a = np.frombuffer(seq, dtype=np.uint8)
    out = np.zeros(len(a), dtype=np.uint8)
    L.npr_encode_bases(ptr(a), len(a), ptr(out))
    return out

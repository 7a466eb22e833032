"""ctypes binding of libnprealign.so (C ABI: include/nprealign.h).

The library is the only execution path of the realigner: if it is missing this module raises
ImportError-like RuntimeError on first use, and `Context()` raises when no gfx950 device is usable.
There is no CPU fallback.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_LOADED = False  # set when the library (and with it the HIP runtime) has been loaded into this process


def want_hw_queues(n=8):
    """The files -> file job (job.py) keeps three batches in flight, each with its own streams; the HIP runtime spreads a process's streams over
    GPU_MAX_HW_QUEUES hardware queues (default 4) and a queue runs its kernels in submission order, so with four the MEA stage of one chunk
    and the DP pass of the next regularly share one (403 against 393 ms per 50 000 reads).  The runtime reads the variable
    at the process's first HIP call.  This is a DEPLOYMENT setting: importing the binding changes nothing in the host
    application's environment -- the job's entry points and bench.py call this, it leaves a value the host has chosen alone, and it says on
    stderr (NPR_TIMING / NPR_JOB_TRACE) what it did, including when it comes too late to matter."""
    have = os.environ.get("GPU_MAX_HW_QUEUES")
    if have is None:
        os.environ["GPU_MAX_HW_QUEUES"] = str(n)
    if os.environ.get("NPR_TIMING") or os.environ.get("NPR_JOB_TRACE"):
        import sys
        sys.stderr.write("[npr] GPU_MAX_HW_QUEUES %s%s\n" % (
            "left at the host's %s" % have if have is not None else "set to %d for this process and its children" % n,
            " (the library is already loaded: the runtime may have read it before)" if LIB_LOADED and have is None else ""))


LIB_PATH = os.environ.get("NPR_LIB") or os.path.join(_HERE, "libnprealign.so")  # NPR_LIB: another build of the library

OK = 0
ERR_INVALID, ERR_ZERO_PROB, ERR_CAPACITY, ERR_MODEL, ERR_NO_DEVICE, ERR_HIP, ERR_BAND_TOO_WIDE, ERR_NOMEM, \
    ERR_STATE = -1, -2, -3, -4, -5, -6, -7, -8, -9
OP_M, OP_I, OP_D = 0, 1, 2
BAND_ANCHOR, BAND_FIXED = 0, 1
MODE_REALIGN, MODE_RESCORE_ORIGINAL, MODE_ALL_POSTERIORS, MODE_EXPECTATIONS = 0, 1, 2, 3
OPT_OVERLAP = 1
FINISH_DEVICE, FINISH_HOST = 0, 1  # npr_batch_debug_finish_stage
OPT_RELEASE_SCRATCH = 2
# test / bring-up switches (include/nprealign.h: NPR_OPT_*; none changes a result)
OPTIONS = dict(kernel=3, arith=4, pair=5, no_tile=6, no_wide=7, tile_rs=8, tile_waves=9, host_mea=13, mea_ring_only=14,
               mea_global_sort=15, em_generic=17, mea_wide_ops=20, em_tile=21, finish_text=22)
OPT_FINISH_TEXT = 22  # NPR_OPT_FINISH_TEXT: the device MEA stage hands over the cigars as SAM text (0 by default; no result changes)
KERNEL_GENERIC, ARITH_CELL, PAIR_NEVER, PAIR_LONG, PAIR_ALL = 1, 1, 1, 2, 3
STATS_WORDS = 40  # NPR_STATS_WORDS
KMER_MAX_K = 6    # the k-mer tables: 4^k + 1 bins, the last one for k-mers with a base outside ACGT
KMER_MAX_GROUPS = 64  # npr_kmer_counts_groups: tables of one call
RQ_POS_BINS, RQ_QUAL_COLS, RQ_GC_COLS, RQ_TOTALS = 336, 95, 102, 8  # NPR_RQ_*: the read-quality tables (npr_read_quality)
RQ_MAX_GROUPS, RQ_TILE = 8, 2048  # NPR_RQ_MAX_GROUPS; NPR_RQ_TILE: positions of one read a workgroup of its kernel takes per step
AQ_MAX_WINDOWS, AQ_WIN_WORDS, AQ_TOTALS, AQ_HOMOPOLYMER = 65536, 8, 8, 3  # NPR_AQ_*: the alignment-quality tables (npr_pileup_coverage, npr_align_quality)
AQ_TILE = 2048    # NPR_AQ_TILE: consecutive rows a workgroup of the coverage kernel takes
SAM_COLS = 16     # NPR_SAM_COLS
SAM_TAIL_COLS = 8  # NPR_SAM_TAIL_COLS: what npr_sam_parse_tail fills per line
BGZF_PAYLOAD = 65280  # NPR_BGZF_PAYLOAD: data bytes of a full BGZF block
BAM_TILE = 4096   # NPR_BAM_TILE: bases of one record a workgroup of the BAM encode kernel takes
SEED_MIN_K, SEED_MAX_K = 8, 32  # npr_seed_index_create: the k of a seed index
SEED_MAP_LDS_ROWS = 4096  # NPR_SEED_MAP_LDS_ROWS: a read of at most so many rows is sorted in LDS by npr_seed_map_create, a longer one in global memory
PILEUP_WORDS = 8  # NPR_PILEUP_WORDS: M columns by read base A C G T other, deletion columns, insertion runs, record starts
SNP_BINS, SNP_MAX_MODELS = 101, 4  # NPR_SNP_BINS, NPR_SNP_MAX_MODELS
MAX_MODELS = 8
E_DEAD = -(1 << 28)


class Params(C.Structure):
    _fields_ = [
        ("band_mode", C.c_int32),
        ("diagonal_expansion", C.c_int32),
        ("constraint_trim", C.c_int32),
        ("split_threshold", C.c_int64),
        ("fixed_width", C.c_int32),
        ("gap_gamma", C.c_double),
        ("match_gamma", C.c_double),
        ("posterior_threshold", C.c_double),
        ("mode", C.c_int32),
        ("max_pairs_per_base", C.c_int32),
    ]


class ReadResult(C.Structure):
    _fields_ = [
        ("status", C.c_int32),
        ("n_segments", C.c_int32),
        ("cells", C.c_int64),
        ("loglik", C.c_double),
        ("loglik_bwd", C.c_double),
        ("score", C.c_double),
        ("n_ops", C.c_int64),
        ("n_pairs", C.c_int64),
    ]


RESULT_DTYPE = np.dtype([("status", np.int32), ("n_segments", np.int32), ("cells", np.int64),
                         ("loglik", np.float64), ("loglik_bwd", np.float64), ("score", np.float64),
                         ("n_ops", np.int64), ("n_pairs", np.int64)], align=True)


class BatchStats(C.Structure):
    _fields_ = [
        ("n_reads", C.c_int64),
        ("n_tasks", C.c_int64),
        ("cells", C.c_int64),
        ("diagonals", C.c_int64),
        ("max_width", C.c_int64),
        ("device_bytes", C.c_int64),
        ("slots", C.c_int64),
        ("kernel_variant", C.c_int32),
    ]


class SnpCalls(C.Structure):  # npr_snp_calls: what the SNP-call entry points return per error model
    _fields_ = [
        ("true_pos", C.c_int64 * SNP_BINS),
        ("false_pos", C.c_int64 * SNP_BINS),
        ("not_called", C.c_int64),
        ("rows_called", C.c_int64),
    ]


class NprError(RuntimeError):
    def __init__(self, code, where, detail=""):
        self.code = code
        msg = "%s failed: %s (%d)" % (where, strerror(code), code)
        if detail:
            msg += " -- " + detail
        RuntimeError.__init__(self, msg)


vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_params, _out = C.POINTER(Params), C.POINTER(vp)
# every symbol include/nprealign.h declares: name -> (restype, argtypes), in the header's order
SIGNATURES = {
    "npr_abi_version": (i32, []),
    "npr_strerror": (C.c_char_p, [i32]),
    "npr_create": (i32, [i32, _out, C.c_char_p, C.c_size_t]),
    "npr_destroy": (None, [vp]),
    "npr_last_error": (C.c_char_p, [vp]),
    "npr_ctx_option": (i32, [vp, i32, i64]),
    "npr_set_hmm": (i32, [vp, i32, vp, vp]),
    "npr_batch_create": (i32, [vp, _params, i64, i64] + [vp] * 8 + [_out]),
    "npr_batch_create_at": (i32, [vp, _params, i64, i64] + [vp] * 9 + [_out]),
    "npr_batch_run": (i32, [vp, C.POINTER(C.c_float)]),
    "npr_batch_finish": (i32, [vp]),
    "npr_batch_destroy": (None, [vp]),
    "npr_batch_get_stats": (i32, [vp, C.POINTER(BatchStats)]),
    "npr_batch_class_stats": (i32, [vp, vp, vp, i32]),
    "npr_batch_segment_arith": (i32, [vp, vp, vp, i64]),
    "npr_batch_results": (i32, [vp, vp]),
    "npr_batch_ops": (i32, [vp, vp, vp, i64]),
    "npr_batch_ops_packed": (i32, [vp, vp, vp, i64]),
    "npr_batch_pairs": (i32, [vp, vp, vp, vp, vp, i64]),
    "npr_batch_debug_set_pairs": (i32, [vp, i64, vp, vp, vp, i64, i32]),
    "npr_batch_debug_finish_stage": (i32, [vp]),
    "npr_batch_debug_refuse": (i32, [vp, vp, i64]),
    "npr_batch_align_stats": (i32, [vp, vp]),
    "npr_align_stats": (i32, [vp, i64, i64] + [vp] * 9),
    "npr_kmer_counts": (i32, [vp, i32, i64, vp, vp, vp]),
    "npr_kmer_counts_groups": (i32, [vp, i32, i64, vp, vp, vp, vp, i32, vp]),
    "npr_align_indel_kmers": (i32, [vp, i32, i64, i64] + [vp] * 10),
    "npr_batch_indel_kmers": (i32, [vp, i32, vp, vp]),
    "npr_read_quality": (i32, [vp, i64] + [vp] * 6 + [i32] + [vp] * 6),
    "npr_pileup_create": (i32, [vp, i64, vp, _out]),
    "npr_pileup_destroy": (None, [vp]),
    "npr_pileup_add_batch": (i32, [vp, vp, vp]),
    "npr_pileup_add": (i32, [vp, i64] + [vp] * 8),
    "npr_pileup_counts": (i32, [vp, vp]),
    "npr_pileup_depth": (i32, [vp, vp, vp]),
    "npr_pileup_coverage": (i32, [vp, vp, vp, i32] + [vp] * 4),
    "npr_align_quality": (i32, [vp, i64] + [vp] * 10 + [i64, vp, vp, i32] + [vp] * 8),
    "npr_seed_index_create": (i32, [vp, i32, i64, vp, vp, _out]),
    "npr_seed_index_destroy": (None, [vp]),
    "npr_seed_matches": (i64, [vp, i64, i32, i64, vp, vp, vp, vp, vp, i64]),
    "npr_seed_sam_text": (i64, [i64] + [vp] * 6 + [i64] + [vp] * 4 + [i64]),
    "npr_seed_chains": (i64, [vp, i64, i64, vp, i64, vp, vp, vp, vp, vp, i64, vp, vp, i64]),
    "npr_seed_chain_sam_text": (i64, [i64] + [vp] * 6 + [i64] + [vp] * 6 + [i64]),
    "npr_seed_map_create": (i32, [vp, i64, i32, i64, i64, vp, vp, vp, _out]),
    "npr_seed_map_counts": (i32, [vp, vp]),
    "npr_seed_map_fetch": (i32, [vp] * 7),
    "npr_seed_map_destroy": (None, [vp]),
    "npr_batch_base_expectations": (i32, [vp, vp, i64, vp, vp, vp]),
    "npr_snp_calls_table": (i32, [vp, i64, vp, vp, vp, vp, i32, vp, vp, vp]),
    "npr_batch_snp_calls": (i32, [vp, vp, i64, vp, vp, vp, i32, vp, vp, vp]),
    "npr_pileup_snp_calls": (i32, [vp, vp, vp, i32, vp, vp, vp]),
    "npr_snp_variants_table": (i64, [vp, i64, vp, vp, vp, vp, vp, dbl] + [vp] * 5 + [i64, C.POINTER(i64)]),
    "npr_batch_snp_variants": (i64, [vp, vp, i64, vp, vp, vp, vp, dbl] + [vp] * 5 + [i64, C.POINTER(i64)]),
    "npr_pileup_snp_variants": (i64, [vp, vp, vp, vp, dbl] + [vp] * 5 + [i64, C.POINTER(i64)]),
    "npr_batch_expectations": (i32, [vp, vp, vp, vp, C.POINTER(C.c_float)]),
    "npr_batch_dense": (i32, [vp, i64, vp, vp, vp, vp, i64]),
    "npr_batch_rs_forward": (i32, [vp, i64, vp, vp, i64]),
    "npr_batch_plan_check": (i64, [vp, vp]),
    "npr_realign_batch": (i32, [vp, _params, i64, i64] + [vp] * 11 + [i64]),
    "npr_plan_create": (i32, [_params, i64, i64, vp, i64, _out]),
    "npr_plan_destroy": (None, [vp]),
    "npr_plan_segments": (i32, [vp]),
    "npr_plan_segment_info": (i32, [vp, i32, vp]),
    "npr_plan_segment_band": (i32, [vp, i32, vp, vp]),
    "npr_plan_frame_schedule": (i32, [vp, i32, i32, i32, vp, vp, vp, vp]),
    "npr_plan_stripes": (i32, [vp, i32, i32, vp, i32, vp]),
    "npr_mea_cigar": (i64, [i64, i64, vp, vp, vp, i64, dbl, dbl, vp, i64, C.POINTER(dbl)]),
    "npr_rescore": (i32, [vp, i64, vp, vp, vp, i64, C.POINTER(dbl)]),
    "npr_chain_hits": (i64, [i64, vp, vp, vp, vp, vp, vp, i64, vp]),
    "npr_chain_merge": (i64, [i64, vp, vp, vp, vp, i64, i64, vp, i64]),
    "npr_format_cigars": (i64, [i64, vp, vp, vp, vp, i64]),
    "npr_format_cigars_packed": (i64, [i64, vp, vp, vp, vp, vp, i64]),
    "npr_cigar_text_packed": (i64, [vp, i64, vp, vp, vp, vp, vp, i64]),
    "npr_batch_cigar_text": (i64, [vp, vp, vp, i64]),
    "npr_format_sam_records": (i64, [i64] + [vp] * 15 + [i64]),
    "npr_encode_bases": (None, [vp, i64, vp]),
    "npr_sam_index": (i64, [vp, i64, C.POINTER(i64), vp, i64]),
    "npr_sam_parse": (i32, [vp, vp, i64, vp, vp, i64, vp]),
    "npr_sam_guides": (i32, [vp, vp, i64, vp, vp]),
    "npr_sam_splice": (i64, [vp, vp, vp, i64, vp, vp, vp, vp, vp, i64]),
    "npr_sam_splice_text": (i64, [vp, vp, vp, i64, vp, vp, vp, vp, i64]),
    "npr_fasta_index": (i64, [vp, i64, vp, vp, i64]),
    "npr_fasta_pack": (i32, [vp, vp, i64, vp, vp]),
    "npr_fastq_index": (i64, [vp, i64, vp, i64]),
    "npr_fastq_qual_index": (i32, [vp, i64, vp, i64, vp]),
    "npr_names_mark": (i64, [vp, vp, i64, vp, vp, vp, i64, vp]),
    "npr_sam_parse_tail": (i32, [vp, vp, vp, i64, vp, vp, i64, vp]),
    "npr_bam_tags": (i64, [vp, vp, i64, vp, vp, i64]),
    "npr_bam_header": (i64, [vp, i64, i32, vp, i64, C.POINTER(i64), vp, i64]),
    "npr_bam_sort_order": (i32, [vp, i64, vp, vp, vp, vp]),
    "npr_bgzf_frame": (i64, [vp, vp, i64, vp, i64]),
    "npr_sam_bam": (i64, [vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, i64, vp, i32, vp, i64, C.POINTER(i64)] + [vp] * 6 + [C.POINTER(i64)]),
    "npr_bgzf_deflate": (i64, [vp, vp, i64, vp, i64, vp]),
    "npr_deflate_last": (i32, [vp, vp]),
    "npr_sam_bam_deflate": (i64, [vp, vp, i64, vp, vp, vp, i64, vp, vp, vp, i64, i64, vp, i32, vp, i64, C.POINTER(i64)] + [vp] * 6 + [C.POINTER(i64)]),
    "npr_bai_write": (i64, [i64, vp, i64] + [vp] * 6 + [i64, vp, i64]),
    "npr_bgzf_scan": (i64, [vp, i64, vp, vp, i64, C.POINTER(i64)]),
    "npr_bgzf_inflate": (i64, [vp, vp, i64, vp, i64]),
    "npr_inflate_last": (i32, [vp, vp]),
    "npr_bam_aux_text": (i64, [vp, vp, i64, vp, vp, vp, vp, i64]),
    "npr_bam_sam": (i64, [vp, vp, i64, vp, i64, C.POINTER(i64)]),
    "npr_bam_open": (i32, [vp, vp, i64, _out]),
    "npr_bam_close": (None, [vp]),
    "npr_bam_stream_info": (i64, [vp, vp]),
    "npr_bam_stream_refs": (i64, [vp, vp, vp, vp, i64]),
    "npr_pileup_add_bam": (i32, [vp, vp, i32, vp]),
    "npr_bai_chunks": (i64, [vp, i64, i32, i64, i64, vp, vp, i64, C.POINTER(i64)]),
    "npr_bam_open_region": (i32, [vp, vp, i64, vp, i64, i32, i64, i64, _out]),
    "npr_bam_stream_restrict": (i64, [vp, i32, i64, i64]),
    "npr_bam_stream_sam": (i64, [vp, vp, i64, C.POINTER(i64)]),
    "npr_bam_streams_bam": (i64, [vp, vp, i64, vp, i64, i32, i32, vp, i64, C.POINTER(i64), C.POINTER(i64)] + [vp] * 6 + [C.POINTER(i64)]),
    "npr_bam_merge_last": (i32, [vp, vp]),
    "npr_bam_index": (i64, [vp, vp, i64, C.POINTER(i64), vp, i64, C.POINTER(i64), vp, vp, vp, vp, i64, vp, i64, vp, C.POINTER(i64)]),
    "npr_batch_create_spans": (i32, [vp, _params, i64, i64] + [vp] * 10 + [_out]),
}
EXPORTS = list(SIGNATURES)

_lib = None


def load():
    """Loads libnprealign.so and gives every symbol its signature; raises RuntimeError (never falls back) when it is absent."""
    global _lib, LIB_LOADED
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("libnprealign.so not found at %s: build it with `python -c 'import __graft_entry__ as g; "
                           "g.build()'` or `make -C nanopore_amd/csrc`; there is no CPU fallback" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    LIB_LOADED = True
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def strerror(code):
    return load().npr_strerror(code).decode()


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(rc, where, ctx=None):
    """The return value of an entry point: a negative one raises NprError (with ctx.last_error() when the Context is given), any other --
    NPR_OK, or the count, length or stage of the entry points that return one -- is handed back."""
    if rc < 0:
        raise NprError(int(rc), where, ctx.last_error() if ctx is not None else "")
    return rc


def _sized(fn, where, args, ctx=None, buffer=None):
    """The two calls of an entry point whose last arguments are (out, cap) and which returns the length of its text: the sizing call
    fn(*args, None, 0), then the filling call into `buffer` (a uint8 array) when that is large enough, else into a new array.  -> the
    text, a view of the array it was written into.  `ctx`: the Context whose last_error() goes with a failure."""
    total = int(check(fn(*args, None, 0), where, ctx))
    if buffer is None or buffer.size < max(total, 1):
        buffer = np.empty(max(total, 1), dtype=np.uint8)  # (filled by the call: no memset first)
    check(fn(*args, ptr(buffer), total), where, ctx)
    return buffer[:total]

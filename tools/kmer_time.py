"""Times the two k-mer kernels (csrc/npr_kmer.hip) on the configs[2] shape: N reads of ~8 kb against their reference windows
(synth.config_c3).  Prints wall times of the C ABI calls and the bytes each kernel has to read; run under
`tools/kstats.sh NAME python tools/kmer_time.py` for the per-kernel device times (rocprofv3 --kernel-trace --stats).

    python tools/kmer_time.py [--reads 50000] [--k 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanopore_amd import _lib, realign, synth  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--k", type=int, default=5)
    args = ap.parse_args()
    hmm = Hmm.loadHmm(os.path.join(os.path.dirname(_lib.LIB_PATH), "mappers", "blasr_hmm_0.txt"))
    w, _ = synth.config_c3(np.asarray(hmm.transitions, dtype=np.float64), np.asarray(hmm.emissions, dtype=np.float64), n_reads=args.reads)
    ctx = realign.Context(0)
    L, ptr = ctx._L, _lib.ptr
    n, nb = args.reads, 4 ** args.k + 1
    read, read_off = np.ascontiguousarray(w["read"]), np.ascontiguousarray(w["read_off"], dtype=np.int64)
    ref, ref_off = np.ascontiguousarray(w["ref"]), np.ascontiguousarray(w["ref_off"], dtype=np.int64)
    ops, ops_off = np.ascontiguousarray(w["guide_ops"], dtype=np.int32), np.ascontiguousarray(w["guide_off"], dtype=np.int64)
    counts, rd, rf = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int64)
    for rep in range(3):
        t0 = time.perf_counter()
        rc = L.npr_kmer_counts(ctx._h, args.k, n, ptr(read), ptr(read_off), ptr(counts))
        t1 = time.perf_counter()
        assert rc == 0, ctx.last_error()
        rc = L.npr_align_indel_kmers(ctx._h, args.k, n, n, ptr(ref), ptr(ref_off), None, ptr(read), ptr(read_off), ptr(ops), ptr(ops_off), None, ptr(rd), ptr(rf))
        t2 = time.perf_counter()
        assert rc == 0, ctx.last_error()
        print("rep %d: npr_kmer_counts %.1f ms (call), npr_align_indel_kmers %.1f ms (call)" % (rep, 1e3 * (t1 - t0), 1e3 * (t2 - t1)))
    print("k_kmer_spectrum reads %d bases (1 byte each) + %d offsets; %d windows counted" % (len(read), n + 1, int(counts.sum())))
    print("k_indel_kmers reads %d cigar words (4 bytes each, twice) of %d records; %d + %d k-mers of %d + %d window bases counted" % (
        len(ops), n, int(rd.sum()), int(rf.sum()), len(read), len(ref)))
    ctx.close()


if __name__ == "__main__":
    main()

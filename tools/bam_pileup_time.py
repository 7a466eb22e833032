"""Times the pileup of a BAM file made where its records lie on the device (analyses/pileup.py pileup_of_bam: npr_bam_open + npr_pileup_add_bam,
csrc/npr_bampile.hip) against the route that existed before it, on the two files tools/bam_read_time.py reads per workload
(synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig, and one eighth of it): the BAM with stored blocks and the one the
device compressed.  Per file, whole calls from the file on disk to the depth arrays on the host, one warm-up, median of seven:
  direct     pileup_of_bam + depth(): read, block scan on the host, inflate, walk, k_bampile_check, k_bampile_add, the running sum and depth
  sam_route  bam_to_sam (file to file) + pileup_of_sam + depth(): the SAM text written, parsed on the host, cigars and bases uploaded again
             (of which bam_to_sam alone is timed too)
The kernels are not timed on their own (the ABI has no event timing): how the wall times split between kernels, copies and host work is not
shown.  Checks that both routes give the same depth, prints the figures and records them in profiles/bam_pileup_time.json.  No threshold.

    python tools/bam_pileup_time.py [--reads 50000] [--out profiles/bam_pileup_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd import synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.analyses.pileup import pileup_of_bam, pileup_of_sam  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def _depth_of(made):
    names, lengths, pileup = made
    try:
        depth, covered = pileup.depth()
        counts = getattr(pileup, "last_bam_counts", None)
    finally:
        pileup.close()
    return depth, covered, counts


def _one(ctx, path, fa):
    sam = path + ".sam"
    (d_depth, d_cov, counts), t_direct = _median_ms(lambda: _depth_of(pileup_of_bam(ctx, path)))
    _, t_text = _median_ms(lambda: ctx.bam_to_sam(path, sam))

    def sam_route():
        ctx.bam_to_sam(path, sam)
        return _depth_of(pileup_of_sam(ctx, sam, fa))
    (s_depth, s_cov, _), t_sam = _median_ms(sam_route)
    return dict(file_bytes=os.path.getsize(path), sam_bytes=os.path.getsize(sam), counts=counts, positions=int(len(d_depth)), m_columns=int(d_depth.sum()),
                same_depth=bool(np.array_equal(d_depth, s_depth) and np.array_equal(d_cov, s_cov)), direct_ms=t_direct, sam_route_ms=t_sam, bam_to_sam_ms=t_text)


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "sorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    ctx.sam_to_bam(sam_path, out)
    ctx.sam_to_bam(sam_path, out + ".z", compress=True)
    print("%d reads: both files written" % n_reads, file=sys.stderr, flush=True)
    return dict(reads=n_reads, stored=_one(ctx, out, fa), compressed=_one(ctx, out + ".z", fa))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_pileup_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times of whole calls from the file on disk to the depth arrays on the host, one warm-up, medians of seven; direct: "
                               "pileup_of_bam + depth(); sam_route: bam_to_sam (file to file) + pileup_of_sam + depth(); the kernels were not timed alone")
    for r in runs:
        for kind in ("stored", "compressed"):
            f = r[kind]
            print("%d reads, %s: %.0f MB file, %d records (%d added), %.0f M M columns: direct %.0f ms; through %.0f MB of SAM text %.0f ms (bam_to_sam alone "
                  "%.0f ms); same depth: %s"
                  % (r["reads"], kind, f["file_bytes"] / 1e6, f["counts"]["records"], f["counts"]["added"], f["m_columns"] / 1e6, f["direct_ms"]["median"],
                     f["sam_bytes"] / 1e6, f["sam_route_ms"]["median"], f["bam_to_sam_ms"]["median"], f["same_depth"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r[k]["same_depth"] for r in runs for k in ("stored", "compressed")):
        sys.exit("the two routes give different depths")


if __name__ == "__main__":
    main()

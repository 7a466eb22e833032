"""Times a region query on an indexed BAM file (analyses/pileup.py pileup_of_bam(region=): npr_bai_chunks + npr_bam_open_region +
npr_pileup_add_bam, csrc/npr_bamregion.hip) against the way to the same numbers that existed before it, on the two files
tools/bam_pileup_time.py reads per workload (synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig, and one eighth of
it): the BAM with stored blocks and the one the device compressed, each with the index the device made.  The region is the hundredth of the
contig in its middle.  Per file, whole calls from the files on disk to the depth array on the host, one warm-up, median of seven:
  region  pileup_of_bam(region=) + depth(), sliced: the index read, the blocks it names crossed and inflated, their chunks walked, the
          overlapping records added
  whole   pileup_of_bam + depth(), sliced: every block inflated, every record walked and added
  brute   pileup_of_bam(region=) with no index: every block inflated, every record walked, the overlapping ones added
Also the blocks and stream bytes inflated by the query against the file's.  The kernels are not timed on their own (the ABI has no event
timing).  Checks that the region's depth is the whole file's there, prints the figures and records them in
profiles/bam_region_time.json.  No threshold.

    python tools/bam_region_time.py [--reads 50000] [--out profiles/bam_region_time.json]
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
from nanopore_amd import bam, synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.analyses.pileup import pileup_of_bam  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def _one(ctx, path):
    names, lengths, pileup = pileup_of_bam(ctx, path)
    pileup.close()
    length = int(lengths[0])
    beg = length // 2
    region = (0, beg, beg + max(length // 100, 1))

    def depth_of(last, **kw):
        names, lengths, pileup = pileup_of_bam(ctx, path, **kw)
        try:
            last.update(bam.inflate_last(ctx), records=pileup.last_bam_counts["records"])
            depth, covered = pileup.depth()
        finally:
            pileup.close()
        return depth[region[1]:region[2]], covered[region[1]:region[2]]
    q, w, b = {}, {}, {}
    (r_depth, r_cov), t_region = _median_ms(lambda: depth_of(q, region=region))
    (w_depth, w_cov), t_whole = _median_ms(lambda: depth_of(w))
    os.rename(path + ".bai", path + ".bai.aside")   # no index beside the file: the whole file, restricted on the device
    try:
        (b_depth, b_cov), t_brute = _median_ms(lambda: depth_of(b, region=region))
    finally:
        os.rename(path + ".bai.aside", path + ".bai")
    same = bool(np.array_equal(r_depth, w_depth) and np.array_equal(r_cov, w_cov) and np.array_equal(b_depth, w_depth) and np.array_equal(b_cov, w_cov))
    return dict(file_bytes=os.path.getsize(path), index_bytes=os.path.getsize(path + ".bai"), region=list(region), positions=length, records=w["records"],
                region_records=q["records"], blocks=w["blocks"], region_blocks=q["blocks"], stream_bytes=w["stream_bytes"], region_stream_bytes=q["stream_bytes"],
                m_columns_in_region=int(w_depth.sum()), same_depth=same, region_ms=t_region, whole_ms=t_whole, brute_ms=t_brute)


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "sorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    ctx.sam_to_bam(sam_path, out)
    ctx.sam_to_bam(sam_path, out + ".z", compress=True)
    print("%d reads: both files written" % n_reads, file=sys.stderr, flush=True)
    return dict(reads=n_reads, stored=_one(ctx, out), compressed=_one(ctx, out + ".z"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_region_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times of whole calls from the files on disk to the depth array on the host, sliced to the region, one warm-up, medians of seven; "
                               "region: pileup_of_bam(region=) through the index; whole: pileup_of_bam of the whole file (the way before); brute: pileup_of_bam(region=) "
                               "without an index; the kernels were not timed alone")
    for r in runs:
        for kind in ("stored", "compressed"):
            f = r[kind]
            print("%d reads, %s: %.0f MB file, region %d-%d of %d: %d of %d blocks inflated, %d of %d records added: through the index %.1f ms; the whole file %.0f ms; "
                  "the whole file restricted %.0f ms; same depth: %s"
                  % (r["reads"], kind, f["file_bytes"] / 1e6, f["region"][1], f["region"][2], f["positions"], f["region_blocks"], f["blocks"], f["region_records"],
                     f["records"], f["region_ms"]["median"], f["whole_ms"]["median"], f["brute_ms"]["median"], f["same_depth"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r[k]["same_depth"] for r in runs for k in ("stored", "compressed")):
        sys.exit("the routes give different depths in the region")


if __name__ == "__main__":
    main()

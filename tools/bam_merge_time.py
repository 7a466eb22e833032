"""Times the BAM -> BAM route (bam.bam_sort: npr_bam_open, npr_bam_streams_bam, csrc/npr_bammerge.hip) on the workloads of
tools/bam_read_time.py (synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig, and one eighth of it), from the BAM
file in the SAM file's order, with stored blocks and with compressed ones.  Per file, one warm-up and the median of seven wall times:
  bam_sort        file to file: the file in the SAM file's order in, the sorted BAM and its BAI out
  text_route      Context.bam_to_sam then Context.sam_to_bam(sort=True) on the same file, file to file: the only route before
  bam_index       (the compressed sorted file) Context.bam_index on the image in memory
  k_merge_gather  the kernel alone, between two events (npr_bam_merge_last), of the last bam_sort: bytes moved = twice the records'
                  bytes (each is read once and written once) over that time
Checks that both routes write the same file and index, prints the figures and records them in profiles/bam_merge_time.json.  No threshold.

    python tools/bam_merge_time.py [--reads 50000] [--out profiles/bam_merge_time.json]
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
from nanopore_amd.hmm import Hmm  # noqa: E402


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def _one(ctx, path, compress):
    direct, text = path + ".direct.bam", path + ".text.bam"

    def text_route():
        ctx.bam_to_sam(path, path + ".sam")
        return ctx.sam_to_bam(path + ".sam", text, sort=True, index=True, compress=compress)

    gather = []

    def direct_route():
        counts = bam.bam_sort(ctx, path, direct, compress=compress)
        gather.append(ctx.bam_merge_last())
        return counts

    counts, t_direct = _median_ms(direct_route)
    _, t_text = _median_ms(text_route)
    same = open(direct, "rb").read() == open(text, "rb").read() and open(direct + ".bai", "rb").read() == open(text + ".bai", "rb").read()
    ns = float(np.median([g["gather_ns"] for g in gather[1:]]))
    moved = 2 * gather[-1]["gather_bytes"]
    out = dict(file_bytes=os.path.getsize(path), stream_bytes=counts["stream_bytes"], records=counts["records"], out_bytes=counts["bytes"], same_file_and_index=bool(same),
               bam_sort_ms=t_direct, text_route_ms=t_text, text_over_direct=t_text["median"] / t_direct["median"],
               k_merge_gather=dict(median_us=ns / 1e3, bytes_moved=moved, tb_per_s=moved / ns / 1e3 if ns else None))
    if compress:
        image = np.fromfile(direct, dtype=np.uint8)
        bai, t_index = _median_ms(lambda: ctx.bam_index(image))
        out["bam_index_ms"], out["bam_index_same"] = t_index, bool(bai.tobytes() == open(direct + ".bai", "rb").read())
    return out


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "unsorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    ctx.sam_to_bam(sam_path, out, sort=False, index=False)
    ctx.sam_to_bam(sam_path, out + ".z", sort=False, index=False, compress=True)
    print("%d reads: both files written" % n_reads, file=sys.stderr, flush=True)
    return dict(reads=n_reads, stored=_one(ctx, out, False), compressed=_one(ctx, out + ".z", True))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_merge_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times file to file, one warm-up, medians of seven; k_merge_gather: between two events around the launch, bytes moved = "
                               "twice the records' bytes")
    for r in runs:
        for kind in ("stored", "compressed"):
            f = r[kind]
            print("%d reads, %s: %.0f MB file, %.0f MB stream: bam_sort %.0f ms, bam_to_sam + sam_to_bam %.0f ms (%.2fx); k_merge_gather %.0f us, %.2f TB/s; "
                  "same file and index: %s%s"
                  % (r["reads"], kind, f["file_bytes"] / 1e6, f["stream_bytes"] / 1e6, f["bam_sort_ms"]["median"], f["text_route_ms"]["median"], f["text_over_direct"],
                     f["k_merge_gather"]["median_us"], f["k_merge_gather"]["tb_per_s"] or 0.0, f["same_file_and_index"],
                     "; bam_index %.0f ms" % f["bam_index_ms"]["median"] if "bam_index_ms" in f else ""), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r[k]["same_file_and_index"] for r in runs for k in ("stored", "compressed")):
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()

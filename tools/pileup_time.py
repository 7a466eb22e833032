"""Times the device pileup (csrc/npr_pileup.hip): `Pileup.add_batch` + `depth()` on a finished batch of bench.py's default workload, and
`pileup_of_sam` + `depth()` on the SAM file of the 50 000-read set of `bench.py --workload c3` (local records on one 4.6 Mb contig).
One warm-up, then the median of seven repetitions with their spread; writes profiles/pileup_time.json.

    python tools/pileup_time.py [--batch-reads 24576] [--sam-reads 50000] [--reps 7] [--out profiles/pileup_time.json]

`--context NAME=SECONDS` (repeatable) records a wall time measured elsewhere beside the device figures, e.g. the reference's path
(`samtools view | sort | depth`) on some CPU: context for a reader, not a comparison this tool makes.
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nanopore_amd import realign, synth  # noqa: E402
from nanopore_amd.analyses.pileup import pileup_of_sam  # noqa: E402


def spread(seconds):
    ms = sorted(1e3 * s for s in seconds)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch-reads", type=int, default=24576)
    ap.add_argument("--sam-reads", type=int, default=50000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup_time.json"))
    ap.add_argument("--context", action="append", default=[])
    args = ap.parse_args()
    ctx = realign.Context(0)
    out = {"tool": "tools/pileup_time.py", "context": dict((kv.split("=", 1)[0], float(kv.split("=", 1)[1])) for kv in args.context)}

    # a finished batch of the default workload: the table is made where its cigars lie
    h, w, W, label = bench.build_workload("northstar", args.batch_reads, 0)
    ctx.set_hmm(h)
    b = ctx.stage_csr(bench.make_params(W), w["ref"], w["ref_off"], w["read"], w["read_off"], w["guide_ops"], w["guide_off"],
                      guide_start=w.get("guide_start"), ref_index=w.get("ref_index"))
    b.run(), b.finish()
    ref_lengths = np.diff(np.asarray(w["ref_off"], dtype=np.int64))
    add, depth, both = [], [], []
    for rep in range(args.reps + 1):
        pl = ctx.pileup(ref_lengths)
        t0 = time.perf_counter()
        pl.add_batch(b)
        t1 = time.perf_counter()
        d, covered = pl.depth()
        t2 = time.perf_counter()
        pl.close()
        if rep:
            add.append(t1 - t0), depth.append(t2 - t1), both.append(t2 - t0)
    out["add_batch"] = {"workload": label, "reads": args.batch_reads, "positions": int(ref_lengths.sum()), "m_columns": int(d.sum()),
                        "covered_positions": int(covered.sum()), "add_batch": spread(add), "depth": spread(depth), "add_batch_and_depth": spread(both)}
    b.close()
    del d, covered
    ctx.release_scratch()

    # the c3 set from its SAM file
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=args.sam_reads)
    with tempfile.TemporaryDirectory() as tmp:
        sam, fa = os.path.join(tmp, "reads.sam"), os.path.join(tmp, "contig.fa")
        synth.write_workload_files(w, sam, fa, ref_names=["ecoli_like_contig"])
        whole, depth = [], []
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            names, lengths, pl = pileup_of_sam(ctx, sam, fa)
            t1 = time.perf_counter()
            d, covered = pl.depth()
            t2 = time.perf_counter()
            pl.close()
            if rep:
                whole.append(t1 - t0), depth.append(t2 - t1)
        out["pileup_of_sam"] = {"reads": args.sam_reads, "sam_bytes": os.path.getsize(sam), "positions": int(lengths.sum()), "m_columns": int(d.sum()),
                                "mean_depth": float(d.mean()), "pileup_of_sam": spread(whole), "depth": spread(depth)}
    ctx.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

"""Times the SNP-variant call on a pileup (csrc/npr_snpcall.hip: k_snp_variants_count / a scan / k_snp_variants_emit) against the host route it replaces,
on one synthetic input: a random 4.6 Mb contig under reads of 5 000 bases at ten-fold depth (the depth of tools/snp_calls_time.py's
defaults), every read a copy of its interval with 10 % of the bases substituted and one M run as its cigar, 1 % of the reference bases
changed afterwards so that there is something to call.  Three figures, each one warm-up and then the median of seven repetitions:
  device    Pileup.snp_variants: best base, quality and the calls at threshold 0.5, everything that comes back included
  host      Pileup.counts() (the table over PCIe), basePosteriors, thresholding and argmax in numpy
  histograms  Pileup.snp_calls with the same error model: what the histogram kernel alone costs, for the price of the second pass and
              the dense outputs
Checks that device and host name the same best bases and calls, prints the medians and writes profiles/snp_variants_time.json.

    python tools/snp_variants_time.py [--genome 4600000] [--read-len 5000] [--depth 10] [--reps 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd import realign  # noqa: E402
from nanopore_amd.analyses.marginAlignSnpCaller import NULL_MATRIX, basePosteriors, errorMatrixOfHmm  # noqa: E402
from nanopore_amd.analyses.utils import trainedModelPath  # noqa: E402

THRESHOLD = 0.5


def spread(seconds):
    ms = sorted(1e3 * s for s in seconds)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def host_route(pileup, ref, error):
    counts = pileup.counts()
    weights = counts[:, :4].astype(np.float64)
    total = weights.sum(axis=1)
    where = np.flatnonzero((counts[:, :5].sum(axis=1) > 0) & (total > 0) & (ref <= 3))
    post = basePosteriors(weights[where] / total[where, None], ref[where], NULL_MATRIX, error)
    best = np.full(len(ref), 4, dtype=np.uint8)
    best[where] = post.argmax(axis=1)
    called = (post >= THRESHOLD) & (np.arange(4)[None, :] != ref[where, None])
    row, alt = np.nonzero(called)
    return best, where[row], alt.astype(np.uint8), post[row, alt]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--depth", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "snp_variants_time.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = rng.integers(0, 4, size=args.genome).astype(np.uint8)
    n = int(args.depth * args.genome / args.read_len)
    starts = rng.integers(0, args.genome - args.read_len, size=n)
    reads = genome[(starts[:, None] + np.arange(args.read_len)[None, :]).reshape(-1)]
    swap = rng.random(reads.size) < 0.1
    reads[swap] = (reads[swap] + rng.integers(1, 4, size=int(swap.sum()))) % 4
    ref = genome.copy()
    at = rng.choice(args.genome, size=args.genome // 100, replace=False)
    ref[at] = (ref[at] + rng.integers(1, 4, size=len(at))) % 4
    error = errorMatrixOfHmm(trainedModelPath("blasr_hmm_20.txt"))
    ctx = realign.Context(0)
    pileup = ctx.pileup([args.genome])
    ops = np.stack([np.zeros(n, dtype=np.int32), np.full(n, args.read_len, dtype=np.int32)], axis=1)
    pileup.add_csr(letters[reads], np.arange(n + 1, dtype=np.int64) * args.read_len, None, ops, np.arange(n + 1, dtype=np.int64),
                   np.zeros(n, dtype=np.int32), start=np.stack([starts, np.zeros(n, dtype=np.int64)], axis=1))
    laps = {"device": [], "host": [], "histograms": []}
    for rep in range(args.reps + 1):
        t0 = time.perf_counter()
        best, qual, row, alt, p = pileup.snp_variants(ref, NULL_MATRIX, error, THRESHOLD)
        t1 = time.perf_counter()
        h_best, h_row, h_alt, h_p = host_route(pileup, ref, error)
        t2 = time.perf_counter()
        counted = pileup.snp_calls(ref, None, NULL_MATRIX, (error,))
        t3 = time.perf_counter()
        if rep:
            laps["device"].append(t1 - t0), laps["host"].append(t2 - t1), laps["histograms"].append(t3 - t2)
    pileup.close()
    ctx.close()
    same = bool(np.array_equal(best, h_best) and np.array_equal(row, h_row) and np.array_equal(alt, h_alt) and np.abs(p - h_p).max() <= 1e-12)
    res = dict(tool="tools/snp_variants_time.py", genome=args.genome, reads=n, read_len=args.read_len, depth=args.depth, threshold=THRESHOLD,
               calls=int(len(row)), rows_called=int(counted[0][3]), same_calls=same, device_ms=spread(laps["device"]), host_ms=spread(laps["host"]),
               histograms_ms=spread(laps["histograms"]),
               note="wall times on one pileup already on the device: device = Pileup.snp_variants (best, qual and calls copied back), host = "
                    "Pileup.counts + basePosteriors + threshold + argmax in numpy, histograms = Pileup.snp_calls with the same error model")
    print("device %.2f ms; host %.1f ms; histograms %.2f ms; %d calls; same calls: %s"
          % (res["device_ms"]["median_ms"], res["host_ms"]["median_ms"], res["histograms_ms"]["median_ms"], res["calls"], same))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not same:
        sys.exit("device and host disagree")


if __name__ == "__main__":
    main()

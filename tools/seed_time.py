"""Times the seed index and the match passes (csrc/npr_seed.hip) on the configs[2]-like shape: N reads of ~8 kb drawn from a 4.6 Mb random
reference through the error channel of blasr_hmm_0, half of them reverse-complemented, k = 16, min_len = 20, both strands.  Records wall
times of the calls (one warm-up, median of seven, min - max) and matches per second into profiles/seed_time.json; run under
`tools/kstats.sh NAME python tools/seed_time.py --launches` for the per-kernel device times (rocprofv3 --kernel-trace --stats).

    python tools/seed_time.py [--reads 50000] [--genome 4600000] [--launches]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd import _lib, realign, synth  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--genome", type=int, default=4600000)
    ap.add_argument("--read-len", type=int, default=8000)
    ap.add_argument("--launches", action="store_true", help="one index build and one match call only (for a kernel trace); writes no profile")
    args = ap.parse_args()
    hmm = Hmm.loadHmm(os.path.join(os.path.dirname(_lib.LIB_PATH), "mappers", "blasr_hmm_0.txt"))
    rng = np.random.default_rng(3)
    genome = rng.integers(0, 4, size=args.genome).astype(np.uint8)
    starts = rng.integers(0, args.genome - args.read_len, size=args.reads)
    off = np.arange(args.reads + 1, dtype=np.int64) * args.read_len
    slices = genome[(starts[:, None] + np.arange(args.read_len)[None, :]).reshape(-1)]
    codes, read_off, _, _ = synth.error_channel(rng, slices, off, np.asarray(hmm.transitions, dtype=np.float64), np.asarray(hmm.emissions, dtype=np.float64))
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    text = letters[codes]
    for i in range(1, args.reads, 2):  # every other read on the reverse strand
        text[read_off[i]:read_off[i + 1]] = letters[3 - codes[read_off[i]:read_off[i + 1]][::-1]]
    begin, end = np.ascontiguousarray(read_off[:-1]), np.ascontiguousarray(read_off[1:])
    ctx = realign.Context(0)
    ref, ref_off = letters[genome], np.array([0, args.genome], dtype=np.int64)
    reps = 1 if args.launches else 8
    t_index, t_match, matches = [], [], 0
    for rep in range(reps):
        t0 = time.perf_counter()
        index = ctx.seed_index_csr(ref, ref_off, 16)
        t1 = time.perf_counter()
        hit_off, hits = index.matches(text, begin, end, 20, 3)
        t2 = time.perf_counter()
        index.close()
        matches = len(hits)
        if rep or args.launches:
            t_index.append(1e3 * (t1 - t0)), t_match.append(1e3 * (t2 - t1))
        print("rep %d: index %.1f ms, matches %.1f ms (%d matches of %d reads)" % (rep, 1e3 * (t1 - t0), 1e3 * (t2 - t1), matches, args.reads))
    ctx.close()
    if args.launches:
        return
    out = dict(reads=args.reads, read_bases=int(read_off[-1]), genome=args.genome, k=16, min_len=20, strands=3, matches=matches,
               index_ms=dict(median=float(np.median(t_index)), min=min(t_index), max=max(t_index)),
               matches_ms=dict(median=float(np.median(t_match)), min=min(t_match), max=max(t_match)),
               matches_per_s=matches / (1e-3 * float(np.median(t_match))),
               note="wall times of SeedIndex() and SeedIndex.matches() (count call + fetch call per chunk of 64 M bases, host sort included)")
    with open(os.path.join(ROOT, "profiles", "seed_time.json"), "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()

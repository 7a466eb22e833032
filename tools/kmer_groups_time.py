"""Times the grouped k-mer count (csrc/npr_kmer.hip: k_kmer_spectrum_groups) beside the one-table kernel on the configs[2] shape:
N reads of ~8 kb (synth.config_c3), k = 5, the reads dealt round-robin into G groups.

    python tools/kmer_groups_time.py [--reads 50000] [--k 5] [--groups 2,8] [--reps 7] [--out FILE.json]
        wall times of whole calls, one warm-up and the median of --reps with the range: `npr_kmer_counts_groups` (staging copy, H2D,
        kernel, D2H) against the same bases sent through `npr_kmer_counts` once per group, with and without the host gather that
        makes a group contiguous first; `npr_kmer_counts` on all bases as one table for scale.  Checks the tables agree.
    tools/kstats.sh NAME python tools/kmer_groups_time.py --launches [--groups ...]
        the same launches in a fixed order and nothing else, for `rocprofv3 --kernel-trace --stats`: 1 + reps of k_kmer_spectrum
        on all bases, then 1 + reps of k_kmer_spectrum_groups per entry of --groups.
    python tools/kmer_groups_time.py --trace KERNEL_TRACE.csv [--groups ...] [--reps 7]
        reads that run's kernel trace: per kernel and group count the median, minimum and maximum of the launches after the warm-up.
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def trace_summary(path, groups, reps):
    with open(path) as f:
        rows = sorted(csv.DictReader(f), key=lambda r: int(r["Start_Timestamp"]))
    ms = lambda grouped: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows
                          if "k_kmer_spectrum" in r["Kernel_Name"] and ("k_kmer_spectrum_groups" in r["Kernel_Name"]) == grouped]
    single, grouped = ms(False), ms(True)
    out = {}
    if len(single) >= reps + 1:
        out["k_kmer_spectrum"] = spread(single[1:reps + 1])
    for i, g in enumerate(groups):
        part = grouped[i * (reps + 1):(i + 1) * (reps + 1)]
        if len(part) == reps + 1:
            out["k_kmer_spectrum_groups, %d groups" % g] = spread(part[1:])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--groups", default="2,8")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", action="store_true")
    ap.add_argument("--trace")
    ap.add_argument("--out")
    args = ap.parse_args()
    groups = [int(g) for g in args.groups.split(",") if g]
    if args.trace:
        out = trace_summary(args.trace, groups, args.reps)
        print(json.dumps(out, sort_keys=True))
        if args.out:
            with open(args.out, "w") as f:
                json.dump(out, f, indent=1, sort_keys=True)
                f.write("\n")
        return
    from nanopore_amd import _lib, realign, synth
    from nanopore_amd.hmm import Hmm
    hmm = Hmm.loadHmm(os.path.join(os.path.dirname(os.path.abspath(_lib.__file__)), "mappers", "blasr_hmm_0.txt"))
    w, _ = synth.config_c3(np.asarray(hmm.transitions, dtype=np.float64), np.asarray(hmm.emissions, dtype=np.float64), n_reads=args.reads)
    ctx = realign.Context(0)
    L, ptr = ctx._L, _lib.ptr
    n, nb, k = args.reads, 4 ** args.k + 1, args.k
    read, off = np.ascontiguousarray(w["read"]), np.ascontiguousarray(w["read_off"], dtype=np.int64)
    begin, end = np.ascontiguousarray(off[:-1]), np.ascontiguousarray(off[1:])

    def one_table(seq, seq_off):
        counts = np.zeros(nb, dtype=np.int64)
        rc = L.npr_kmer_counts(ctx._h, k, len(seq_off) - 1, ptr(seq), ptr(seq_off), ptr(counts))
        assert rc == 0, ctx.last_error()
        return counts

    def timed(fn, reps=args.reps):
        ms, res = [], None
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            res = fn()
            if rep:
                ms.append(1e3 * (time.perf_counter() - t0))
        return res, ms

    whole, ms = timed(lambda: one_table(read, off))
    out = {"tool": "tools/kmer_groups_time.py", "reads": n, "k": k, "bases": int(len(read)), "windows": int(whole.sum()),
           "npr_kmer_counts, all bases, one table": spread(ms)}
    for G in groups:
        group = (np.arange(n) % G).astype(np.int32)
        tables, ms = timed(lambda: ctx.kmer_counts_groups(read, begin, end, group, G, k))
        assert tables.sum(axis=0).tolist() == whole.tolist()
        entry = {"npr_kmer_counts_groups": spread(ms)}
        if not args.launches:
            def gather(g):
                mine = np.nonzero(group == g)[0]
                lens = end[mine] - begin[mine]
                sub_off = np.zeros(len(mine) + 1, dtype=np.int64)
                np.cumsum(lens, out=sub_off[1:])
                idx = np.repeat(begin[mine] - sub_off[:-1], lens) + np.arange(int(sub_off[-1]), dtype=np.int64)
                return read[idx], sub_off

            packed = [gather(g) for g in range(G)]
            per_group, ms = timed(lambda: [one_table(*packed[g]) for g in range(G)])
            assert [t.tolist() for t in per_group] == tables.tolist()
            entry["npr_kmer_counts once per group, bases already contiguous"] = spread(ms)
            _, ms = timed(lambda: [one_table(*gather(g)) for g in range(G)], reps=min(args.reps, 3))
            entry["npr_kmer_counts once per group, numpy gather included"] = spread(ms)
        out["%d groups" % G] = entry
    ctx.close()
    print(json.dumps(out, sort_keys=True))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()

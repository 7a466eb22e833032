"""Times the read-quality pass (Context.read_quality: npr_read_quality, csrc/npr_readqual.hip) on one synthetic FASTQ file: N reads of about
8 kb (lognormal lengths), random bases, quality bytes that drift slowly inside a sequencer's range and so cluster per position bin.
  device       the whole call -- staging, H2D, both kernels, all six tables copied back: one warm-up, median of seven wall times
  numpy        the restatement of the definitions the tests use (tests/read_quality_reference.py) on the same file, once
  k-mer pass   Context.kmer_counts at k = 5 on the same reads (one warm-up, median of seven): the yardstick for an LDS-histogram pass over
               the same base bytes; the read-quality pass reads two bytes per base, so the ratio is also given per byte read
Checks that the device's tables equal numpy's, prints the times and records them in profiles/read_quality_time.json.

    python tools/read_quality_time.py [--reads 20000] [--read-len 8000] [--out profiles/read_quality_time.json]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import read_quality_reference as ref  # noqa: E402
from nanopore_amd import ingest  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=20000)
    ap.add_argument("--read-len", type=int, default=8000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "read_quality_time.json"))
    args = ap.parse_args()
    rng = np.random.default_rng(3)
    lengths = np.maximum(1, rng.lognormal(np.log(args.read_len), 0.4, size=args.reads)).astype(np.int64)
    letters = np.frombuffer(b"ACGTACGTACGTACGTACGTN", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        fq = os.path.join(d, "reads.fq")
        with open(fq, "wb") as fh:
            for i, n in enumerate(lengths.tolist()):
                seq = letters[rng.integers(0, len(letters), size=n)].tobytes()
                walk = 12 + np.cumsum(rng.integers(-1, 2, size=n))   # mean quality near 12, as nanopore 2D reads, drifting by one per base
                qual = (33 + np.clip(walk % 24 + rng.integers(0, 4, size=n), 1, 40)).astype(np.uint8).tobytes()
                fh.write(b"@read_%d\n%s\n+\n%s\n" % (i, seq, qual))
        table = ingest.FastqTable(fq)
        ctx = utils._context()
        group = np.zeros(len(table), dtype=np.int32)
        qual_span = table.qual_span
        got, t_dev = _median_ms(lambda: ctx.read_quality(table.text, table.seq_span, qual_span, group, 1))
        seqs = [bytes(table.text[a:b]) for a, b in table.seq_span]
        _, t_kmer = _median_ms(lambda: ctx.kmer_counts(seqs, 5))
        t0 = time.perf_counter()
        want = ref.tables(table.text, table.seq_span, qual_span, group, 1)
        t_numpy = 1e3 * (time.perf_counter() - t0)
        same = all(np.array_equal(a, b) for a, b in zip(got.arrays(), want))
    bases = int(lengths.sum())
    ratio = t_dev["median"] / t_kmer["median"]
    res = dict(reads=args.reads, bases=bases, tables_equal=bool(same), read_quality_ms=t_dev, kmer_counts_k5_ms=t_kmer, numpy_reference_ms=t_numpy,
               ratio_to_kmer_pass=ratio, ratio_to_kmer_pass_per_byte_read=ratio / 2,
               note="wall times of the whole calls, host staging and copies included (one warm-up, medians of seven; numpy once); "
                    "kmer_counts includes joining the Python list of reads into one buffer")
    print("read_quality %.1f ms; kmer_counts k=5 %.1f ms (ratio %.2f, %.2f per byte read); numpy %.0f ms; %d reads, %d bases; tables equal: %s"
          % (t_dev["median"], t_kmer["median"], ratio, ratio / 2, t_numpy, args.reads, bases, same))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not same:
        sys.exit("the device's tables differ from numpy's")


if __name__ == "__main__":
    main()

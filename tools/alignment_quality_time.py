"""Times the two alignment-quality calls (Pileup.coverage: npr_pileup_coverage; Context.align_quality: npr_align_quality; csrc/npr_alnqual.hip) on
one synthetic mapping: a 4.6 Mb contig at ten-fold depth, reads of about 8 kb whose cigars alternate M runs (geometric, mean 8) with I and D runs
of 1 .. 3.
  coverage       the whole call on the filled pileup -- reference bytes up, the running sum, the largest-depth pass, the coverage pass, the
                 tables back: one warm-up, median of seven wall times.  Its bytes/s = rows x 33 B (one table row and one reference byte, what
                 the coverage pass itself reads once) over that time, beside the streaming rate a copy kernel reaches on the part (6.29 TB/s):
                 the call does more than the pass, so the figure is a floor for the pass
  align_quality  the whole call -- packing the cigars, reads, reference and records up, the kernel, the tables back: the same way
  yardstick      Pileup.add_csr + Pileup.depth on the same records into a fresh table (create and destroy outside the clock): the path that
                 existed before and moves the same table; the ratio (coverage + align_quality) / yardstick is recorded
No gate on any number.  Writes profiles/alignment_quality_time.json.

    python tools/alignment_quality_time.py [--contig 4600000] [--depth 10] [--read-len 8000] [--windows 400] [--out profiles/alignment_quality_time.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd.analyses import utils  # noqa: E402

COPY_RATE = 6.29e12  # bytes/s of a float4 copy kernel on one MI355X (79 % of the 8 TB/s the part states)


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def mapping(rng, contig, depth, read_len):
    """-> dict of the arrays Pileup.add_csr and Context.align_quality take, for contig * depth / read_len records"""
    n = max(1, contig * depth // read_len)
    runs = max(1, read_len // 9)                       # M runs per record; an I or D run of 1 .. 3 between two of them
    m = rng.geometric(1.0 / 8.0, size=(n, runs)).astype(np.int32)
    gap_op = rng.integers(1, 3, size=(n, runs - 1)).astype(np.int32)
    gap_len = rng.integers(1, 4, size=(n, runs - 1)).astype(np.int32)
    ops = np.zeros((n, 2 * runs - 1, 2), dtype=np.int32)
    ops[:, 0::2, 1] = m
    ops[:, 1::2, 0], ops[:, 1::2, 1] = gap_op, gap_len
    ref_span = m.sum(axis=1) + np.where(gap_op == 2, gap_len, 0).sum(axis=1)
    read_span = m.sum(axis=1) + np.where(gap_op == 1, gap_len, 0).sum(axis=1)
    assert int(ref_span.max()) < contig
    start = np.zeros((n, 2), dtype=np.int64)
    start[:, 0] = (rng.random(n) * (contig - ref_span)).astype(np.int64)
    read_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(read_span, out=read_off[1:])
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    return dict(read=letters[rng.integers(0, 4, size=int(read_off[-1]))], read_begin=read_off[:-1].copy(), read_end=read_off[1:].copy(),
                ops=ops.reshape(-1, 2), ops_off=np.arange(n + 1, dtype=np.int64) * (2 * runs - 1), ref_index=np.zeros(n, dtype=np.int32), start=start,
                mapq=rng.integers(0, 61, size=n).astype(np.int32), clip=rng.integers(0, 40, size=(n, 2)).astype(np.int64),
                ref_text=letters[rng.integers(0, 4, size=contig)], ref_off=np.array([0, contig], dtype=np.int64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contig", type=int, default=4600000)
    ap.add_argument("--depth", type=int, default=10)
    ap.add_argument("--read-len", type=int, default=8000)
    ap.add_argument("--windows", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alignment_quality_time.json"))
    args = ap.parse_args()
    a = mapping(np.random.default_rng(4), args.contig, args.depth, args.read_len)
    ctx = utils._context()
    records = (a["read"], a["read_begin"], a["read_end"], a["ops"], a["ops_off"], a["ref_index"])

    pileup = ctx.pileup([args.contig])
    pileup.add_csr(*records, start=a["start"])
    coverage, t_cov = _median_ms(lambda: pileup.coverage(a["ref_text"], a["ref_off"], args.windows))
    depth, _ = pileup.depth()
    pileup.close()
    quality, t_qual = _median_ms(lambda: ctx.align_quality(*records, a["mapq"], a["clip"], a["ref_text"], a["ref_off"], start=a["start"], n_windows=args.windows))

    def yardstick():
        t0 = time.perf_counter()
        table.add_csr(*records, start=a["start"])
        out = table.depth()
        return 1e3 * (time.perf_counter() - t0), out

    times = []
    for rep in range(8):  # the first is the warm-up
        table = ctx.pileup([args.contig])
        ms, _ = yardstick()
        table.close()
        times.append(ms)
    t_yard = dict(median=float(np.median(times[1:])), min=min(times[1:]), max=max(times[1:]))

    # what must hold between the calls (the tests compare every count with the restatement on small inputs)
    same = int(coverage.totals[1]) == int(depth.sum()) == int(quality.totals[1]) == int(quality.win_mapq[:, 0].sum()) and \
        np.array_equal(coverage.win[:, 1], quality.win_mapq[:, 0]) and int(quality.totals[0]) == len(a["mapq"]) == int(coverage.totals[5])
    pass_bytes = args.contig * 33
    rate = pass_bytes / (1e-3 * t_cov["median"])
    ratio = (t_cov["median"] + t_qual["median"]) / t_yard["median"]
    res = dict(contig=args.contig, records=len(a["mapq"]), m_columns=int(quality.totals[1]), cigar_runs=int(len(a["ops"])), windows=args.windows, sums_agree=bool(same),
               coverage_ms=t_cov, align_quality_ms=t_qual, add_csr_plus_depth_ms=t_yard, ratio_to_add_csr_plus_depth=ratio,
               coverage_pass_bytes=pass_bytes, coverage_call_bytes_per_s=rate, copy_kernel_bytes_per_s=COPY_RATE, fraction_of_copy_rate=rate / COPY_RATE,
               note="wall times of the whole calls, host staging and copies included (one warm-up, medians of seven); the coverage call also uploads the "
                    "reference, sums the difference array and reduces the largest depth, so its bytes/s is a floor for the coverage pass alone")
    print("coverage %.2f ms (%.3g B/s of the pass's %d bytes, %.1f %% of a copy kernel); align_quality %.1f ms; add_csr + depth %.1f ms; ratio %.2f; sums agree: %s"
          % (t_cov["median"], rate, pass_bytes, 100 * rate / COPY_RATE, t_qual["median"], t_yard["median"], ratio, same))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not same:
        sys.exit("the two calls and the pileup disagree on the M columns")


if __name__ == "__main__":
    main()

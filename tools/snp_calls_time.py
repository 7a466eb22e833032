"""Times the calling step of MarginAlignSnpCaller both ways on one synthetic input: a random contig with 1 % of its bases held out
(analyses/mutate_reference.py), N reads drawn from the true contig through the error channel of blasr_hmm_0 and written as a chained
(global) SAM against the mutated copy.  One hmm type (trained_0) and one sample (all reads), end to end through MarginAlignSnpCaller.run:
  host      callsOnDevice = False: the expectations table fetched, candidate posteriors in numpy, one tuple per call appended to Python lists
  device    callsOnDevice = True: Batch.snp_calls + Pileup.snp_calls (csrc/npr_snpcall.hip), only the histograms leave the device
Both include the same batched DP pass; their difference is the calling step.  Checks that the two XML files are equal, prints both wall
times (each: one warm-up, then the median of three) and records them in profiles/snp_calls_time.json.

    python tools/snp_calls_time.py [--reads 400] [--read-len 5000] [--genome 200000]
"""
import argparse
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd import _lib, bioio, synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.analyses.marginAlignSnpCaller import MarginAlignSnpCaller  # noqa: E402
from nanopore_amd.analyses.mutate_reference import mutateReferenceSequences  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=400)
    ap.add_argument("--read-len", type=int, default=5000)
    ap.add_argument("--genome", type=int, default=200000)
    args = ap.parse_args()
    hmm = Hmm.loadHmm(os.path.join(os.path.dirname(_lib.LIB_PATH), "mappers", "blasr_hmm_0.txt"))
    rng = np.random.default_rng(3)
    genome = rng.integers(0, 4, size=args.genome).astype(np.uint8)
    starts = rng.integers(0, args.genome - args.read_len, size=args.reads)
    off = np.arange(args.reads + 1, dtype=np.int64) * args.read_len
    slices = genome[(starts[:, None] + np.arange(args.read_len)[None, :]).reshape(-1)]
    codes, read_off, cols, col_off = synth.error_channel(rng, slices, off, np.asarray(hmm.transitions, dtype=np.float64), np.asarray(hmm.emissions, dtype=np.float64))
    runs, run_off = synth.columns_to_runs(cols, col_off)
    letters = np.frombuffer(b"ACGT", dtype=np.uint8)
    with tempfile.TemporaryDirectory() as d:
        true_fa, fq, sam = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "mapping.sam")
        bioio.fastaWrite(true_fa, "contig", letters[genome].tobytes().decode())
        fa = mutateReferenceSequences([true_fa], rng=random.Random(3))[1]  # the 1 % copy; its truth file lies next to it
        with open(fq, "w") as fqh, open(sam, "w") as sh:
            sh.write("@SQ\tSN:contig\tLN:%d\n" % args.genome)
            for i in range(args.reads):
                read = letters[codes[read_off[i]:read_off[i + 1]]].tobytes().decode()
                fqh.write("@read_%d\n%s\n+\n%s\n" % (i, read, "I" * len(read)))
                # a chained record is global: the contig before and after the read's interval as deletions
                ops = [(2, int(starts[i]))] + [(int(o), int(n)) for o, n in runs[run_off[i]:run_off[i + 1]]] + [(2, args.genome - int(starts[i]) - args.read_len)]
                cigar = "".join("%d%s" % (n, "MID"[o]) for o, n in ops if n)
                sh.write("\t".join(["read_%d" % i, "0", "contig", "1", "255", cigar, "*", "0", "0", read, "*"]) + "\n")
        ctx = utils._context()
        times, xml = {}, {}
        for name, on_device in (("device", True), ("host", False)):
            laps = []
            for rep in range(4):
                out = os.path.join(d, "%s_%d" % (name, rep))
                os.mkdir(out)
                an = MarginAlignSnpCaller(fq, "2D", fa, sam, out)
                an.hmmTypes, an.coverages, an.callsOnDevice = ("trained_0",), (1000000,), on_device
                t0 = time.perf_counter()
                an.run(ctx=ctx, seed=5)
                if rep:
                    laps.append(1e3 * (time.perf_counter() - t0))
                an.cleanup()
                xml[name] = open(os.path.join(out, "marginaliseConsensus.xml")).read()
            times[name] = dict(median=float(np.median(laps)), min=min(laps), max=max(laps))
    same = xml["device"] == xml["host"]
    res = dict(reads=args.reads, read_bases=int(read_off[-1]), genome=args.genome, hmm_type="trained_0", samples=1, files_equal=bool(same),
               host_ms=times["host"], device_ms=times["device"],
               note="wall times of MarginAlignSnpCaller.run, one hmm type and one sample (median of three after a warm-up); both include the same batched DP pass")
    print("host %.1f ms; device %.1f ms; files equal: %s" % (times["host"]["median"], times["device"]["median"], same))
    with open(os.path.join(ROOT, "profiles", "snp_calls_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not same:
        sys.exit("the two XML files differ")


if __name__ == "__main__":
    main()

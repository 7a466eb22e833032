"""Times the chain step of the seed mapper both ways on one synthetic input: N reads drawn from a random reference through the error channel
of blasr_hmm_0, half of them reverse-complemented, written as FASTQ + FASTA and seeded by SeedMapper (k = 16, min_len = 20, both strands).
  record at a time   utils.chainSamFile on SeedMapper's SAM: parse the records, bucket them, npr_chain_hits + npr_chain_merge per bucket, write
  batched            Context.seed_chains on the hit arrays SeedMapper kept (csrc/npr_seedchain.hip), realign.seed_chain_sam_text, write
Checks that the two files are equal, prints both wall times (the batched one: one warm-up, median of five; its device call and its host
formatter also on their own) and records them in profiles/seed_chain_time.json.

    python tools/seed_chain_time.py [--reads 2000] [--read-len 4000] [--genome 1000000]
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
from nanopore_amd import _lib, realign, synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402
from nanopore_amd.mappers.seedMapper import SeedMapper  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=4000)
    ap.add_argument("--genome", type=int, default=1000000)
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
    with tempfile.TemporaryDirectory() as d:
        fa, fq, sam = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq"), os.path.join(d, "seeds.sam")
        with open(fa, "wb") as fh:
            fh.write(b">genome synthetic\n" + letters[genome].tobytes() + b"\n")
        with open(fq, "wb") as fh:
            for i in range(args.reads):
                seq = text[read_off[i]:read_off[i + 1]].tobytes()
                fh.write(b"@read_%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))
        mapper = SeedMapper(fq, "2D", fa, sam)
        mapper.run()
        fa_t, fq_t, begin, end, hit_off, hits = mapper._seeds
        ctx = utils._context()
        names = [n.encode() for n in fa_t.names]
        t_all, t_dev, t_text = [], [], []
        for rep in range(6):
            t0 = time.perf_counter()
            mapper._writeChainedSam(os.path.join(d, "batched.sam"))
            t1 = time.perf_counter()
            out = ctx.seed_chains(fq_t.lengths, np.diff(fa_t.off), hit_off, hits, mapper.maxGap)
            t2 = time.perf_counter()
            realign.seed_chain_sam_text(fq_t.text, fq_t.name_span, begin, end, names, *out)
            t3 = time.perf_counter()
            if rep:
                t_all.append(1e3 * (t1 - t0)), t_dev.append(1e3 * (t2 - t1)), t_text.append(1e3 * (t3 - t2))
        t0 = time.perf_counter()
        utils.chainSamFile(sam, os.path.join(d, "by_record.sam"), fq, fa)
        t_record = 1e3 * (time.perf_counter() - t0)
        same = open(os.path.join(d, "batched.sam"), "rb").read() == open(os.path.join(d, "by_record.sam"), "rb").read()
        mapper.cleanup()
    res = dict(reads=args.reads, read_bases=int(read_off[-1]), genome=args.genome, k=mapper.k, min_len=mapper.minLength, hits=int(len(hits)), chains=int(len(out[1])),
               op_pairs=int(len(out[3])), files_equal=bool(same), record_at_a_time_ms=t_record,
               batched_ms=dict(median=float(np.median(t_all)), min=min(t_all), max=max(t_all)),
               seed_chains_ms=float(np.median(t_dev)), seed_chain_sam_text_ms=float(np.median(t_text)),
               note="wall times, file to file: utils.chainSamFile on the seed SAM (once) against SeedMapper's chain from the hit arrays (median of five)")
    print("record at a time %.1f ms; batched %.1f ms (seed_chains %.1f ms, seed_chain_sam_text %.1f ms); %d hits, %d chains; files equal: %s"
          % (t_record, res["batched_ms"]["median"], res["seed_chains_ms"], res["seed_chain_sam_text_ms"], res["hits"], res["chains"], same))
    with open(os.path.join(ROOT, "profiles", "seed_chain_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not same:
        sys.exit("the two chained files differ")


if __name__ == "__main__":
    main()

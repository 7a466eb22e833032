"""Times the device-resident seed map against the two calls it stands for, and the fused SeedMapper against the unfused one, on the input of
tools/seed_chain_time.py: N reads drawn from a random reference through the error channel of blasr_hmm_0, half of them reverse-complemented,
written as FASTQ + FASTA (k = 16, min_len = 20, both strands).
  chains and guides   from the ingested tables and a built index: SeedIndex.matches + Context.seed_chains (the rows cross PCIe twice, sorted
                      on the host in between) against SeedIndex.map (csrc/npr_seedmap.hip: the rows stay on the device); arrays compared
  realigned SAM       FASTQ + FASTA -> mapping.sam by SeedMapperRealign.run() with fused off (temp.sam written and parsed back) against on
                      (job.SeedSource); files compared
The timed calls alternate in one process: one warm-up round, then five rounds, median and range of each.  Records profiles/seed_map_time.json.

    python tools/seed_map_time.py [--reads 2000] [--read-len 4000] [--genome 1000000] [--out profiles/seed_map_time.json]
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
from nanopore_amd import _lib, ingest, synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402
from nanopore_amd.mappers import variants  # noqa: E402

ROUNDS = 5


def _stats(ms):
    return dict(median=float(np.median(ms)), min=float(min(ms)), max=float(max(ms)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=2000)
    ap.add_argument("--read-len", type=int, default=4000)
    ap.add_argument("--genome", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seed_map_time.json"))
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
    k, min_len, max_gap = variants.SeedMapper.k, variants.SeedMapper.minLength, variants.SeedMapper.maxGap
    with tempfile.TemporaryDirectory() as d:
        fa, fq = os.path.join(d, "ref.fa"), os.path.join(d, "reads.fq")
        with open(fa, "wb") as fh:
            fh.write(b">genome synthetic\n" + letters[genome].tobytes() + b"\n")
        with open(fq, "wb") as fh:
            for i in range(args.reads):
                seq = text[read_off[i]:read_off[i + 1]].tobytes()
                fh.write(b"@read_%d\n%s\n+\n%s\n" % (i, seq, b"I" * len(seq)))

        # chains and guides from the tables: the two calls against the one
        ctx = utils._context()
        fa_t, fq_t = ingest.FastaTable(fa), ingest.FastqTable(fq)
        begin, end = np.ascontiguousarray(fq_t.seq_span[:, 0]), np.ascontiguousarray(fq_t.seq_span[:, 1])
        index = ctx.seed_index_csr(fa_t.seq, fa_t.off, k)
        t_two, t_map = [], []
        try:
            for rep in range(ROUNDS + 1):
                t0 = time.perf_counter()
                hit_off, hits = index.matches(fq_t.text, begin, end, min_len, 3)
                two = ctx.seed_chains(fq_t.lengths, np.diff(fa_t.off), hit_off, hits, max_gap)
                t1 = time.perf_counter()
                one = index.map(fq_t.text, begin, end, min_len, 3, max_gap)
                t2 = time.perf_counter()
                if rep:
                    t_two.append(1e3 * (t1 - t0)), t_map.append(1e3 * (t2 - t1))
        finally:
            index.close()
        arrays_equal = all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(one, two))

        # FASTQ + FASTA to the realigned SAM, fused off and on
        t_file = {False: [], True: []}
        for rep in range(ROUNDS + 1):
            for fused in (False, True):
                mapper = variants.SeedMapperRealign(fq, "2D", fa, os.path.join(d, "mapping_%d.sam" % fused))
                mapper.fused = fused
                t0 = time.perf_counter()
                mapper.run()
                t1 = time.perf_counter()
                mapper.cleanup()
                if rep:
                    t_file[fused].append(1e3 * (t1 - t0))
        realigned = open(os.path.join(d, "mapping_0.sam"), "rb").read()
        files_equal = realigned == open(os.path.join(d, "mapping_1.sam"), "rb").read()
    res = dict(reads=args.reads, read_bases=int(read_off[-1]), genome=args.genome, k=k, min_len=min_len, max_gap=max_gap, hits=int(len(hits)), chains=int(len(two[1])),
               op_pairs=int(len(two[3])), records=realigned.count(b"\n") - 1, arrays_equal=bool(arrays_equal), files_equal=bool(files_equal),
               matches_plus_seed_chains_ms=_stats(t_two), map_ms=_stats(t_map), realigned_sam_unfused_ms=_stats(t_file[False]),
               realigned_sam_fused_ms=_stats(t_file[True]),
               note="wall times, alternating in one process, one warm-up round then five: tables + index -> chains and guides by the two calls and by "
                    "SeedIndex.map; FASTQ + FASTA -> realigned SAM by SeedMapperRealign.run() with fused off and on")
    print("chains and guides: matches + seed_chains %.1f ms, map %.1f ms; realigned SAM: unfused %.1f ms, fused %.1f ms; %d hits, %d chains; arrays equal: %s, "
          "files equal: %s" % (res["matches_plus_seed_chains_ms"]["median"], res["map_ms"]["median"], res["realigned_sam_unfused_ms"]["median"],
                               res["realigned_sam_fused_ms"]["median"], res["hits"], res["chains"], arrays_equal, files_equal))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not (arrays_equal and files_equal):
        sys.exit("the two paths differ")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Generates the fixtures under tests/golden/pileup/: two seeded sets of SAM records with their reference FASTA, and what
samtools 0.1.19 -- the program the reference calls for its coverage depth and its pileup
(nanopore/metaAnalyses/coverageDepth.py:49-65, analyses/consensus.py) -- prints for them.  No test runs this; the samtools
binary is built elsewhere (`make samtools` in a copy of its source) and is neither committed nor needed by any test.

    python tests/golden/make_pileup_golden.py --samtools /path/to/samtools

Per set x: samtools view -bS x.sam > x.bam; samtools sort x.bam x.sorted; samtools depth x.sorted.bam > x.depth.txt;
samtools mpileup -B -Q 0 -q 0 -d 1000000 x.sorted.bam > x.mpileup.txt.  Kept: x.sam, x.fa, x.depth.txt, x.mpileup.txt.

  local   three contigs (one without a record), 64 records: both strands, soft and hard clips, lowercase and N read bases,
          an I next to a D in both orders, two adjacent I runs, a leading I, a trailing I, flags 4 / 256 / 512 / 1024
          (samtools leaves them out) and 2048 (it keeps them), QUAL present and `*`
  global  records shaped like chainSamFile's output, the shape of every realigned SAM: POS 1, the cigar spans the whole
          contig with leading / trailing D runs and I runs before, between and after them; 32 records on two contigs
"""
import argparse
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pileup")


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[i] for i in rng.integers(0, len(alphabet), size=n))


def body(rng, n_m, m_lo=3, m_hi=40):
    """M runs with an I, a D, an I then a D or a D then an I between them."""
    ops = []
    for j in range(n_m):
        if j:
            gap = int(rng.integers(0, 4))
            i_run, d_run = ("I", int(rng.integers(1, 5))), ("D", int(rng.integers(1, 7)))
            ops += [[i_run], [d_run], [i_run, d_run], [d_run, i_run]][gap]
        ops.append(("M", int(rng.integers(m_lo, m_hi))))
    return ops


def spans(ops):
    ref = sum(n for op, n in ops if op in "MD")
    read = sum(n for op, n in ops if op in "MIS")
    return ref, read


def record(rng, name, contig, pos0, ops, flag=0, mapq=None, qual=None, alphabet="ACGT"):
    _, n = spans(ops)
    seq = rand_seq(rng, n, alphabet)
    mapq = int(rng.integers(0, 61)) if mapq is None else mapq
    with_qual = bool(rng.integers(0, 2)) if qual is None else qual
    q = "".join(chr(33 + int(v)) for v in rng.integers(2, 41, size=n)) if with_qual else "*"
    return "\t".join([name, str(flag), contig, str(pos0 + 1), str(mapq), "".join("%d%s" % (n_, op) for op, n_ in ops), "*", "0", "0", seq, q])


def local_set(rng):
    contigs = [("ctgA", 420), ("ctgB", 310), ("ctgNone", 150)]
    lines = []
    hand = [  # (cigar, flag, alphabet)
        ("2I20M", 0, "ACGT"), ("3S2I25M", 16, "ACGT"),                      # a leading I
        ("20M3I", 0, "ACGT"), ("22M3I4S", 16, "ACGT"),                      # a trailing I
        ("10M2I3D12M", 0, "ACGT"), ("10M3D2I12M", 0, "ACGT"),               # I next to D, both orders
        ("11M2I3D9M4D1I8M", 16, "ACGT"),
        ("10M2I3I10M", 0, "ACGT"),                                          # two adjacent I runs
        ("5H20M5H", 0, "ACGT"), ("5H3S21M2S6H", 16, "ACGT"),                # hard clips
        ("30M", 0, "ACGTacgtN"), ("12M2D14M1I9M", 16, "ACGTacgtNn"),        # lowercase and N read bases
        ("25M", 4, "ACGT"), ("26M", 256, "ACGT"), ("27M", 512, "ACGT"), ("28M", 1024, "ACGT"),  # left out
        ("18M2D9M", 4 | 16, "ACGT"), ("24M", 256 | 16, "ACGT"),
        ("29M", 2048, "ACGT"), ("14M1I15M", 2048 | 16, "ACGT"),             # kept
    ]
    for j, (cigar, flag, alphabet) in enumerate(hand):
        ops, num = [], ""
        for ch in cigar:
            if ch.isdigit():
                num += ch
            else:
                ops.append((ch, int(num)))
                num = ""
        name, length = contigs[j % 2]
        ref, _ = spans(ops)
        pos0 = int(rng.integers(0, length - ref + 1))
        lines.append(record(rng, "hand%02d" % j, name, pos0, ops, flag=flag, alphabet=alphabet, qual=(j % 3 != 0)))
    for j in range(64 - len(hand)):
        name, length = contigs[int(rng.integers(0, 2))]
        ops = body(rng, int(rng.integers(1, 6)))
        if rng.integers(0, 3) == 0:
            ops = [("S", int(rng.integers(1, 9)))] + ops
        if rng.integers(0, 3) == 0:
            ops = ops + [("S", int(rng.integers(1, 9)))]
        if rng.integers(0, 5) == 0:
            ops = [("H", int(rng.integers(1, 9)))] + ops
        ref, _ = spans(ops)
        # the first and the last position of ctgA are covered too
        pos0 = 0 if j == 0 else (length - ref if j == 1 else int(rng.integers(0, length - ref + 1)))
        lines.append(record(rng, "rand%02d" % j, name, pos0, ops, flag=16 * int(rng.integers(0, 2)), alphabet="ACGT" if j % 4 else "ACGTNacgt"))
    return contigs, lines


def global_set(rng):
    contigs = [("chrG", 640), ("chrH", 260)]
    lines = []
    for j in range(32):
        name, length = contigs[0] if j % 4 else contigs[1]
        inner = body(rng, int(rng.integers(2, 7)), 5, 30)
        ref, _ = spans(inner)
        lead = int(rng.integers(0, length - ref + 1)) if j % 7 else 0
        trail = length - ref - lead if j % 5 else 0
        lead = length - ref - trail
        i_run = lambda: ("I", int(rng.integers(1, 6)))  # noqa: E731
        head = [[("D", lead)], [i_run(), ("D", lead)], [("D", lead), i_run()], [i_run(), ("D", lead), i_run()]][int(rng.integers(0, 4))]
        tail = [[("D", trail)], [i_run(), ("D", trail)], [("D", trail), i_run()], [i_run(), ("D", trail), i_run()]][int(rng.integers(0, 4))]
        ops = [o for o in head + inner + tail if o[1] > 0]
        assert spans(ops)[0] == length
        lines.append(record(rng, "chained%02d" % j, name, 0, ops, flag=16 * int(rng.integers(0, 2)), mapq=255 if j % 2 else None,
                            alphabet="ACGT" if j % 3 else "ACGTNacgt"))
    return contigs, lines


def write_set(name, contigs, lines, rng, samtools):
    os.makedirs(OUT, exist_ok=True)
    sam, fa = os.path.join(OUT, name + ".sam"), os.path.join(OUT, name + ".fa")
    with open(fa, "w") as f:
        for cname, length in contigs:
            seq = rand_seq(rng, length)
            f.write(">%s\n" % cname + "".join(seq[i:i + 70] + "\n" for i in range(0, length, 70)))
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.0\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in contigs) + "".join(ln + "\n" for ln in lines))
    with tempfile.TemporaryDirectory() as tmp:
        bam, srt = os.path.join(tmp, "x.bam"), os.path.join(tmp, "x.sorted")
        with open(bam, "wb") as f:
            subprocess.check_call([samtools, "view", "-bS", sam], stdout=f)
        subprocess.check_call([samtools, "sort", bam, srt])
        with open(os.path.join(OUT, name + ".depth.txt"), "wb") as f:
            subprocess.check_call([samtools, "depth", srt + ".bam"], stdout=f)
        with open(os.path.join(OUT, name + ".mpileup.txt"), "wb") as f:
            subprocess.check_call([samtools, "mpileup", "-B", "-Q", "0", "-q", "0", "-d", "1000000", srt + ".bam"], stdout=f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samtools", required=True, help="a samtools 0.1.19 binary")
    args = ap.parse_args()
    rng = np.random.default_rng(20190)
    for name, make in (("local", local_set), ("global", global_set)):
        contigs, lines = make(rng)
        write_set(name, contigs, lines, rng, args.samtools)
        print(name, len(lines), "records", {f: os.path.getsize(os.path.join(OUT, f)) for f in sorted(os.listdir(OUT)) if f.startswith(name)})


if __name__ == "__main__":
    main()

"""Times the device BGZF reader (bam.bgzf_inflate: npr_bgzf_inflate, csrc/npr_inflate.hip) on the two files tools/bam_deflate_time.py makes per
workload (synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig, and one eighth of it): the BAM with stored blocks
and the one the device compressed.  Per file:
  bgzf_inflate    the whole call on the file image in memory -- the block scan on the host, the image up, k_bgzf_inflate, the stream back --:
                  one warm-up, median of seven
  zlib            a fresh raw inflater per block over the same blocks, with the CRC-32 of every payload, on one core: the same
  bam_to_sam      the whole Context.bam_to_sam, file to file (read, inflate, walk, auxiliary text on the host, lines, write): the same
The kernels are not timed on their own (the ABI has no event timing): how the wall times split between kernels and copies is not shown.
Checks that the device's stream is zlib's, prints the figures and records them in profiles/bam_read_time.json.  No threshold.

    python tools/bam_read_time.py [--reads 50000] [--out profiles/bam_read_time.json]
"""
import argparse
import json
import os
import struct
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nanopore_amd import bam, synth  # noqa: E402
from nanopore_amd.analyses import utils  # noqa: E402
from nanopore_amd.hmm import Hmm  # noqa: E402


def _median_ms(fn, reps=7):
    fn()  # warm-up
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        times.append(1e3 * (time.perf_counter() - t0))
    return out, dict(median=float(np.median(times)), min=min(times), max=max(times))


def _zlib(data, block_off):
    out = []
    for at, end in zip(block_off[:-1], block_off[1:]):
        xlen = struct.unpack("<H", data[at + 10:at + 12])[0]
        payload = zlib.decompressobj(-15).decompress(data[at + 12 + xlen:end - 8])
        assert zlib.crc32(payload) == struct.unpack("<I", data[end - 8:end - 4])[0]
        out.append(payload)
    return b"".join(out)


def _one(ctx, path):
    data = open(path, "rb").read()
    image = np.frombuffer(data, np.uint8)
    offs = bam.bgzf_scan(image)
    block_off = [int(v) for v in offs[0]]
    out = np.empty(max(int(offs[1][-1]), 1), np.uint8)
    stream, t_dev = _median_ms(lambda: bam.bgzf_inflate(ctx, image, out=out))
    want, t_zlib = _median_ms(lambda: _zlib(data, block_off))
    counts, t_sam = _median_ms(lambda: ctx.bam_to_sam(path, path + ".sam"))
    return dict(file_bytes=len(data), stream_bytes=len(want), blocks=len(block_off) - 1, same_stream=bool(stream.tobytes() == want), bgzf_inflate_ms=t_dev,
                zlib_one_core_ms=t_zlib, bam_to_sam_ms=t_sam, records=counts["records"], sam_bytes=counts["bytes"])


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "sorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    ctx.sam_to_bam(sam_path, out)
    ctx.sam_to_bam(sam_path, out + ".z", compress=True)
    print("%d reads: both files written" % n_reads, file=sys.stderr, flush=True)
    return dict(reads=n_reads, stored=_one(ctx, out), compressed=_one(ctx, out + ".z"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_read_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times, one warm-up, medians of seven; bgzf_inflate: the whole call on the file image in memory (host scan, H2D, "
                               "k_bgzf_inflate, D2H); zlib: a fresh raw inflater and a CRC-32 per block on one core")
    for r in runs:
        for kind in ("stored", "compressed"):
            f = r[kind]
            print("%d reads, %s: %.0f MB file, %.0f MB stream, %d blocks: bgzf_inflate %.0f ms, zlib on one core %.0f ms; same stream: %s; "
                  "bam_to_sam (file to file, %.0f MB of SAM) %.0f ms"
                  % (r["reads"], kind, f["file_bytes"] / 1e6, f["stream_bytes"] / 1e6, f["blocks"], f["bgzf_inflate_ms"]["median"],
                     f["zlib_one_core_ms"]["median"], f["same_stream"], f["sam_bytes"] / 1e6, f["bam_to_sam_ms"]["median"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r[k]["same_stream"] for r in runs for k in ("stored", "compressed")):
        sys.exit("a stream differs from zlib's")


if __name__ == "__main__":
    main()

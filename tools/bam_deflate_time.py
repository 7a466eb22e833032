"""Times the compressed BAM writer (Context.sam_to_bam(compress=True): npr_sam_bam_deflate, csrc/npr_deflate.hip) against the stored one on
the two workloads of tools/sorted_bam_time.py (synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig, and one eighth
of it).  Per workload:
  file size       stored and compressed
  zlib            levels 1 and 6 over the same uncompressed stream in the same 65 280-byte blocks, raw deflate, on one core: the size (with
                  the 26 bytes of a block's frame and the end-of-file block) and the time, once
  sam_to_bam      the whole call -- mapping and parsing the file, the tag bytes, the device call, both files written -- with and without
                  compress: one warm-up, median of seven
  device part     npr_sam_bam / npr_sam_bam_deflate alone on the parsed file: the same
  chosen          the blocks emitted as (a) dynamic Huffman over matches and literals, (b) over the literals alone, (c) stored
Checks that the compressed file reads back (tests/bgzf_deflate_reference.py) to the stored file's stream, prints the figures and records
them in profiles/bam_deflate_time.json.  No threshold.

    python tools/bam_deflate_time.py [--reads 50000] [--out profiles/bam_deflate_time.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_reference as ref  # noqa: E402
import bgzf_deflate_reference as dref  # noqa: E402
from nanopore_amd import bam, ingest, synth  # noqa: E402
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


def _zlib(stream, level):
    t0 = time.perf_counter()
    size = 28
    for at in range(0, len(stream), ref.P):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        size += 26 + len(z.compress(stream[at:at + ref.P])) + len(z.flush())
    return dict(bytes=size, one_core_ms_once=1e3 * (time.perf_counter() - t0))


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "sorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    _, t_all = _median_ms(lambda: ctx.sam_to_bam(sam_path, out))
    _, t_all_z = _median_ms(lambda: ctx.sam_to_bam(sam_path, out + ".z", compress=True))
    sam = ingest.SamText(sam_path)
    fields = sam.parse()
    tail = bam.parse_tail(sam, fields)
    tag_off, tags = bam.bam_tags(sam.text, tail)
    header, ref_len = bam.bam_header(sam.header, True)
    (image, _), t_dev = _median_ms(lambda: bam.convert(ctx, sam, fields, tail, tag_off, tags, header, ref_len))
    (image_z, _), t_dev_z = _median_ms(lambda: bam.convert(ctx, sam, fields, tail, tag_off, tags, header, ref_len, compress=True))
    chosen = bam.deflate_last(ctx)
    stream, _ = ref.bgzf_read(image.tobytes())
    stream_z, blocks = dref.bgzf_read(image_z.tobytes())
    ok = stream_z == stream and image_z.tobytes() == open(out + ".z", "rb").read() and chosen["stream_bytes"] == len(stream)
    ok = ok and chosen["a"] + chosen["b"] + chosen["c"] == len(blocks)
    print("%d reads: converted and read back; zlib next" % n_reads, file=sys.stderr, flush=True)
    return dict(reads=n_reads, sam_bytes=int(len(sam.text)), stream_bytes=len(stream), bam_bytes_stored=int(len(image)), bam_bytes_compressed=int(len(image_z)),
                zlib_level_1=_zlib(stream, 1), zlib_level_6=_zlib(stream, 6), reads_back=bool(ok), chosen={k: chosen[k] for k in "abc"},
                sam_to_bam_ms=t_all, sam_to_bam_compress_ms=t_all_z, device_part_ms=t_dev, device_part_compress_ms=t_dev_z)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bam_deflate_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times (one warm-up, medians of seven; zlib once, on one core, in the same 65 280-byte blocks); sam_to_bam includes "
                               "parsing and writing both files; chosen: blocks emitted as (a) dynamic Huffman over matches and literals, (b) over "
                               "literals alone, (c) stored")
    for r in runs:
        print("%d reads, %.0f MB SAM, %.0f MB stream: stored %.0f MB, compressed %.0f MB (zlib -1 %.0f MB in %.0f ms, -6 %.0f MB in %.0f ms); sam_to_bam %.0f ms, "
              "compressed %.0f ms; device part %.0f ms, compressed %.0f ms; chosen %s; reads back: %s"
              % (r["reads"], r["sam_bytes"] / 1e6, r["stream_bytes"] / 1e6, r["bam_bytes_stored"] / 1e6, r["bam_bytes_compressed"] / 1e6,
                 r["zlib_level_1"]["bytes"] / 1e6, r["zlib_level_1"]["one_core_ms_once"], r["zlib_level_6"]["bytes"] / 1e6, r["zlib_level_6"]["one_core_ms_once"],
                 r["sam_to_bam_ms"]["median"], r["sam_to_bam_compress_ms"]["median"], r["device_part_ms"]["median"], r["device_part_compress_ms"]["median"],
                 r["chosen"], r["reads_back"]), flush=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r["reads_back"] for r in runs):
        sys.exit("a file did not read back")


if __name__ == "__main__":
    main()

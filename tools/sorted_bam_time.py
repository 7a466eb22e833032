"""Times the SAM -> sorted BAM + BAI conversion (Context.sam_to_bam: npr_sam_bam, csrc/npr_bam.hip) on a synthetic SAM file of the c3 shape
(synth.config_c3_shared: ~8 kb lognormal reads on one E. coli-sized contig) and on one eighth of it.
  sam_to_bam     the whole call -- mapping and parsing the file, the tag bytes, the device call, both files written: one warm-up, median of seven
  device part    npr_sam_bam alone (upload, sort, encode, frame, index, download) on the parsed file: the same
  zlib.crc32     over the same uncompressed stream on one core, in the same process: what the checksum alone costs a host writer
  realignSamFile the realignment of the same records (analyses/utils.realignSamFile, blasr_hmm_0): the job that made such a file
Checks that the file reads back (tests/bam_reference.py) with the records in key order, prints the times and records them in
profiles/sorted_bam_time.json.  No threshold.

    python tools/sorted_bam_time.py [--reads 50000] [--out profiles/sorted_bam_time.json]
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


def measure(ctx, hmm_file, n_reads, d):
    h = Hmm.loadHmm(hmm_file)
    w, _ = synth.config_c3_shared(h.transitions, h.emissions, n_reads=n_reads)
    sam_path, fa, fq, out = (os.path.join(d, "%d.%s" % (n_reads, e)) for e in ("sam", "fa", "fq", "sorted.bam"))
    synth.write_workload_files(w, sam_path, fa, fastq_path=fq, ref_names=["ecoli_like_contig"])
    _, t_all = _median_ms(lambda: ctx.sam_to_bam(sam_path, out))
    sam = ingest.SamText(sam_path)
    fields = sam.parse()
    tail = bam.parse_tail(sam, fields)
    tag_off, tags = bam.bam_tags(sam.text, tail)
    header, ref_len = bam.bam_header(sam.header, True)
    (image, _), t_dev = _median_ms(lambda: bam.convert(ctx, sam, fields, tail, tag_off, tags, header, ref_len))
    stream, _ = ref.bgzf_read(image.tobytes())
    pos = fields[:, 8]
    ok = image.tobytes() == open(out, "rb").read() and len(stream) > len(sam.text) // 2
    if n_reads <= 8192:   # (the Python decoder takes a minute per 10^5 records)
        records = ref.bam_decode(stream)[2]
        ok = ok and [r["pos"] for r in records] == sorted(pos.tolist()) and len(records) == len(sam)
    _, t_crc = _median_ms(lambda: zlib.crc32(stream))
    t0 = time.perf_counter()
    utils.realignSamFile(sam_path, os.path.join(d, "realigned.sam"), fq, fa, hmm_file, 0.5, 0.0, ctx=ctx)
    t_realign = 1e3 * (time.perf_counter() - t0)
    return dict(reads=n_reads, sam_bytes=int(len(sam.text)), bam_bytes=int(len(image)), reads_back=bool(ok), sam_to_bam_ms=t_all, device_part_ms=t_dev,
                zlib_crc32_one_core_ms=t_crc, realignSamFile_ms_once=t_realign)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sorted_bam_time.json"))
    args = ap.parse_args()
    hmm_file = os.path.join(ROOT, "nanopore_amd", "mappers", "blasr_hmm_0.txt")
    ctx = utils._context()
    with tempfile.TemporaryDirectory() as d:
        runs = [measure(ctx, hmm_file, n, d) for n in (max(1, args.reads // 8), args.reads)]
    res = dict(runs=runs, note="wall times (one warm-up, medians of seven; realignSamFile once); sam_to_bam includes parsing and writing both files; "
                               "the BAM is BGZF with stored blocks: about the size of the uncompressed stream")
    for r in runs:
        print("%d reads, %.0f MB SAM: sam_to_bam %.0f ms, device part %.0f ms; zlib.crc32 of the stream on one core %.0f ms; realignSamFile %.0f ms; reads back: %s"
              % (r["reads"], r["sam_bytes"] / 1e6, r["sam_to_bam_ms"]["median"], r["device_part_ms"]["median"], r["zlib_crc32_one_core_ms"]["median"],
                 r["realignSamFile_ms_once"], r["reads_back"]))
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    if not all(r["reads_back"] for r in runs):
        sys.exit("a file did not read back")


if __name__ == "__main__":
    main()

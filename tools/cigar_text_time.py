"""Times the tail of the gather on bench.py's default workload: the cigars of a finished batch as packed words (the default) against SAM text
made on the device (NPR_OPT_FINISH_TEXT, csrc/npr_cigtext.hip), each with the splice of the batch's SAM records that follows it.

    python tools/cigar_text_time.py [--reads 24576,6250] [--threads 2,16] [--reps 7] [--out profiles/cigar_text_time.json]

Per batch size and NPR_HOST_THREADS, one warm-up and then `reps` repetitions, the two paths alternating:
  words  npr_batch_finish with the option at 0 -- its lap "gather + D2H of the ops" (NPR_TIMING=1, read back from stderr) --, then the fetch of
         the words (npr_batch_ops_packed) and npr_sam_splice;
  text   the same with the option at 1 (the lap is then gather + text kernels + D2H of the text), npr_batch_cigar_text and npr_sam_splice_text.
The outputs of the two are compared byte for byte before anything is timed.  Medians, minima and maxima in ms; the bytes that cross PCIe in
both forms.  `--kernels-only`: three finishes with the option at 1 and nothing else, the target of `tools/kstats.sh` (rocprofv3 --kernel-trace
--stats, in a run of its own); `--kernel-stats CSV` then adds the k_cigtext_* rows of that table to the JSON that is there already.
"""
import argparse
import csv
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from nanopore_amd import _lib, ingest, realign  # noqa: E402

HBM_ACHIEVABLE_TBS = 6.3  # streaming rate an MI355X reaches (8 TB/s peak)
LAP = re.compile(r"device_mea / gather \+ D2H of the ops: ([0-9.]+) ms")


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": statistics.median(ms), "min_ms": ms[0], "max_ms": ms[-1], "reps": len(ms)}


def finish_lap(b, log):
    """b.finish() with the library's stage times (stderr) going to `log`: -> ms of the gather lap"""
    sys.stderr.flush()
    at = os.lseek(log, 0, os.SEEK_END)
    keep = os.dup(2)
    os.dup2(log, 2)
    try:
        b.finish()
    finally:
        os.dup2(keep, 2)
        os.close(keep)
    m = LAP.findall(os.pread(log, 1 << 20, at).decode(errors="replace"))
    if len(m) != 1:
        raise SystemExit("no 'gather + D2H of the ops' lap: the batch did not take the device MEA stage")
    return float(m[0])


def sam_of(w, path):
    """The workload's records as a SAM text (no FASTA: nothing here reads the references)."""
    n = len(w["read_off"]) - 1
    names = ["ref_%d" % k for k in range(len(w["ref_off"]) - 1)]
    g = np.asarray(w["guide_ops"], dtype=np.int64).reshape(-1, 2)
    goff = np.asarray(w["guide_off"], dtype=np.int64)
    ri = w.get("ref_index")
    gs = w.get("guide_start")
    buf, _ = realign.format_sam_records([b"read_%d" % i for i in range(n)], [s.encode() for s in names],
                                        np.asarray(ri, dtype=np.int32) if ri is not None else np.arange(n, dtype=np.int32),
                                        (np.asarray(gs, dtype=np.int64)[:, 0] if gs is not None else np.zeros(n, dtype=np.int64)) + 1, goff[:-1],
                                        np.diff(goff), ((g[:, 1] << 2) | g[:, 0]).astype(np.uint32), np.ascontiguousarray(w["read"], dtype=np.uint8),
                                        np.asarray(w["read_off"], dtype=np.int64))
    with open(path, "wb") as fh:
        fh.write(b"@HD\tVN:1.0\tSO:unsorted\n")
        for k, s in enumerate(names):
            fh.write(("@SQ\tSN:%s\tLN:%d\n" % (s, int(w["ref_off"][k + 1] - w["ref_off"][k]))).encode())
        fh.write(memoryview(buf))


def staged(ctx, w, W):
    b = ctx.stage_csr(bench.make_params(W), w["ref"], w["ref_off"], w["read"], w["read_off"], w["guide_ops"], w["guide_off"],
                      guide_start=w.get("guide_start"), ref_index=w.get("ref_index"))
    b.run()
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", default="24576,6250")
    ap.add_argument("--threads", default="2,16")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cigar_text_time.json"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--kernel-stats")
    args = ap.parse_args()

    if args.kernel_stats:
        out = json.load(open(args.out))
        rows = {re.search(r"k_cigtext_\w+", r["Name"]).group(0): r for r in csv.DictReader(open(args.kernel_stats)) if "k_cigtext_" in r["Name"]}
        big = out["batches"][0]
        k = {name: {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3, "max_us": float(r["MaxNs"]) / 1e3}
             for name, r in sorted(rows.items())}
        wr = k["k_cigtext_write"]["mean_us"]
        every = sum(v["mean_us"] for v in k.values())
        out["kernels"] = {"reads": big["reads"], "source": "rocprofv3 --kernel-trace --stats, a run of its own (tools/kstats.sh)", "per_kernel": k,
                          "all_five_us": every, "text_bytes": big["text_bytes"], "words_read_bytes": 4 * big["ops"],
                          "write_pass_text_bytes_per_s": big["text_bytes"] / (wr * 1e-6),
                          "write_pass_read_plus_written_bytes_per_s": (big["text_bytes"] + 4 * big["ops"]) / (wr * 1e-6),
                          "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE_TBS * 1e12}
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print(json.dumps(out["kernels"], sort_keys=True))
        return

    os.environ["NPR_TIMING"] = "1"
    sizes = [int(x) for x in args.reads.split(",")]
    if args.kernels_only:
        h, w, W, _ = bench.build_workload("northstar", sizes[0], 0)
        ctx = realign.Context(0)
        ctx.set_hmm(h)
        ctx.set_option(_lib.OPT_FINISH_TEXT, 1)
        b = staged(ctx, w, W)
        for _ in range(3):
            b.finish()
        print("text bytes", int(b.cigar_text()[1][-1]))
        b.close(), ctx.close()
        return

    out = {"tool": "tools/cigar_text_time.py", "batches": [], "hbm_achievable_bytes_per_s": HBM_ACHIEVABLE_TBS * 1e12}
    log = os.open(os.path.join(tempfile.gettempdir(), "cigar_text_time.%d.log" % os.getpid()), os.O_RDWR | os.O_CREAT | os.O_TRUNC, 0o600)
    for n in sizes:
        h, w, W, label = bench.build_workload("northstar", n, 0)
        with tempfile.TemporaryDirectory() as tmp:
            sam_of(w, os.path.join(tmp, "reads.sam"))
            st = ingest.SamText(os.path.join(tmp, "reads.sam"))
            fields, span = st.parse(), np.ascontiguousarray(st.span)
            assert len(fields) == n and (fields[:, ingest.F_STATUS] == 0).all()
            entry = {"reads": n, "workload": label, "threads": {}}
            for threads in [int(x) for x in args.threads.split(",")]:
                os.environ["NPR_HOST_THREADS"] = str(threads)
                ctx = realign.Context(0)  # (a context takes its host threads when it is made)
                ctx.set_hmm(h)
                b = staged(ctx, w, W)
                words_buf = text_buf = None
                pool = {}

                def take(nbytes, key):  # (one record buffer per path, kept over the repetitions as the job's pool keeps its own)
                    if key not in pool or pool[key].nbytes < nbytes:
                        pool[key] = np.empty(nbytes + nbytes // 8, dtype=np.uint8)
                    return pool[key]
                t = {k: [] for k in ("words_lap", "words_fetch", "words_splice", "text_lap", "text_fetch", "text_splice")}
                for rep in range(args.reps + 1):
                    ctx.set_option(_lib.OPT_FINISH_TEXT, 0)
                    lap0 = finish_lap(b, log)
                    t0 = time.perf_counter()
                    off, words, words_buf = b.ops_packed_into(words_buf)
                    t1 = time.perf_counter()
                    rec0 = st.splice(span, fields, off[:-1], np.diff(off), words, take=lambda nb: take(nb, "w"))
                    t2 = time.perf_counter()
                    ctx.set_option(_lib.OPT_FINISH_TEXT, 1)
                    lap1 = finish_lap(b, log)
                    t3 = time.perf_counter()
                    text, str_off = b.cigar_text(text_buf)
                    text_buf = text.base if text.base is not None else text
                    t4 = time.perf_counter()
                    rec1 = st.splice_text(span, fields, str_off, text, take=lambda nb: take(nb, "t"))
                    t5 = time.perf_counter()
                    if rep == 0:
                        assert np.array_equal(rec0, rec1), "the two paths write different records"
                        res = b.results()
                        entry.update(ops=int(off[-1]), text_bytes=int(str_off[-1]), record_bytes=int(len(rec0)), failed_reads=int((res["status"] != 0).sum()),
                                     longest_run=int((words >> 2).max()))
                        continue
                    for k, v in zip(("words_lap", "words_fetch", "words_splice", "text_lap", "text_fetch", "text_splice"),
                                    (lap0, 1e3 * (t1 - t0), 1e3 * (t2 - t1), lap1, 1e3 * (t4 - t3), 1e3 * (t5 - t4))):
                        t[k].append(v)
                e = {k: spread(v) for k, v in t.items()}
                for path in ("words", "text"):
                    e[path + "_lap_plus_splice"] = spread([a + c for a, c in zip(t[path + "_lap"], t[path + "_splice"])])
                    e[path + "_lap_fetch_splice"] = spread([a + f + c for a, f, c in zip(t[path + "_lap"], t[path + "_fetch"], t[path + "_splice"])])
                base = e["words_lap_plus_splice"]
                e["baseline_spread_ms"] = base["max_ms"] - base["min_ms"]
                e["text_minus_words_median_ms"] = e["text_lap_plus_splice"]["median_ms"] - base["median_ms"]
                entry["threads"][str(threads)] = e
                b.close(), ctx.close()
            narrow = entry["longest_run"] < (1 << 14)
            entry["pcie_bytes"] = {"text": entry["text_bytes"] + 8 * (n + 1), "words_2_byte": 2 * entry["ops"], "words_4_byte": 4 * entry["ops"],
                                   "default_path_sends": "words_2_byte" if narrow else "words_4_byte"}
            out["batches"].append(entry)
            del st
    os.close(log)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()

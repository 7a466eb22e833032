"""The definitions of npr_read_quality (include/nprealign.h) in numpy: np.add.at over a vectorised bin(p), integer arithmetic only.
The oracle of tests/test_read_quality_host.py and tests/test_gpu_read_quality.py."""
import numpy as np

POS_BINS, QUAL_COLS, GC_COLS, TOTALS = 336, 95, 102, 8


def pos_bin(p):
    """bin(p) for an int64 array of positions."""
    p = np.asarray(p, dtype=np.int64)
    q = np.maximum(p, 16)
    e = np.zeros(p.shape, dtype=np.int64)
    for k in range(1, 63):  # floor(log2 q) without floating point
        e += (q >> k) > 0
    b = 16 * (e - 3) + ((q >> (e - 4)) & 15)
    return np.where(p < 16, p, np.where(p >= 1 << 24, POS_BINS - 1, b))


_CODE = np.full(256, 4, dtype=np.int64)
for _i, _ch in enumerate("ACGT"):
    _CODE[ord(_ch)] = _CODE[ord(_ch.lower())] = _i


def tables(text, seq_span, qual_span, group, n_groups):
    """The six tables, first axis = group, for reads given as spans in `text` (uint8): (pos_qual, pos_base, len_hist, meanq_hist,
    gc_hist, totals), int64."""
    text = np.asarray(text, dtype=np.uint8)
    seq_span, qual_span = np.asarray(seq_span, dtype=np.int64).reshape(-1, 2), np.asarray(qual_span, dtype=np.int64).reshape(-1, 2)
    pos_qual = np.zeros((n_groups, POS_BINS, QUAL_COLS), dtype=np.int64)
    pos_base = np.zeros((n_groups, POS_BINS, 5), dtype=np.int64)
    len_hist = np.zeros((n_groups, POS_BINS), dtype=np.int64)
    meanq_hist = np.zeros((n_groups, QUAL_COLS), dtype=np.int64)
    gc_hist = np.zeros((n_groups, GC_COLS), dtype=np.int64)
    totals = np.zeros((n_groups, TOTALS), dtype=np.int64)
    totals[:, 2:6] = -1
    for (sa, sb), (qa, qb), g in zip(seq_span.tolist(), qual_span.tolist(), np.asarray(group).tolist()):
        if g < 0:
            continue
        n = sb - sa
        assert qb - qa == n
        t = totals[g]
        t[0] += 1
        t[1] += n
        t[2] = n if t[2] < 0 else min(t[2], n)
        t[3] = max(t[3], n)
        len_hist[g, pos_bin(n)] += 1
        if n == 0:
            t[6] += 1
            continue
        q, code = text[qa:qb].astype(np.int64), _CODE[text[sa:sb]]
        ok = (q >= 33) & (q <= 126)
        bins = pos_bin(np.arange(n, dtype=np.int64))
        np.add.at(pos_qual[g], (bins, np.where(ok, q - 33, QUAL_COLS - 1)), 1)
        np.add.at(pos_base[g], (bins, code), 1)
        t[4] = int(q.min()) if t[4] < 0 else min(t[4], int(q.min()))
        t[5] = max(t[5], int(q.max()))
        if ok.all():
            meanq_hist[g, int((q - 33).sum()) // n] += 1
        else:
            meanq_hist[g, QUAL_COLS - 1] += 1
            t[7] += 1
        acgt, gc = int((code < 4).sum()), int(((code == 1) | (code == 2)).sum())
        gc_hist[g, (200 * gc + acgt) // (2 * acgt) if acgt else GC_COLS - 1] += 1
    return pos_qual, pos_base, len_hist, meanq_hist, gc_hist, totals


def fastq_text(reads):
    """[(bases, quality)] (bytes) as FASTQ text -> (uint8 text, seq spans [n, 2], quality spans [n, 2])."""
    parts, seq, qual, at = [], [], [], 0
    for i, (s, q) in enumerate(reads):
        head = b"@r%d\n" % i
        seq.append((at + len(head), at + len(head) + len(s)))
        qa = seq[-1][1] + 3
        qual.append((qa, qa + len(q)))
        parts.append(head + s + b"\n+\n" + q + b"\n")
        at += len(parts[-1])
    return (np.frombuffer(b"".join(parts), dtype=np.uint8), np.array(seq, dtype=np.int64).reshape(-1, 2),
            np.array(qual, dtype=np.int64).reshape(-1, 2))

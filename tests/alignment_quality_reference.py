"""The definitions of npr_pileup_coverage and npr_align_quality (include/nprealign.h) restated in plain Python / numpy, one row, one
record, one position at a time, integer arithmetic only.  Written from the header's text; shares no code with the kernels.
The oracle of tests/test_alignment_quality_host.py and tests/test_gpu_alignment_quality.py."""
import numpy as np

POS_BINS, GC_COLS, WIN_WORDS, TOTALS, HOMOPOLYMER, MAX_WINDOWS = 336, 102, 8, 8, 3, 65536
ERR_INVALID, ERR_CAPACITY = -1, -3
OP_M, OP_I, OP_D = 0, 1, 2


def pos_bin(v):
    """bin(v) of one non-negative integer: exact below 16, then sixteen per octave, 335 from 2^24 on."""
    if v < 16:
        return v
    if v >= 1 << 24:
        return POS_BINS - 1
    e = v.bit_length() - 1
    return 16 * (e - 3) + ((v >> (e - 4)) & 15)


def code(ch):
    """base code of one byte (an int)"""
    return "ACGT".find(chr(ch).upper()) if chr(ch).upper() in "ACGT" else 4


def window_of_row(r, T, W):
    return ((r + 1) * W - 1) // T


def window_rows(w, T, W):
    """[lo, hi) of window w"""
    return w * T // W, (w + 1) * T // W


def longest_window(T, W):
    return max(hi - lo for lo, hi in (window_rows(w, T, W) for w in range(W)))


def capacity_refuses(largest_depth, T, W):
    """the NPR_ERR_CAPACITY rule"""
    return largest_depth * largest_depth * longest_window(T, W) >= 1 << 63


def coverage(table, ref, W):
    """table: [T][8] counts as npr_pileup_counts returns them; ref: the T reference bytes, sequences back to back.
    -> (win [W][8], depth_hist [336], start_hist [336], totals [8]) int64, or ERR_INVALID / ERR_CAPACITY."""
    if not 1 <= W <= MAX_WINDOWS:
        return ERR_INVALID
    table = np.asarray(table, dtype=np.int64).reshape(-1, 8)
    T = len(table)
    assert len(ref) == T
    depth = [int(v) for v in table[:, :5].sum(axis=1)]
    if T and capacity_refuses(max(depth), T, W):
        return ERR_CAPACITY
    win = [[0] * WIN_WORDS for _ in range(W)]
    depth_hist, start_hist, totals = [0] * POS_BINS, [0] * POS_BINS, [0] * TOTALS
    for r in range(T):
        d, dels, ins, starts = depth[r], int(table[r, 5]), int(table[r, 6]), int(table[r, 7])
        c = code(ref[r])
        w = win[window_of_row(r, T, W)]
        w[0] += 1
        w[1] += d
        w[2] += d * d
        w[3] += d >= 1
        w[4] += c in (1, 2)
        w[5] += c < 4
        w[6] += starts
        w[7] += dels
        depth_hist[pos_bin(d)] += 1
        start_hist[pos_bin(starts)] += 1
        totals[0] += 1
        totals[1] += d
        totals[2] = max(totals[2], d)
        totals[3] += d >= 1
        totals[4] = max(totals[4], starts)
        totals[5] += starts
        totals[6] += dels
        totals[7] += ins
    return tuple(np.array(x, dtype=np.int64) for x in (win, depth_hist, start_hist, totals))


def record(ref_index, read, cigar, mapq=0, clip=(0, 0), start=(0, 0), use=True):
    """One record: read = the bytes read[read_begin:read_end], cigar = [(op, length)], start = (reference position, read position)."""
    return dict(ref_index=ref_index, read=read.encode() if isinstance(read, str) else bytes(read), cigar=list(cigar), mapq=mapq, clip=tuple(clip),
                start=tuple(start), use=use)


def record_is_valid(rec, refs):
    k, (sx, sy) = rec["ref_index"], rec["start"]
    if not 0 <= k < len(refs) or sx < 0 or sy < 0 or sy > len(rec["read"]) or sx > len(refs[k]):
        return False
    if not 0 <= rec["mapq"] <= 255 or rec["clip"][0] < 0 or rec["clip"][1] < 0:
        return False
    if any(op not in (OP_M, OP_I, OP_D) or n < 0 for op, n in rec["cigar"]):
        return False
    x = sx + sum(n for op, n in rec["cigar"] if op != OP_I)
    y = sy + sum(n for op, n in rec["cigar"] if op != OP_D)
    return x <= len(refs[k]) and y <= len(rec["read"])


def _side(seq, positions, b):
    """how many of `positions` in a row, from the first on, hold code b inside seq -- at most HOMOPOLYMER"""
    n = 0
    for q in positions:
        if n == HOMOPOLYMER or not 0 <= q < len(seq) or code(seq[q]) != b:
            break
        n += 1
    return n


def indel_class(seq, x, run_codes, deletion):
    """seq: the record's own reference sequence, x: position in it of the next column at the run, run_codes: the codes of the inserted read
    bases / deleted reference bases"""
    b = run_codes[0]
    if b >= 4 or any(c != b for c in run_codes):
        return 4
    n = len(run_codes)
    left = _side(seq, range(x - 1, x - 1 - HOMOPOLYMER, -1), b)
    right = _side(seq, range(x + n, x + n + HOMOPOLYMER) if deletion else range(x, x + HOMOPOLYMER), b)
    return b if left + (n if deletion else 0) + right >= HOMOPOLYMER else 4


def quality(records, refs, W):
    """records: what record() makes; refs: the reference sequences (bytes).  -> ((mapq_hist, win_mapq, pos_base, clip_hist, gc_hist, indel,
    indel_len, totals), invalid) or ERR_INVALID for what the host refuses."""
    if not 1 <= W <= MAX_WINDOWS:
        return ERR_INVALID
    refs = [r.encode() if isinstance(r, str) else bytes(r) for r in refs]
    first = [0]
    for r in refs:
        first.append(first[-1] + len(r))
    T = first[-1]
    mapq_hist, win_mapq = [0] * 256, [[0, 0] for _ in range(W)]
    pos_base, clip_hist, gc_hist = [[0] * 5 for _ in range(POS_BINS)], [0] * POS_BINS, [0] * GC_COLS
    indel, indel_len, totals = [[0] * 5 for _ in range(2)], [[0] * POS_BINS for _ in range(2)], [0] * TOTALS
    invalid = False
    for rec in records:
        if not rec["use"]:
            continue
        if not record_is_valid(rec, refs):
            invalid = True
            continue
        seq, read, q, (c0, c1), (x, y) = refs[rec["ref_index"]], rec["read"], rec["mapq"], rec["clip"], rec["start"]
        row0 = first[rec["ref_index"]]
        mapq_hist[q] += 1
        totals[0] += 1
        totals[6] += c0 + c1
        totals[7] += c0 + c1 > 0
        for p in list(range(c0)) + list(range(c0 + len(read), c0 + len(read) + c1)):
            clip_hist[pos_bin(p)] += 1
        if len(read):
            codes = [code(ch) for ch in read]
            acgt, gc = sum(c < 4 for c in codes), sum(c in (1, 2) for c in codes)
            gc_hist[(200 * gc + acgt) // (2 * acgt) if acgt else GC_COLS - 1] += 1
        for op, n in rec["cigar"]:
            if n == 0:
                continue
            if op == OP_M:
                totals[1] += n
                for j in range(n):
                    w = win_mapq[window_of_row(row0 + x + j, T, W)]
                    w[0] += 1
                    w[1] += q
            else:
                run = [code(ch) for ch in (read[y:y + n] if op == OP_I else seq[x:x + n])]
                kind = 0 if op == OP_I else 1
                indel[kind][indel_class(seq, x, run, op == OP_D)] += 1
                indel_len[kind][pos_bin(n)] += 1
                totals[2 + 2 * kind] += 1
                totals[3 + 2 * kind] += n
            if op != OP_D:
                for j in range(n):
                    pos_base[pos_bin(c0 + y + j)][code(read[y + j])] += 1
                y += n
            if op != OP_I:
                x += n
    return tuple(np.array(t, dtype=np.int64) for t in (mapq_hist, win_mapq, pos_base, clip_hist, gc_hist, indel, indel_len, totals)), invalid


def fasta_sequences(text):
    """{name: bytes} of FASTA text (name = first word of the header)"""
    out, name = {}, None
    for line in text.split("\n"):
        if line.startswith(">"):
            name = line[1:].split()[0]
            out[name] = b""
        elif name is not None:
            out[name] += line.strip().encode()
    return out


def records_of_sam(sam_text, dropped_flags=0x4 | 0x100 | 0x200 | 0x400):
    """(names, records) of SAM text: the records samtools' pileup keeps (flag mask, RNAME not "*"), read = SEQ without its soft clips,
    clip = the S operations at either end, start = (POS - 1, 0), MAPQ as stated."""
    names, records = [], []
    for line in sam_text.split("\n"):
        if line.startswith("@SQ"):
            names.append(dict(f.split(":", 1) for f in line.split("\t")[1:])["SN"])
        if not line or line.startswith("@"):
            continue
        f = line.split("\t")
        if int(f[1]) & dropped_flags or f[2] == "*":
            continue
        runs, num = [], ""
        for ch in f[5]:
            if ch.isdigit():
                num += ch
            else:
                runs.append((ch, int(num)))
                num = ""
        runs = [r for r in runs if r[0] != "H"]
        c0 = runs[0][1] if runs and runs[0][0] == "S" else 0
        c1 = runs[-1][1] if len(runs) > 1 and runs[-1][0] == "S" else 0
        cigar = [("MID".index(ch), n) for ch, n in runs if ch != "S"]
        records.append(record(names.index(f[2]), f[9][c0:len(f[9]) - c1], cigar, mapq=int(f[4]), clip=(c0, c1), start=(int(f[3]) - 1, 0)))
    return names, records


def arrays_of(records, refs):
    """The records as the entry points take them: dict(read, read_begin, read_end, ops, ops_off, ref_index, start, use, mapq, clip, ref_text,
    ref_off).  The reads are laid out with a gap byte between them so that read_end matters."""
    refs = [r.encode() if isinstance(r, str) else bytes(r) for r in refs]
    ref_off = np.zeros(len(refs) + 1, dtype=np.int64)
    np.cumsum([len(r) for r in refs], out=ref_off[1:])
    text, begin, end, ops, ops_off = b"", [], [], [], [0]
    for rec in records:
        begin.append(len(text))
        text += rec["read"]
        end.append(len(text))
        text += b"#"
        ops.extend(rec["cigar"])
        ops_off.append(len(ops))
    return dict(read=np.frombuffer(text or b"#", dtype=np.uint8), read_begin=np.array(begin, dtype=np.int64), read_end=np.array(end, dtype=np.int64),
                ops=np.array(ops, dtype=np.int32).reshape(-1, 2), ops_off=np.array(ops_off, dtype=np.int64),
                ref_index=np.array([r["ref_index"] for r in records], dtype=np.int32), start=np.array([r["start"] for r in records], dtype=np.int64).reshape(-1, 2),
                use=np.array([r["use"] for r in records], dtype=np.uint8), mapq=np.array([r["mapq"] for r in records], dtype=np.int32),
                clip=np.array([r["clip"] for r in records], dtype=np.int64).reshape(-1, 2),
                ref_text=np.frombuffer(b"".join(refs) or b"#", dtype=np.uint8), ref_off=ref_off)

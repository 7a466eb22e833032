"""The seven host formatters over the one record writer (csrc/npr_textout.h), without a device: every record against a plain Python restatement
of it, on inputs aimed at what a shared writer can get wrong -- run lengths across every digit boundary up to 2^30 - 1, numbers at 0 and at
their largest values, an empty cigar, an empty SEQ, both strands with lower-case and non-ACGT bases, clips of length zero, no record at all.
For each formatter: the sizing call returns what the filling call returns and what the last offset says, a buffer of exactly that size is
filled and not a byte behind it, a buffer one byte short gives NPR_ERR_CAPACITY and stays as it was, and every kind of bad record gives
NPR_ERR_INVALID with the buffer as it was."""
import numpy as np
import pytest

from nanopore_amd import _lib
from nanopore_amd._lib import ERR_CAPACITY, ERR_INVALID, ptr

I32, I64 = 2 ** 31 - 1, 2 ** 63 - 1
# 0, 9, 10, 99, 100, ... 10^9, 2^30 - 1: one to ten digits, both sides of every boundary
LENGTHS = sorted({0, 2 ** 30 - 1} | {10 ** d - 1 for d in range(1, 10)} | {10 ** d for d in range(1, 10)})
SENTINEL = 0xA5
COMPLEMENT = bytes.maketrans(b"ACGTacgt", b"TGCAtgca")


def revcomp(s):
    return s.translate(COMPLEMENT)[::-1]


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def u8(b):
    return np.frombuffer(bytes(b) or b"\0", dtype=np.uint8)


def ragged(items):
    off = np.zeros(len(items) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in items], out=off[1:])
    return u8(b"".join(items)), off


def cigar(ops, letters="MID"):
    return "".join("%d%s" % (n, letters[op]) for op, n in ops).encode() or b"*"


def pack(lists):
    """(word_off, n_ops, words) of op lists, laid out in reverse order with a gap between them: the lists may lie anywhere"""
    words, word_off = [], [0] * len(lists)
    for i in reversed(range(len(lists))):
        words.append(0xFFFFFFFF)  # (between the lists: an operation code outside the table, which nobody may read)
        word_off[i] = len(words)
        words.extend(n << 2 | op for op, n in lists[i])
    return i64(word_off), i64([len(x) for x in lists]), np.ascontiguousarray(words + [0xFFFFFFFF], dtype=np.uint32)


def fn(name):
    return getattr(_lib.load(), name)


def check(name, head, want):
    """head: the arguments before (offsets, out, cap); want: the records"""
    f, text = fn(name), b"".join(want)
    off = np.full(len(want) + 1, -7, dtype=np.int64)
    assert f(*head, ptr(off), None, 0) == len(text), name
    assert off.tolist() == np.concatenate([[0], np.cumsum([len(r) for r in want], dtype=np.int64)]).tolist(), name
    off2 = np.full(len(want) + 1, -7, dtype=np.int64)
    buf = np.full(len(text) + 16, SENTINEL, dtype=np.uint8)
    assert f(*head, ptr(off2), ptr(buf), len(text)) == len(text) == off2[-1], name
    got = bytes(buf[:len(text)])
    for k, r in enumerate(want):
        assert got[off2[k]:off2[k + 1]] == r, (name, k)
    assert (buf[len(text):] == SENTINEL).all(), name
    if text:
        short = np.full(len(text), SENTINEL, dtype=np.uint8)
        assert f(*head, ptr(off2), ptr(short), len(text) - 1) == ERR_CAPACITY, name
        assert (short == SENTINEL).all(), name


def check_invalid(name, head, n_records, why):
    f = fn(name)
    off = np.zeros(n_records + 1, dtype=np.int64)
    buf = np.full(1 << 16, SENTINEL, dtype=np.uint8)
    assert f(*head, ptr(off), None, 0) == ERR_INVALID, (name, why)
    assert f(*head, ptr(off), ptr(buf), buf.size) == ERR_INVALID, (name, why)
    assert (buf == SENTINEL).all(), (name, why)


# op lists: every length with the three operations in turn, lists of one operation at the extremes, an empty list first, last and in between
MID_LISTS = [[], [(k % 3, n) for k, n in enumerate(LENGTHS)], [], [(2, 2 ** 30 - 1)], [(0, 0)], [(1, 9), (0, 10)], []]


def test_format_cigars():
    lists = MID_LISTS + [[(0, I32), (2, 10 ** 9), (1, 2 ** 30)]]  # (op, length) pairs of int32 go further than the packed form
    ops_off = i64(np.concatenate([[0], np.cumsum([len(x) for x in lists])]))
    ops = i32([p for x in lists for p in x]).reshape(-1, 2)
    check("npr_format_cigars", [len(lists), ptr(ops_off), ptr(ops)], [cigar(x) for x in lists])
    check("npr_format_cigars", [0, ptr(ops_off), ptr(ops)], [])
    for why, bad in (("op 3", (3, 5)), ("op -1", (-1, 5)), ("negative length", (1, -1))):
        broken = ops.copy()
        broken[len(broken) // 2] = bad
        check_invalid("npr_format_cigars", [len(lists), ptr(ops_off), ptr(broken)], len(lists), why)


def test_format_cigars_packed():
    word_off, n_ops, words = pack(MID_LISTS)
    check("npr_format_cigars_packed", [len(MID_LISTS), ptr(word_off), ptr(n_ops), ptr(words)], [cigar(x) for x in MID_LISTS])
    check("npr_format_cigars_packed", [0, ptr(word_off), ptr(n_ops), ptr(words)], [])
    broken = words.copy()
    broken[word_off[1] + 4] |= 3
    check_invalid("npr_format_cigars_packed", [len(MID_LISTS), ptr(word_off), ptr(n_ops), ptr(broken)], len(MID_LISTS), "op 3")


def test_format_sam_records():
    refs = [b"chr1", b"", b"a reference with words"]
    rows = [  # qname, flag, reference, pos, mapq, cigar list, seq
        (b"read/0", 0, 0, 0, 0, MID_LISTS[1], b"ACGTNacgtn"),
        (b"", I32, 2, I64, I32, [], b""),
        (b"r", 16, 1, 9, 9, [(0, 9)], b"A"),
        (b"another read", 99, 0, 10, 10, [(1, 10), (2, 2 ** 30 - 1)], b""),
        (b"x" * 300, 100, 2, 10 ** 18, 255, [], b"acgt" * 100),
    ]
    qn, qoff = ragged([r[0] for r in rows])
    rn, roff = ragged(refs)
    seq, soff = ragged([r[6] for r in rows])
    word_off, n_ops, words = pack([r[5] for r in rows])
    flag, ref_index, pos, mapq = i32([r[1] for r in rows]), i32([r[2] for r in rows]), i64([r[3] for r in rows]), i32([r[4] for r in rows])

    def head(n=len(rows), flag=flag, ref_index=ref_index, pos=pos, mapq=mapq, n_ops=n_ops, words=words):
        return [n, ptr(qn), ptr(qoff), ptr(flag), ptr(rn), ptr(roff), ptr(ref_index), ptr(pos), ptr(mapq), ptr(word_off), ptr(n_ops), ptr(words),
                ptr(seq), ptr(soff)]

    def record(r, flag=None, mapq=None):
        return b"\t".join([r[0], b"%d" % (r[1] if flag is None else flag), refs[r[2]], b"%d" % r[3], b"%d" % (r[4] if mapq is None else mapq), cigar(r[5]),
                           b"*", b"0", b"0", r[6] or b"*", b"*"]) + b"\n"

    check("npr_format_sam_records", head(), [record(r) for r in rows])
    check("npr_format_sam_records", head(flag=None, mapq=None), [record(r, flag=0, mapq=255) for r in rows])
    check("npr_format_sam_records", head(n=0), [])

    def with_one(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    broken = words.copy()
    broken[word_off[0] + 7] |= 3
    for why, kw in (("op 3", dict(words=broken)), ("negative n_ops", dict(n_ops=with_one(n_ops, 2, -1))), ("negative pos", dict(pos=with_one(pos, 3, -1))),
                    ("negative flag", dict(flag=with_one(flag, 0, -1))), ("negative mapq", dict(mapq=with_one(mapq, 4, -1))),
                    ("negative reference index", dict(ref_index=with_one(ref_index, 1, -1)))):
        check_invalid("npr_format_sam_records", head(**kw), len(rows), why)


def sam_lines():
    """SAM lines, their spans in the text and the two field columns the splices read: [3], [4] = where the CIGAR column begins and ends"""
    lines = [b"r0\t0\tchr1\t1\t60\t5M\t*\t0\t0\tACGTA\tIIIII\tNM:i:0", b"\t4\t*\t0\t0\t*\t*\t0\t0\t*\t*", b"r2\t16\tchr2\t%d\t255\t3M1I2D7M\t=\t7\t-9\tacgtn\t*" % I32,
             b"last\t0\tchr1\t9\t9\t" + cigar(MID_LISTS[1]) + b"\t*\t0\t0\tA\t*\tXX:Z:a tag\twith\ttabs"]
    text, span, fields, at = b"@HD\tVN:1.0\n", [], np.zeros((len(lines), 16), dtype=np.int64), 0
    for i, line in enumerate(lines):
        at = len(text)
        cols = line.split(b"\t")
        fields[i, 3] = at + len(b"\t".join(cols[:5])) + 1
        fields[i, 4] = fields[i, 3] + len(cols[5])
        span.append((at, at + len(line)))
        text += line + (b"\r\n" if i == 1 else b"\n")
    return lines, u8(text), i64(span), fields


def spliced(line, cig):
    cols = line.split(b"\t")
    return b"\t".join(cols[:5] + [cig] + cols[6:]) + b"\n"


def test_sam_splice():
    lines, text, span, fields = sam_lines()
    lists = [MID_LISTS[1], [], [(0, 2 ** 30 - 1)], [(1, 9), (2, 10), (0, 0)]]
    word_off, n_ops, words = pack(lists)
    head = [ptr(text), ptr(span), ptr(fields), len(lines), ptr(word_off), ptr(n_ops)]
    check("npr_sam_splice", head + [ptr(words)], [spliced(line, cigar(x)) for line, x in zip(lines, lists)])
    check("npr_sam_splice", [ptr(text), ptr(span), ptr(fields), 0, ptr(word_off), ptr(n_ops), ptr(words)], [])
    none = i64([0] * len(lines))  # (no operation anywhere: there need be no words)
    check("npr_sam_splice", [ptr(text), ptr(span), ptr(fields), len(lines), ptr(word_off), ptr(none), None], [spliced(line, b"*") for line in lines])
    broken = words.copy()
    broken[word_off[3] + 1] |= 3
    check_invalid("npr_sam_splice", head + [ptr(broken)], len(lines), "op 3")
    check_invalid("npr_sam_splice", head + [None], len(lines), "operations and no words")
    negative = n_ops.copy()
    negative[1] = -1
    check_invalid("npr_sam_splice", head[:5] + [ptr(negative), ptr(words)], len(lines), "negative n_ops")


def test_sam_splice_text():
    lines, text, span, fields = sam_lines()
    cigars = [cigar(MID_LISTS[1]), b"*", b"", b"1073741823M9I10D"]
    ctext, str_off = ragged(cigars)
    head = [ptr(text), ptr(span), ptr(fields), len(lines)]
    check("npr_sam_splice_text", head + [ptr(str_off), ptr(ctext)], [spliced(line, c) for line, c in zip(lines, cigars)])
    check("npr_sam_splice_text", [ptr(text), ptr(span), ptr(fields), 0, ptr(str_off), ptr(ctext)], [])
    flat = i64([5] * (len(lines) + 1))  # (no text anywhere: there need be none)
    check("npr_sam_splice_text", head + [ptr(flat), None], [spliced(line, b"") for line in lines])
    decreasing = str_off.copy()
    decreasing[2] = decreasing[1] - 1
    check_invalid("npr_sam_splice_text", head + [ptr(decreasing), ptr(ctext)], len(lines), "offsets that decrease")
    check_invalid("npr_sam_splice_text", head + [ptr(str_off), None], len(lines), "text offsets and no text")


# the reads of the two seed formatters: (name, bases); the long one lets clips cross 9 / 10, 99 / 100 and 999 / 1000
READS = [(b"zeta", b"ACGTNacgtnRYKMryk-" * 120), (b"alpha with a description", b"acgttgcaNGGCTAGG"), (b"", b"G"), (b"alph", b""), (b"beta", b"TTAGCAtcgaTCGGATATCGN")]
REFS = [b"chrA", b"", b"chrB some words"]


def seed_inputs():
    text, name_span, begin, end = b"", [], [], []
    for name, seq in READS:
        text += b"@"
        name_span.append((len(text), len(text) + len(name)))
        text += name + b"\n"
        begin.append(len(text))
        end.append(len(text) + len(seq))
        text += seq + b"\n+\n"
    rn, roff = ragged(REFS)
    return u8(text), i64(name_span), i64(begin), i64(end), rn, roff


def test_seed_sam_text():
    text, name_span, begin, end, rn, roff = seed_inputs()
    n0 = len(READS[0][1])
    clips = [0, 9, 10, 99, 100, 999, 1000]
    # rows (read, reference, a, b, strand, L): every pair of clip lengths on the long read in both orientations, then the short reads
    rows = [(0, (j + k) % 3, a, b, strand, n0 - b - rest) for strand in (0, 1) for j, b in enumerate(clips) for k, rest in enumerate(clips)
            for a in ((0, 9, 99, I32 - 1, I32)[(j + k) % 5],)]
    rows += [(1, 2, 0, 0, 0, 16), (1, 0, 5, 3, 1, 8), (1, 1, 9, 15, 1, 1), (2, 0, 0, 0, 1, 1), (4, 2, 10, 1, 0, 19), (4, 2, 10, 0, 1, 21)]
    hit_off = i64(np.concatenate([[0], np.cumsum(np.bincount([r[0] for r in rows], minlength=len(READS)))]))
    hits = i32([(r, a, b - 2 ** 31 if strand else b, L) for _, r, a, b, strand, L in rows])  # (the strand is the top bit of the third column)

    def head(n=len(READS), hit_off=hit_off, hits=hits, end=end, n_refs=len(REFS)):
        return [n, ptr(text), ptr(name_span), ptr(begin), ptr(end), ptr(rn), ptr(roff), n_refs, ptr(hit_off), ptr(hits)]

    def record(i, r, a, b, strand, L):
        name, seq = READS[i]
        rest = len(seq) - b - L
        cig = (b"%dH" % b if b else b"") + b"%dM" % L + (b"%dH" % rest if rest else b"")
        shown = (revcomp(seq) if strand else seq)[b:b + L]
        return b"\t".join([name, b"16" if strand else b"0", REFS[r], b"%d" % (a + 1), b"255", cig, b"*", b"0", b"0", shown, b"*"]) + b"\n"

    check("npr_seed_sam_text", head(), [record(*r) for r in rows])
    no_rows = i64([0] * (len(READS) + 1))
    check("npr_seed_sam_text", head(n=0, hit_off=no_rows), [])
    check("npr_seed_sam_text", head(hit_off=no_rows), [])

    def with_row(k, **kw):
        row = dict(zip(("r", "a", "b", "L"), (int(hits[k, 0]), int(hits[k, 1]), int(hits[k, 2]), int(hits[k, 3]))))
        row.update(kw)
        broken = hits.copy()
        broken[k] = (row["r"], row["a"], row["b"], row["L"])
        return broken

    k = len(rows) - 6  # (the first row of read 1: 16 bases)
    for why, kw in (("reference past the list", dict(hits=with_row(k, r=len(REFS)))), ("negative reference", dict(hits=with_row(k, r=-1))),
                    ("negative a", dict(hits=with_row(k, a=-1))), ("L = 0", dict(hits=with_row(k, L=0))), ("row past its read", dict(hits=with_row(k, L=17))),
                    ("row past its read, reverse", dict(hits=with_row(k + 1, L=14))), ("a list of no references", dict(n_refs=0)),
                    ("offsets that decrease", dict(hit_off=i64([hit_off[0], hit_off[2], hit_off[1]] + list(hit_off[3:])))),
                    ("offsets that start past 0", dict(hit_off=i64([1] + list(hit_off[1:])))),
                    ("a read that ends before it begins", dict(end=i64([end[0], end[1], begin[2] - 1, end[3], end[4]])))):
        check_invalid("npr_seed_sam_text", head(**kw), len(rows), why)


def test_seed_chain_sam_text():
    text, name_span, begin, end, rn, roff = seed_inputs()
    sam_ops = [(k % 9, n) for k, n in enumerate(LENGTHS + [I32, 2 ** 30])]
    # chains (read, reference, strand, ops) in chain order: a read's chains lie together; the records come out by (reference, name)
    chains = [(0, 2, 0, sam_ops), (0, 0, 1, [(0, 9)]), (1, 0, 0, []), (1, 2, 1, [(8, 0), (7, 10)]), (2, 0, 1, [(4, 1)]), (2, 1, 0, []), (3, 0, 0, []), (3, 2, 1, [(3, 99)]),
              (4, 0, 1, [(0, 21)]), (4, 1, 1, [(5, 100), (6, 999)])]
    chain_off = i64(np.concatenate([[0], np.cumsum(np.bincount([c[0] for c in chains], minlength=len(READS)))]))
    rows = i32([(r, strand, 0, 0) for _, r, strand, _ in chains])
    ops_off = i64(np.concatenate([[0], np.cumsum([len(c[3]) for c in chains])]))
    ops = i32([p for c in chains for p in c[3]]).reshape(-1, 2)

    def head(n=len(READS), chain_off=chain_off, rows=rows, ops_off=ops_off, ops=ops, name_span=name_span, n_refs=len(REFS)):
        return [n, ptr(text), ptr(name_span), ptr(begin), ptr(end), ptr(rn), ptr(roff), n_refs, ptr(chain_off), ptr(rows), ptr(ops_off), ptr(ops)]

    def record(i, r, strand, guide):
        name, seq = READS[i]
        return b"\t".join([name, b"16" if strand else b"0", REFS[r], b"1", b"255", cigar(guide, "MIDNSHP=X"), b"*", b"0", b"0", revcomp(seq) if strand else seq, b"*"]) + b"\n"

    want = [record(*c) for c in sorted(chains, key=lambda c: (c[1], READS[c[0]][0]))]
    assert want[0].startswith(b"\t16\tchrA\t1\t255\t1S\t") and want[1].startswith(b"alph\t0\tchrA\t1\t255\t*\t*\t0\t0\t\t*\n")  # (an empty name first, then a name before its extensions)
    check("npr_seed_chain_sam_text", head(), want)
    no_chains = i64([0] * (len(READS) + 1))
    check("npr_seed_chain_sam_text", head(n=0, chain_off=no_chains), [])
    check("npr_seed_chain_sam_text", head(chain_off=no_chains), [])

    def with_one(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    same_name = name_span.copy()
    same_name[4] = same_name[0]
    for why, kw in (("op 9", dict(ops=with_one(ops, 3, (9, 5)))), ("op -1", dict(ops=with_one(ops, 3, (-1, 5)))), ("negative length", dict(ops=with_one(ops, 3, (0, -1)))),
                    ("strand 2", dict(rows=with_one(rows, 4, (0, 2, 0, 0)))), ("reference past the list", dict(rows=with_one(rows, 4, (len(REFS), 0, 0, 0)))),
                    ("negative reference", dict(rows=with_one(rows, 4, (-1, 0, 0, 0)))), ("two reads of one name", dict(name_span=same_name)),
                    ("op offsets that decrease", dict(ops_off=with_one(ops_off, 2, ops_off[1] - 1))), ("op offsets that start past 0", dict(ops_off=with_one(ops_off, 0, 1))),
                    ("chain offsets that decrease", dict(chain_off=with_one(chain_off, 2, chain_off[1] - 1)))):
        check_invalid("npr_seed_chain_sam_text", head(**kw), len(chains), why)


@pytest.mark.parametrize("v", [0, 9, 10, 10 ** 9, 10 ** 10 - 1, 10 ** 10, 10 ** 18 - 1, 10 ** 18, I64])
def test_numbers_of_every_width(v):
    """pos is the one int64 field a formatter prints: up to nineteen digits"""
    qn, off1 = ragged([b"q"])
    none, first, pos, words = i64([0]), i32([0]), i64([v]), np.zeros(1, dtype=np.uint32)
    head = [1, ptr(qn), ptr(off1), None, ptr(qn), ptr(off1), ptr(first), ptr(pos), None, ptr(none), ptr(none), ptr(words), ptr(qn), ptr(off1)]
    check("npr_format_sam_records", head, [b"q\t0\tq\t%d\t255\t*\t*\t0\t0\tq\t*\n" % v])

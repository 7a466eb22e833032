"""What the index-scale tests share (tests/test_bam_index_cases_host.py, tests/test_gpu_bam_index_scale.py; include/nprealign.h,
"coordinate-sorted BAM"): two SAM texts from a fixed seed, as text for the device's writer and as a sorted BAM stream from the encoder of
tests/bam_pileup_reference.py, and the regions queried on the first.  Imports nothing from the product.
  wide    300 references and about 6 000 records of 4 to 12 bases, shuffled.  `big` (refID 1) and `big2` (refID 298) are 2^29 bases long;
          the others draw their lengths from SMALL_LENGTHS.  On the two long ones: 3 600 records, one per 16 kb window, so every one is a
          run of its own; per shift s of SHIFTS records of 10M that start 5 bases before a multiple of 2^s that is no multiple of 2^(s+1)
          (EDGE[s] is one of them), on both strands: their bins are of the level above, bin 0 for 2^26; the same across odd multiples of
          the powers of two between those (BETWEEN), which belong to the next level up; records made long with an N run;
          records at POS 1 and at POS 2^29 (the parser's bound: the second ends past 2^29, bin 0) and an N run that crosses 2^29; on
          `big` the 128 kb stretch from RECUR in which window records and records across a window edge alternate, so the stretch's bin gets
          seven chunks, and a stretch FREE without a record; big2's last record starts at 2^29 - 2^17 + 16380 with 10M: bin 4680, the
          bin of the no-coordinate records behind it.  The short ones carry 4 to 10 records as a rule (a few carry 1): two of three hold
          all of them in window 0 (neighbours then meet in bin 4681 and only the refID tells the runs apart), the third spreads them with
          a record at the last base and over window edges; refIDs of EMPTY carry none (the first, the last, three in a row); refID
          PAST_END (20 000 bases) carries a record at POS 50 001.  Pairs on both strands at one position, records of equal keys, records
          with FLAG 4 and an RNAME (one with a cigar), and 320 records without coordinates.
  single  one reference of 2^29 bases, 2 100 records at POS 1 to 100 on both strands, none unmapped: the largest sort key has 8 bits."""
import numpy as np

import bam_pileup_reference as bp
import bam_reference as ref

TOP = 1 << 29
SHIFTS = (14, 17, 20, 23, 26)
SMALL_LENGTHS = (1, 16384, 16385, 20000, 131072, 131073, 300000)
N_REFS, BIG, BIG2, PAST_END = 300, 1, 298, 10
EMPTY = (0, 150, 151, 152, 299)
EDGE_MULTIPLES = {14: (3, 1001, 12345, 30001), 17: (1, 77, 2001, 4001), 20: (1, 33, 255, 501), 23: (1, 7, 33, 63), 26: (1, 3, 5, 7)}   # odd: of 2^s alone
EDGE = {s: EDGE_MULTIPLES[s][1] << s for s in SHIFTS}
BETWEEN = {15: (5, 9999), 16: (3, 4097), 18: (1, 1025), 19: (7, 513), 21: (3, 129), 22: (1, 65), 24: (5, 17), 25: (1, 9)}   # odd multiples of the powers of two between the levels
RECUR = 8000 << 14                      # 128 kb stretch number 1000 of `big`: bin 585 + 1000
FREE = (20000 << 14, 20100 << 14)       # no record of `big` lies in here
LAST_4680 = TOP - (1 << 17) + 16380
PER_BIG = 1800
NO_COOR = 320
_CASES = {}


def level(b):
    """the level of a bin: 0 for bin 0 (2^29 positions) to 5 for the 16 kb bins"""
    return sum(b >= first for first in (1, 9, 73, 585, 4681))


def _seq(rng, n):
    return "".join("ACGT"[c] for c in rng.integers(0, 4, n))


def _wide():
    rng = np.random.default_rng(2929)
    lengths = [int(v) for v in rng.choice(SMALL_LENGTHS, N_REFS)]
    lengths[BIG] = lengths[BIG2] = TOP
    lengths[PAST_END] = 20000
    refs = [("big" if k == BIG else "big2" if k == BIG2 else "s%d" % k, ln) for k, ln in enumerate(lengths)]
    out = []

    def add(label, flag, tid, pos, cigar, l_seq=None):
        l_seq = bp.consumed(bp.cigar_words(cigar), bp.READ_OPS) if cigar != "*" else (7 if l_seq is None else l_seq)
        out.append(dict(name="%s_%d" % (label, len(out)), flag=flag, tid=tid, pos=pos, cigar=cigar, seq=_seq(rng, l_seq)))

    def clipped(pos, rl, limit):
        """rl bases at pos: matched up to `limit`, the rest clipped"""
        m = max(1, min(rl, limit - pos))
        return "%dM" % m + ("%dS" % (rl - m) if rl > m else "")

    # ---- the two long references
    edge_windows = {(m << s) >> 14 for table in (EDGE_MULTIPLES, BETWEEN) for s in table for m in table[s]}
    taken = {0, 32767} | edge_windows | {w - 1 for w in edge_windows} | set(range(FREE[0] >> 14, FREE[1] >> 14)) | set(range((RECUR >> 14) - 1, (RECUR >> 14) + 9))
    for tid in (BIG, BIG2):
        free = np.array([w for w in range(32760 if tid == BIG2 else 32768) if w not in taken])
        for k, w in enumerate(rng.choice(free, PER_BIG, replace=False)):
            rl = int(rng.integers(4, 13))
            off = (0, 16384 - rl)[k % 2] if k % 50 < 2 else int(rng.integers(0, 16384 - rl + 1))    # some begin or end exactly at a window edge
            add("w", 16 * int(rng.integers(0, 2)), tid, (int(w) << 14) + off, "%dM" % rl)
        for s in SHIFTS:
            for m in EDGE_MULTIPLES[s]:
                for flag in (0, 16):
                    add("e%d" % s, flag, tid, (m << s) - 5, "10M")
        for s in BETWEEN:    # across an edge of 2^s alone: the level is the next one of SHIFTS above s, and a bin rule that shifts by one too few misses it
            for m in BETWEEN[s]:
                add("x%d" % s, 16 * (m & 2) // 2, tid, (m << s) - 5, "10M")
        for pos, cigar in ((5000000, "5M70000000N5M"), (400000000, "5M70000000N5M"), (100000123, "5M200000N5M"), (200000000, "5M2000000N5M"), (250000000, "5M20000N5M"),
                           (60000000, "4M9000000N2M3I2M")):
            add("n", 16 * (pos & 1), tid, pos, cigar)
        add("first", 0, tid, 0, "10M"), add("first", 16, tid, 0, "6M"), add("first", 0, tid, 0, "10M")
        add("unmapped_placed", 4, tid, 123456789, "*"), add("unmapped_placed", 4 + 16, tid, 123456789, "8M")   # the interval is one base, whatever the cigar says
    add("at_bound", 0, BIG, TOP - 1, "10M"), add("at_bound", 16, BIG, TOP - 1, "10M")            # POS 2^29: ends past 2^29, bin 0
    add("over_bound", 0, BIG, TOP - 1000, "5M70000000N5M")                                        # an N run across 2^29: bin 0, the last window
    add("last4680", 0, BIG2, LAST_4680, "10M")
    for q in range(7):   # window, edge, window, edge, ...: the bin of the stretch recurs with other bins between
        add("recur16", 16 * (q & 1), BIG, RECUR + (q << 14) + 100, "8M")
        add("recur128", 0, BIG, RECUR + ((q + 1) << 14) - 5, "10M")
    add("recur16", 0, BIG, RECUR + (7 << 14) + 100, "8M")

    # ---- the short ones
    for tid in range(N_REFS):
        if tid in EMPTY or tid in (BIG, BIG2):
            continue
        ln = lengths[tid]
        count = 1 if tid % 29 == 5 else int(rng.integers(4, 11))
        first = len(out)
        if tid % 3:      # everything in window 0: the reference begins and ends in bin 4681
            for _ in range(count):
                pos, rl = int(rng.integers(0, min(ln, 16384))), int(rng.integers(4, 13))
                add("a", 16 * int(rng.integers(0, 2)), tid, pos, clipped(pos, rl, min(ln, 16384)))
        else:
            for _ in range(count):
                pos, rl = int(rng.integers(0, ln)), int(rng.integers(4, 13))
                add("b", 16 * int(rng.integers(0, 2)), tid, pos, clipped(pos, rl, ln))
            add("b_last_base", 0, tid, ln - 1, "1M5S")
            if ln > 16384:
                add("b_edge", 16, tid, 16384 - 5, "10M")
            if ln >= 131072:
                add("b_edge", 0, tid, 131072 - 5, clipped(131072 - 5, 10, ln)), add("b_n", 0, tid, 3000, "5M%dN5M" % int(rng.integers(10000, 120000)))
        r = out[first]
        add("twin", r["flag"] ^ 16, tid, r["pos"], r["cigar"]), add("twin", r["flag"], tid, r["pos"], r["cigar"])    # both strands at one position; an equal key
        if tid % 12 == 1:
            add("unmapped_placed", 4, tid, int(rng.integers(0, min(ln, 16384))), "*")
    add("past_end", 0, PAST_END, 50000, "9M")          # POS 50 001 on 20 000 bases: bin 4684, the reference's last window
    for k in range(NO_COOR):
        add("u", 4 + 16 * (k % 3 == 0), -1, -1, "*", l_seq=int(rng.integers(4, 13)))
    order = rng.permutation(len(out))
    return dict(refs=refs, records=[out[i] for i in order])


def _single():
    rng = np.random.default_rng(100)
    out = []
    for k in range(2100):
        rl = int(rng.integers(4, 13))
        out.append(dict(name="s_%d" % k, flag=16 * int(rng.integers(0, 2)), tid=0, pos=int(rng.integers(0, 100)), cigar="%dM" % rl, seq=_seq(rng, rl)))
    return dict(refs=[("solo", TOP)], records=out)


def case(name):
    """name "wide" or "single" -> dict(refs=[(name, length)], records=[dict(name, flag, tid, pos, cigar, seq)] in the SAM file's order); built once"""
    if name not in _CASES:
        _CASES[name] = {"wide": _wide, "single": _single}[name]()
    return _CASES[name]


def header_text(name, order="unsorted"):
    return "@HD\tVN:1.4\tSO:%s\n" % order + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in case(name)["refs"])


def lines(name):
    """the records as SAM lines, which are also the lines of the specification's decoder (upper-case bases, no qualities)"""
    refs = case(name)["refs"]
    return ["\t".join([r["name"], str(r["flag"]), refs[r["tid"]][0] if r["tid"] >= 0 else "*", str(r["pos"] + 1), "30" if r["tid"] >= 0 else "0", r["cigar"], "*", "0", "0",
                       r["seq"], "*"]) for r in case(name)["records"]]


def sam_text(name):
    return header_text(name) + "\n".join(lines(name)) + "\n"


def key_order(name):
    """the places of the file's lines in stable coordinate order"""
    recs, n_refs = case(name)["records"], len(case(name)["refs"])
    return sorted(range(len(recs)), key=lambda i: ref.sort_key(recs[i]["tid"], recs[i]["pos"], recs[i]["flag"], n_refs))


def counts(name):
    """what sam_to_bam counts: records, no_coordinate, unmapped (FLAG 4)"""
    recs = case(name)["records"]
    return dict(records=len(recs), no_coordinate=sum(r["tid"] < 0 for r in recs), unmapped=sum(bool(r["flag"] & 4) for r in recs))


def sorted_stream(name):
    """The coordinate-sorted BAM stream of the records, by the Python encoder (no qualities, bin 0): what the host test decodes."""
    recs = case(name)["records"]
    out = [bp.header(case(name)["refs"], text=header_text(name, "coordinate"))]
    for i in key_order(name):
        r = recs[i]
        out.append(bp.record(r["name"], r["flag"], r["tid"], r["pos"], bp.cigar_words(r["cigar"]) if r["cigar"] != "*" else [], [1 << "ACGT".index(c) for c in r["seq"]],
                             mapq=30 if r["tid"] >= 0 else 0))
    return b"".join(out)


def _regions():
    """about 60 (tid, beg, end) on `wide`, every one inside its reference"""
    length = [ln for _, ln in case("wide")["refs"]]
    rng = np.random.default_rng(61)
    out = []
    for s in SHIFTS:
        out += [(BIG, EDGE[s] - 1, EDGE[s]), (BIG, EDGE[s], EDGE[s] + 1), (BIG, EDGE[s] - 20, EDGE[s] + 20)]
    out += [(BIG, 0, TOP), (BIG2, 0, TOP), (PAST_END, 0, 20000), (3, 0, length[3]), (256, 0, length[256]), (297, 0, length[297])]      # whole references
    out += [(BIG, FREE[0] + 5, FREE[1] - 5), (BIG, FREE[0] + 16384, FREE[0] + 16385)]                                                  # where `big` has no record
    out += [(0, 0, length[0]), (151, 0, 1), (299, 0, length[299])]                                                                     # references without a record
    out += [(BIG, 0, 1), (BIG, TOP - 1, TOP), (BIG2, TOP - (1 << 17), TOP), (BIG2, TOP - 1, TOP), (BIG, RECUR, RECUR + (1 << 17)), (BIG, RECUR + 16383, RECUR + 16384),
            (PAST_END, 19999, 20000), (BIG2, EDGE[26] - 1, EDGE[26] + 1), (BIG, 40000000, 40000001)]
    for k in range(12):
        tid = (BIG, BIG2)[k & 1]
        beg = int(rng.integers(0, TOP - 1))
        out.append((tid, beg, min(TOP, beg + int(rng.choice([1, 100, 20000, 2000000, 100000000])))))
    for _ in range(10):
        tid = int(rng.integers(2, 298))
        beg = int(rng.integers(0, length[tid]))
        out.append((tid, beg, min(length[tid], beg + int(rng.choice([1, 50, 5000, 200000])))))
    return out


REGIONS = _regions()

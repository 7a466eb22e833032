"""Constructed BAM files for npr_pileup_add_bam (tests/test_bam_pileup_host.py, tests/test_gpu_bam_pileup.py): each case a few records
on references of at most a few thousand bases (the long cigars: 70 000), written with the encoder of tests/bam_pileup_reference.py.
cases() -> {name: dict(refs, records, stream, file)}; the files are built once."""
import struct

import numpy as np

import bam_pileup_reference as bp

_rng = np.random.default_rng(41)
REFS = [("one", 3000)]


def _nibbles(n):
    """mostly A C G T, now and then another code"""
    nib = np.array([1, 2, 4, 8])[_rng.integers(0, 4, n)]
    other = _rng.random(n) < 0.1
    nib[other] = np.array([0, 15, 3, 5, 14])[_rng.integers(0, 5, n)][other]
    return [int(v) for v in nib]


def _rec(name, pos, cigar, flag=0, tid=0, **kw):
    words = bp.cigar_words(cigar) if isinstance(cigar, str) else list(cigar)
    return bp.record(name, flag, tid, pos, words, _nibbles(bp.consumed(words, bp.READ_OPS)), **kw)


def _mixed(n):
    """a cigar of n operations: M I M D ... with lengths 1 .. 4"""
    ops = [0, 1, 0, 2]
    return [int(_rng.integers(1, 5)) << 4 | ops[k % 4] for k in range(n)]


def _build():
    out = {}

    def case(name, records, refs=REFS, member=65280, level=6):
        stream = bp.header(refs) + b"".join(records)
        out[name] = dict(refs=refs, records=records, stream=stream, file=bp.bgzf(stream, member=member, level=level))

    case("cigar lengths", [_rec("ops%d" % n, 10 + n, _mixed(n)) for n in (1, 63, 64, 65, 128, 129)], member=777)
    m63 = [(1 << 4) | (k & 1) for k in range(63)]   # 1M 1I 1M ... 1M: 63 operations
    case("chunk boundaries", [
        _rec("deal", 5, "100M"),                                      # an M run across the 64-column deal
        _rec("deal and chunk", 40, m63 + bp.cigar_words("70M70M3I")),   # ... across the deal in operations 63 and 64, of two chunks
        _rec("I after the chunk's end", 300, m63 + bp.cigar_words("5M2I4M")),        # operation 63 a column, 64 an I
        _rec("I after I over the edge", 500, m63[:62] + bp.cigar_words("5M2I3I4M")),   # operations 63 and 64 both I
        _rec("I after N over the edge", 700, m63[:62] + bp.cigar_words("5M9N2I4M")),   # 62 a column, 63 an N, 64 an I
        _rec("leading I over the edge", 900, [(1 << 4) | 1] * 64 + bp.cigar_words("2I3M1I")),  # no column in the first chunk
    ])
    case("sequence edges", [
        _rec("odd", 0, "7M"), _rec("even", 3, "8M"), _rec("one", 2999, "1M"),
        bp.record("all codes", 0, 0, 100, bp.cigar_words("16M"), list(range(16))),
        bp.record("all codes from the low nibble", 0, 0, 101, bp.cigar_words("1S16M"), [1] + list(range(16))),
    ])
    case("other operations", [
        _rec("eq and x", 10, "3=2X4M"), _rec("N then I", 50, "5M10N2I5M"), _rec("P H S", 100, "2H3S5M1P5M4S2H"),
        _rec("zero lengths", 150, "5M0I0D0M0N0S3M"), _rec("I after a zero M", 200, "5M0M2I3M"), _rec("I 0M I", 250, "4M2I0M3I5M"),
        _rec("I P I", 300, "4M2I1P3I5M"), _rec("I N I", 350, "4M2I7N3I5M"), _rec("D then N then I", 400, "2M3D6N1I2M"),
        _rec("only clips", 450, "6S"), _rec("N first", 500, "9N4M"), _rec("D first", 550, "3D4M"),
    ], level=1)
    case("insertion rule", [_rec("leading I", 10, "2I5M"), _rec("2I3I", 30, "5M2I3I5M"), _rec("trailing I", 60, "5M3I"),
                            _rec("I after D", 90, "5M2I2D1I3M"), _rec("only I", 120, "4I"), _rec("I I M", 150, "1I2I3M1I")])
    case("reference bounds", [_rec("ends at l_ref", 2990, "10M"), _rec("one past l_ref", 2991, "10M"), _rec("D ends with the sequence", 2992, "5M3D"),
                              _rec("N past l_ref", 2990, "5M6N"), _rec("in bounds", 1000, "10M")])
    short = bp.record("read one short", 0, 0, 40, bp.cigar_words("5M"), _nibbles(6))
    long_ = bp.record("read one long", 0, 0, 50, bp.cigar_words("5M1I"), _nibbles(5))
    case("validation", [_rec("fine", 10, "6M"), short, long_, _rec("pos -1", -1, "6M"), _rec("operation 9", 70, [(3 << 4) | 0, (2 << 4) | 9, (3 << 4) | 0]),
                        _rec("fine too", 20, "6M")])
    case("not selected", [_rec("refID -1", 10, "5M", tid=-1), bp.record("l_seq 0", 0, 0, 10, bp.cigar_words("5M"), []),
                          bp.record("no cigar", 0, 0, 10, [], _nibbles(5))] +
         [_rec("flag %x" % f, 10, "5M", flag=f) for f in (0x4, 0x100, 0x200, 0x400, 0x800, 0x10, 0x904)])
    case("not one selected", [_rec("unmapped", 10, "5M", flag=4), _rec("refID -1", -1, "5M", tid=-1)])
    case("no records", [])
    three = [("first", 500), ("middle", 700), ("last", 300)]
    case("several sequences", [_rec("a", 490, "10M", tid=0), _rec("b", 0, "3M2D3M", tid=2), _rec("c", 290, "5M5D", tid=2), _rec("d", 0, "4M1I4M", tid=0),
                               _rec("past the last", 291, "5M5D", tid=2)], refs=three)
    big = [("long", 70000)]
    words = bp.cigar_words("1M1D") * 32768
    nib = _nibbles(32768)
    z, b = b"XzZsome text\0", b"XbBc" + struct.pack("<I3b", 3, -1, 2, 3)
    case("long cigar", [bp.cg_record("cg", 0, 0, 100, words, nib),
                        bp.cg_record("cg third", 16, 0, 4000, words, nib, aux_before=z + b),
                        bp.cg_record("cg then more", 0, 0, 7, bp.cigar_words("5M2I5M"), _nibbles(12), aux_after=z),
                        bp.cg_record("no cg", 0, 0, 200, words, nib, with_cg=False, aux_before=z),
                        bp.cg_record("two cg: the first", 0, 0, 300, bp.cigar_words("3M"), _nibbles(3), aux_after=b"CGBI" + struct.pack("<II", 1, 3 << 4 | 2)),
                        bp.cg_record("empty cg", 0, 0, 300, [], _nibbles(3)),
                        bp.record("CG without the placeholder", 0, 0, 400, bp.cigar_words("4M"), _nibbles(4), aux=b"CGBI" + struct.pack("<II", 1, 9 << 4))],
         refs=big)
    ok = bp.cigar_words("4M1D4M")

    def broken(name, pos, aux_before=b"", aux_after=b"", words=ok):
        return bp.cg_record(name, 0, 0, pos, words, _nibbles(bp.consumed(words, bp.READ_OPS)), aux_before=aux_before, aux_after=aux_after)

    case("malformed auxiliary bytes", [
        _rec("before", 10, "9M"),
        broken("Z without NUL", 100, aux_after=b"XzZno end"),
        broken("fine", 130),
        broken("B count past the record", 200, aux_before=b"XbBs" + struct.pack("<I", 1000) + b"\1\0"),
        broken("unknown type", 300, aux_before=b"XqQ\0\0\0\0"),
        broken("unknown subtype", 350, aux_before=b"XbBq" + struct.pack("<I", 0)),
        broken("a field cut by the end", 400, aux_after=b"Xi"),
        broken("an integer cut by the end", 450, aux_after=b"XiI\0\0"),
        broken("CG element with operation 9", 500, words=[(4 << 4) | 0, (1 << 4) | 9, (4 << 4) | 0]),
        # the same bytes are no one's business without the placeholder: the stored cigar applies and the fields are not walked
        bp.record("malformed but no placeholder", 0, 0, 600, bp.cigar_words("5M"), _nibbles(5), aux=b"XzZno end"),
        _rec("after", 700, "9M"),
    ], member=333)
    return out


_CASES = None


def cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES

"""Constructed BAM files for the BAM reader (npr_bam_sam, npr_bam_open + npr_pileup_add_bam; tests/test_bam_read_cases_host.py,
tests/test_gpu_bam_read_scale.py), written with the encoder of tests/bam_pileup_reference.py and compressed by Python's zlib: another
writer's files.
  field_cases()     records this project's writer never makes, each named for what it carries, on about 3000 references
  refusal_cases()   three records each, the second one refused by a check only the device makes in npr_bam_sam
  many(n)           n minimal records built with numpy, with the SAM body and the pileup table they must give, for the sizes at which
                    the reader's tables and grids begin to stride (below); many(n, tag_every=1): auxiliary bytes in every record
Imports nothing from the product."""
import itertools
import struct

import numpy as np

import bam_pileup_reference as bp
import bam_reference as ref

# Where the reader starts another round or another trip of a grid-stride loop.  SOURCE: (file under nanopore_amd/csrc, the text of the
# defining line, how often it stands there); tests/test_bam_read_cases_host.py fails when a line no longer reads so.
WALK = 1 << 18           # npr_bam_api.cpp: constexpr int64_t kWalk = int64_t(1) << 18;   (npr_bam_sam and npr_bam_open: offsets a walk round)
GATHER_GRID = 65536      # npr_bamread.hip: k_bam_gather_aux, dim3(static_cast<unsigned>(a.n < 65536 ? a.n : 65536))
EMIT_GRID = 1 << 20      # npr_bamread.hip: k_bam_emit, dim3(static_cast<unsigned>(a.n_items < (1 << 20) ? a.n_items : (1 << 20)))
PILE_RECORDS = 4096 * 4  # npr_bampile.hip: groups < 4096 ? groups : 4096 workgroups of THREADS / WAVE = 256 / 64 wavefronts, a record each
SOURCE = {
    "WALK": [("npr_bam_api.cpp", "constexpr int64_t kWalk = int64_t(1) << 18;", 2)],
    "GATHER_GRID": [("npr_bamread.hip", "k_bam_gather_aux, dim3(static_cast<unsigned>(a.n < 65536 ? a.n : 65536))", 1),
                    ("npr_bamread.hip", "for (int64_t i = blockIdx.x; i < a.n; i += gridDim.x) {", 1)],
    "EMIT_GRID": [("npr_bamread.hip", "k_bam_emit, dim3(static_cast<unsigned>(a.n_items < (1 << 20) ? a.n_items : (1 << 20)))", 1),
                  ("npr_bamread.hip", "for (int64_t item = blockIdx.x; item < a.n_items; item += gridDim.x) {", 1)],
    "PILE_RECORDS": [("npr_bampile.hip", "const int grid = static_cast<int>(groups < 4096 ? groups : 4096);", 1),
                     ("npr_bampile.hip", "constexpr int WAVE = 64;", 1), ("npr_bampile.hip", "constexpr int THREADS = 256;", 1),
                     ("npr_bampile.hip", "constexpr int WAVES = THREADS / WAVE;", 1),
                     ("npr_bampile.hip", "r < a.n; r += static_cast<int64_t>(gridDim.x) * WAVES) {", 1)],
}

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
# operation lengths on both sides of every change in the number of decimal digits, 0 and the largest a cigar word holds
DIGIT_EDGES = [0] + [v for k in range(1, 9) for v in (10 ** k - 1, 10 ** k)] + [(1 << 28) - 1]


# ---------------------------------------------------------------- records other writers make
N_REFS, ONE_LETTER, LONG_NAME = 3000, 1500, 2999


def _refs():
    refs = [("r%d" % k, 60) for k in range(N_REFS)]
    refs[0] = ("first", 5000)
    refs[ONE_LETTER] = ("q", 60)
    refs[LONG_NAME] = ("a_reference_sequence_with_a_name_of_some_length", 60)
    return refs


def _edge_words(ops):
    """every length of DIGIT_EDGES, on the operations given in turn (H and P consume nothing: the record stays one a pileup adds)"""
    return [v << 4 | ref.OPS.index(ops[k % len(ops)]) for k, v in enumerate(DIGIT_EDGES)]


def _counted_words(n):
    """n operations M I M D ... with lengths 1 .. 12: one and two digits, so that the places in the text are no multiple of anything"""
    return [(k % 12 + 1) << 4 | (0, 1, 0, 2)[k % 4] for k in range(n)]


def _build_fields():
    rng = np.random.default_rng(23)
    refs = _refs()

    def nib(n):
        return [int(v) for v in np.array([1, 2, 4, 8, 15, 0, 3])[rng.integers(0, 7, n)]]

    def rec(name, cigar, pos=3, tid=0, flag=0, folded=False, **kw):
        words = bp.cigar_words(cigar) if isinstance(cigar, str) else list(cigar)
        make = bp.cg_record if folded else bp.record
        return name, make(name, flag, tid, pos, words, nib(bp.consumed(words, bp.READ_OPS)), **kw)

    z, i8, arr = b"XzZsome text\0", b"XcC\x07", b"XbBs" + struct.pack("<I2h", 2, -3, 4)
    m5 = bp.cigar_words("5M")
    out = [
        # cigar text: lengths at every decimal boundary, operation counts around the 256 of a trip, stored and folded into CG
        rec("lengths at the digit edges", _edge_words("HP") + m5),
        rec("lengths at the digit edges on N and D", m5 + _edge_words("ND")),          # (a pileup refuses it: past l_ref)
        rec("lengths at the digit edges folded", _edge_words("PH") + m5, folded=True),
        rec("a length of 0 first and last", "0M5M0I0D"),
    ]
    for n in (255, 256, 257, 513):
        out.append(rec("%d operations" % n, _counted_words(n), pos=n % 7))
        out.append(rec("%d operations folded" % n, _counted_words(n), pos=n % 5, folded=True, flag=16))
    out += [
        # column extremes
        rec("flag 65535 and mapq 255", "5M", flag=65535, mapq=255),
        rec("pos -1 on a real refID", "5M", pos=-1, tid=5),
        rec("the largest pos and next_pos", "5M", pos=INT32_MAX - 1, tid=7, next_tid=7, next_pos=INT32_MAX - 1),
        rec("tlen INT32_MIN", "5M", tlen=INT32_MIN), rec("tlen INT32_MAX", "5M", tlen=INT32_MAX), rec("tlen -1", "5M", tlen=-1),
        rec("next_pos -1 beside a next_refID", "5M", next_tid=3, next_pos=-1),
        rec("refID -1 with a next_refID", "5M", pos=-1, tid=-1, next_tid=LONG_NAME, next_pos=11),
        rec("refID -1 with a one-letter next_refID", "5M", pos=-1, tid=-1, next_tid=ONE_LETTER, next_pos=0),
        rec("a one-letter RNAME, a long RNEXT", "5M", tid=ONE_LETTER, next_tid=LONG_NAME, next_pos=9),
        rec("a long RNAME, a one-letter RNEXT", "5M", tid=LONG_NAME, next_tid=ONE_LETTER, next_pos=99),
        rec("next_refID equal to refID", "5M", tid=ONE_LETTER, next_tid=ONE_LETTER, next_pos=12, tlen=-40),
        rec("x", "5M"),
        rec("n" * 254, "5M"),
        rec("a non-zero bin", "5M", bin=37449),
        ("odd l_seq, garbage in the unused nibble", bp.record("odd l_seq, garbage in the unused nibble", 0, 0, 40, m5, [1, 2, 4, 8, 1, 15], l_seq=5, qual=bytes([0, 1, 2, 3, 4]))),
        ("one base, garbage in the unused nibble", bp.record("one base, garbage in the unused nibble", 16, 0, 50, bp.cigar_words("1M"), [8, 9], l_seq=1, qual=bytes([93]))),
        ("qualities 0 to 93", bp.record("qualities 0 to 93", 0, 0, 100, bp.cigar_words("94M"), nib(94), qual=bytes(range(94)))),
        ("no cigar, no bases", bp.record("no cigar, no bases", 4, -1, -1, [], [])),
        # tag placement around a folded CG
        rec("CG the only field", "3M2I3M", folded=True),
        rec("CG first", "3M2I3M", folded=True, aux_after=z + i8),
        rec("CG in the middle", "3M2I3M", folded=True, aux_before=z, aux_after=arr + i8),
        rec("CG last", "3M2I3M", folded=True, aux_before=i8 + arr),
        rec("CG of no element", [], folded=True, aux_before=i8),
        rec("a second CG stays a tag", "4M", folded=True, aux_after=b"CGBI" + struct.pack("<II", 1, 3 << 4 | 2)),
        rec("CG without the placeholder stays a tag", "4M", aux=b"CGBI" + struct.pack("<II", 1, 7 << 4)),
        rec("tags and no CG", "4M", aux=z + arr + i8),
    ]
    names, records = [n for n, _ in out], [r for _, r in out]
    assert len(set(names)) == len(names)
    stream = bp.header(refs) + b"".join(records)
    text, got_refs, decoded = ref.bam_decode(stream, any_writer=True)
    assert got_refs == refs and [d["line"].split("\t")[0] for d in decoded] == names
    return dict(refs=refs, names=names, records=records, stream=stream, file=bp.bgzf(stream, member=4001, level=6), header_text=text,
                lines=[d["line"] for d in decoded])


_FIELDS = None


def field_cases():
    """-> dict(refs, names, records, stream, file, header_text, lines): lines[k] is what record k (names[k]) prints, by the specification's
    decoder (tests/bam_reference.py bam_decode, any_writer=True)."""
    global _FIELDS
    if _FIELDS is None:
        _FIELDS = _build_fields()
    return _FIELDS


def refusal_cases():
    """-> {name: dict(stream, file, decoder)}: three records, the second one refused by npr_bam_sam on the device.  decoder: what bam_decode
    makes of the stream -- the exception it raises, or "POS" / "PNEXT" when it decodes and that column of the second line exceeds SAM's
    2^31 - 1 (the reader's decision for a stored pos of INT32_MAX: refused in the walk, by npr_bam_open too)."""
    refs = [("one", 3000)]
    m4, nib = bp.cigar_words("4M"), [1, 2, 4, 8]
    fine = [bp.record("before", 0, 0, 10, m4, nib), bp.record("after", 16, 0, 20, m4, nib, aux=b"XzZfine\0")]
    second = {
        "cigar operation 9": (bp.record("bad", 0, 0, 15, [2 << 4, 2 << 4 | 9], nib), IndexError),
        "cigar operation 15": (bp.record("bad", 0, 0, 15, [4 << 4 | 15], nib), IndexError),
        "Z without NUL": (bp.record("bad", 0, 0, 15, m4, nib, aux=b"XaAq" + b"XzZno end"), ValueError),
        "pos INT32_MAX": (bp.record("bad", 0, 0, INT32_MAX, m4, nib), "POS"),
        "next_pos INT32_MAX": (bp.record("bad", 0, 0, 15, m4, nib, next_tid=0, next_pos=INT32_MAX), "PNEXT"),
    }
    out = {}
    for name, (bad, decoder) in second.items():
        stream = bp.header(refs) + fine[0] + bad + fine[1]
        out[name] = dict(stream=stream, file=bp.bgzf(stream, level=6), decoder=decoder, walk=isinstance(decoder, str))
    return out


# ---------------------------------------------------------------- many minimal records
L = 5000
MANY_REFS = [("one", L)]
_DIGITS = "0123456789abcdefghijklmnopqrstuvwxyz"
_MANY = {}


def _names(n):
    """0 1 .. z 10 11 ..: the index in base 36, made by counting, not by dividing (many() divides: the host test holds both together)"""
    out, width = [], 1
    while len(out) < n:
        first = 0 if width == 1 else 36 ** (width - 1)   # (products before this one begin with 0)
        out.extend("".join(t) for t in itertools.islice(itertools.product(_DIGITS, repeat=width), first, first + n - len(out)))
        width += 1
    return out


def special_fits(i):
    """whether record i, a multiple of 4099 (2M1D1M, four reference bases), ends inside the reference: else a pileup refuses it"""
    return (7 * i) % (L - 1) + 4 <= L


def many(n, tag_every=1000):
    """n records on one reference of L bases: QNAME i in base 36, flag 0 / 16, pos (7 i) % (L - 1), mapq 30, cigar 1M, the base of nibble
    1 << (i & 3), quality i % 94; every tag_every-th (1000th) with a tag Xi:i:<i>, every 4099th 2M1D1M with that base and quality three times.
    -> dict(stream, file, offsets: where each record begins in the stream and the stream's end, header_text, body: the SAM lines as bytes,
    table int32 [L, 8], counts).  Built once per (n, tag_every)."""
    if (n, tag_every) in _MANY:
        return _MANY[(n, tag_every)]
    i = np.arange(n, dtype=np.int64)
    width = np.ones(n, dtype=np.int64)
    for k in range(1, 8):
        width += i >= 36 ** k
    special, tagged = i % 4099 == 0, i % tag_every == 0
    l_seq = np.where(special, 3, 1)
    pos, flag, nibble, quality = (7 * i) % (L - 1), 16 * (i & 1), 1 << (i & 3), i % 94
    size = 32 + (width + 1) + 4 * l_seq + (l_seq + 1) // 2 + l_seq + 7 * tagged   # (as many operations as bases)
    header = bp.header(MANY_REFS)
    offsets = len(header) + np.concatenate([[0], np.cumsum(size + 4)])
    buf = np.zeros(int(offsets[-1]), dtype=np.uint8)
    buf[:len(header)] = np.frombuffer(header, dtype=np.uint8)
    fixed = np.dtype([("size", "<i4"), ("tid", "<i4"), ("pos", "<i4"), ("l_name", "u1"), ("mapq", "u1"), ("bin", "<u2"), ("n_cig", "<u2"), ("flag", "<u2"),
                      ("l_seq", "<i4"), ("ntid", "<i4"), ("npos", "<i4"), ("tlen", "<i4")])
    assert fixed.itemsize == 36
    code = np.frombuffer(_DIGITS.encode(), dtype=np.uint8)
    for w in range(1, int(width.max()) + 1):
        for s in (False, True):
            for t in (False, True):
                idx = np.flatnonzero((width == w) & (special == s) & (tagged == t))
                if not len(idx):
                    continue
                m, bases = len(idx), 3 if s else 1
                head = np.zeros(m, dtype=fixed)
                head["size"], head["pos"], head["l_name"], head["mapq"], head["n_cig"] = size[idx], pos[idx], w + 1, 30, bases
                head["flag"], head["l_seq"], head["ntid"], head["npos"] = flag[idx], bases, -1, -1
                name = np.zeros((m, w + 1), dtype=np.uint8)
                for d in range(w):
                    name[:, w - 1 - d] = code[(idx // 36 ** d) % 36]
                words = np.array(bp.cigar_words("2M1D1M" if s else "1M"), dtype="<u4")
                cigar = np.broadcast_to(words.view(np.uint8), (m, 4 * bases))
                nb = nibble[idx].astype(np.uint8)
                seq = np.stack([nb << 4 | nb, nb << 4], axis=1) if s else (nb << 4)[:, None]
                qual = np.repeat(quality[idx].astype(np.uint8)[:, None], bases, axis=1)
                parts = [head.view(np.uint8).reshape(m, 36), name, cigar, seq, qual]
                if t:
                    parts.append(np.concatenate([np.broadcast_to(np.frombuffer(b"Xii", dtype=np.uint8), (m, 3)), idx.astype("<i4").view(np.uint8).reshape(m, 4)], axis=1))
                mat = np.concatenate(parts, axis=1)
                assert mat.shape[1] == 4 + size[idx[0]]
                at = offsets[idx]
                for c in range(mat.shape[1]):
                    buf[at + c] = mat[:, c]
    stream = buf.tobytes()

    # the SAM body, by string formatting of the same fields
    lines = ["%s\t%d\tone\t%d\t30\t%s\t*\t0\t0\t%s\t%s" % (q, 16 * (k & 1), (7 * k) % (L - 1) + 1, "1M" if k % 4099 else "2M1D1M", "ACGT"[k & 3] * (1 if k % 4099 else 3),
                                                           chr(33 + k % 94) * (1 if k % 4099 else 3)) for k, q in enumerate(_names(n))]
    for k in range(0, n, tag_every):
        lines[k] += "\tXi:i:%d" % k
    body = ("\n".join(lines) + "\n").encode() if n else b""

    # the pileup table, by the rules of bam_pileup_reference.pileup: words 0-3 the base's column, 5 a deleted column, 7 the first column
    table = np.zeros((L, 8), dtype=np.int32)
    base = (i & 3)
    plain, fits = ~special, special & (pos + 4 <= L)
    np.add.at(table, (pos[plain], base[plain]), 1)
    np.add.at(table, (pos[plain], 7), 1)
    for d in (0, 1, 3):
        np.add.at(table, (pos[fits] + d, base[fits]), 1)
    np.add.at(table, (pos[fits] + 2, 5), 1)
    np.add.at(table, (pos[fits], 7), 1)
    refused = int((special & ~fits).sum())
    table.setflags(write=False)
    _MANY[(n, tag_every)] = dict(n=n, stream=stream, file=bp.bgzf(stream, level=1), offsets=offsets, header_text=header[8:8 + struct.unpack_from("<i", header, 4)[0]].decode(),
                    body=body, table=table, counts=dict(records=n, selected=n, added=n - refused, refused=refused))
    return _MANY[(n, tag_every)]


def with_block_size(m, k, value):
    """the file of many() case m with the block_size of record k overwritten -> (file, the record's stream byte)"""
    at = int(m["offsets"][k])
    stream = bytearray(m["stream"])
    stream[at:at + 4] = struct.pack("<i", value)
    return bp.bgzf(bytes(stream), level=1), at

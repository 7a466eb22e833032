"""The host side of the FastQC analysis (no device): the position bins and their inverse, the quality-line scanner
(npr_fastq_qual_index), the percentile rule, and the report writer with every status rule driven to warn and fail."""
import numpy as np
import pytest

import read_quality_reference as ref
from nanopore_amd import _lib, ingest
from nanopore_amd.analyses import fastqc
from nanopore_amd.realign import ReadQuality


def _plain_bin(p):
    if p < 16:
        return p
    if p >= 1 << 24:
        return 335
    e = 0
    while (p >> (e + 1)) > 0:
        e += 1
    return 16 * (e - 3) + ((p >> (e - 4)) & 15)


def test_position_bins_against_a_plain_loop():
    ps = [0, 15, 16, 31, 32, 33, 63, 64, (1 << 24) + 5]
    for k in range(25):
        ps += [p for p in ((1 << k) - 1, 1 << k, (1 << k) + 1) if p >= 0]
    want = [_plain_bin(p) for p in ps]
    assert ref.pos_bin(np.array(ps)).tolist() == want == [fastqc.posBin(p) for p in ps]
    assert _plain_bin(31) == 31 and _plain_bin(32) == 32 and _plain_bin(33) == 32 and _plain_bin(63) == 47 and _plain_bin(64) == 48
    assert _plain_bin(2047) == 127 and _plain_bin(2048) == 128 and _plain_bin((1 << 24) - 1) == 335 == ref.POS_BINS - 1
    dense = np.arange(0, 5000)
    assert ref.pos_bin(dense).tolist() == [_plain_bin(int(p)) for p in dense]


def test_inverse_edges_tile_the_positions_without_gap_or_overlap():
    at = 0
    for b in range(ref.POS_BINS):
        lo, hi = fastqc.binRange(b)
        assert lo == at and hi > lo
        assert _plain_bin(lo) == b and _plain_bin(hi - 1) == b
        at = hi
    assert at == 1 << 24


def _index(text):
    L = _lib.load()
    buf = np.frombuffer(text, dtype=np.uint8) if text else np.zeros(0, dtype=np.uint8)
    n = L.npr_fastq_index(_lib.ptr(buf), len(buf), None, 0)
    assert n >= 0
    rec, qual = np.zeros((n, 4), dtype=np.int64), np.full((n, 2), -7, dtype=np.int64)
    assert L.npr_fastq_index(_lib.ptr(buf), len(buf), _lib.ptr(rec), n) == n
    rc = L.npr_fastq_qual_index(_lib.ptr(buf), len(buf), _lib.ptr(rec), n, _lib.ptr(qual))
    return rc, rec, qual


HAND = b"@r0 first\nACGT\n+r0 first\nIIII\n@r1\n\n+\n\n@r2\r\nAC\r\n+\r\n#5\r\n@r3\nACGTN\n+\n!~ZZ@"


def test_quality_line_index_on_a_hand_written_file(tmp_path):
    rc, rec, qual = _index(HAND)
    assert rc == _lib.OK
    lines = HAND.decode().split("\n")
    want = [lines[4 * k + 3].rstrip("\r") for k in range(4)]
    assert want == ["IIII", "", "#5", "!~ZZ@"]
    assert [HAND[a:b].decode() for a, b in qual] == want
    assert (qual[:, 1] - qual[:, 0]).tolist() == (rec[:, 3] - rec[:, 2]).tolist()
    assert qual[3, 1] == len(HAND)   # a last record without a trailing newline
    path = tmp_path / "hand.fq"
    path.write_bytes(HAND)
    t = ingest.FastqTable(str(path))
    assert t._qual_span is None   # made when first asked for
    assert t.qual_span.tolist() == qual.tolist() and t.qual_span is t.qual_span
    # a last record cut off after its '+' line: an empty span at the end of the text; cut off inside the '+' line the same
    for cut in (b"@r0\nACGT\n+\n", b"@r0\nACGT\n+"):
        rc, rec, qual = _index(cut)
        assert rc == _lib.OK and qual.tolist() == [[len(cut), len(cut)]]
    rc, rec, qual = _index(b"")
    assert rc == _lib.OK and len(qual) == 0
    # records that are not what npr_fastq_index gave: refused
    L = _lib.load()
    buf = np.frombuffer(HAND, dtype=np.uint8)
    for bad in ([0, 0, 5, len(HAND) + 1], [0, 0, 9, 3], [0, 0, 0, 3]):
        rec1, out = np.array([bad], dtype=np.int64), np.zeros((1, 2), dtype=np.int64)
        assert L.npr_fastq_qual_index(_lib.ptr(buf), len(buf), _lib.ptr(rec1), 1, _lib.ptr(out)) == _lib.ERR_INVALID


def test_percentile_rule_on_hand_histograms():
    single = [0] * 94
    single[40] = 7
    assert [fastqc.percentile(single, k) for k in (10, 25, 50, 75, 90)] == [40] * 5
    halves = [0] * 94
    halves[10] = halves[30] = 50
    assert [fastqc.percentile(halves, k) for k in (10, 25, 50, 75, 90)] == [10, 10, 10, 30, 30]   # ceil(100 * 50 / 100) = 50 is reached at 10
    halves[10] = 49
    assert fastqc.percentile(halves, 50) == 30   # ceil(99 * 50 / 100) = 50 > 49
    one = [0] * 94
    one[3] = 1
    assert [fastqc.percentile(one, k) for k in (10, 50, 90)] == [3, 3, 3]
    with pytest.raises(ValueError):
        fastqc.percentile([0] * 94, 50)


def _tables(reads):
    text, seq, qual = ref.fastq_text(reads)
    return ReadQuality(*[a[0] for a in ref.tables(text, seq, qual, [0] * len(reads), 1)])


EXPECTED = """##FastQC\t%s
>>Basic Statistics\tpass
#Measure\tValue
Filename\thand.fq
File type\tConventional base calls
Encoding\tSanger / Illumina 1.9
Total Sequences\t2
Sequence length\t2-2
%%GC\t50
#Malformed records\t3
>>END_MODULE
>>Per base sequence quality\tpass
#Base\tMean\tMedian\tLower Quartile\tUpper Quartile\t10th Percentile\t90th Percentile
1\t35.0\t30\t30\t40\t30\t40
2\t40.0\t40\t40\t40\t40\t40
>>END_MODULE
>>Per sequence quality scores\tpass
#Quality\tCount
35\t1
40\t1
>>END_MODULE
>>Per base sequence content\tpass
#Base\tG\tA\tT\tC
1\t0.0\t50.0\t50.0\t0.0
2\t50.0\t0.0\t0.0\t50.0
>>END_MODULE
>>Per sequence GC content\tpass
#GC Content\tCount
%s
>>END_MODULE
>>Per base N content\tpass
#Base\tN-Count
1\t0.0
2\t0.0
>>END_MODULE
>>Sequence Length Distribution\tpass
#Length\tCount
2-2\t2
>>END_MODULE
"""


def test_report_text_of_a_hand_made_table_set(tmp_path):
    t = _tables([(b"AC", b"?I"), (b"TG", b"II")])   # '?' = 30, 'I' = 40
    gc_rows = "\n".join("%d\t%d" % (p, 2 if p == 50 else 0) for p in range(101))
    want = EXPECTED % (fastqc.VERSION, gc_rows)
    assert fastqc.fastqcDataText(t, "hand.fq", malformed=3) == want
    path = tmp_path / "fastqc_data.txt"
    fastqc.writeFastqcData(str(path), t, "hand.fq", malformed=3)
    assert path.read_text() == want


def _status(reads):
    text = fastqc.fastqcDataText(_tables(reads), "x.fq")
    return dict(line[2:].split("\t") for line in text.split("\n") if line.startswith(">>") and line != ">>END_MODULE")


def _q(*values):
    return bytes(33 + v for v in values)


def test_every_status_rule_goes_to_warn_and_fail():
    base = _status([(turn * 4, _q(*[40] * 16)) for turn in (b"ACGT", b"CGTA", b"GTAC", b"TACG")])   # every base a quarter of every position
    assert set(base.values()) == {"pass"} and list(base) == [
        "Basic Statistics", "Per base sequence quality", "Per sequence quality scores", "Per base sequence content", "Per sequence GC content",
        "Per base N content", "Sequence Length Distribution"]
    # per base quality: lower quartile < 10 (warn), < 5 (fail); median < 25 (warn), < 20 (fail) -- four reads AT, position 0 varies
    def at0(*qs):
        return _status([(b"AT", _q(q, 40)) for q in qs])["Per base sequence quality"]
    assert at0(9, 40, 40, 40) == "warn" and at0(4, 40, 40, 40) == "fail" and at0(10, 40, 40, 40) == "pass"
    assert at0(24, 24, 40, 40) == "warn" and at0(19, 19, 40, 40) == "fail" and at0(25, 25, 40, 40) == "pass"
    # per sequence quality: the most frequent mean
    def means(*qs):
        return _status([(b"AT", _q(q, q)) for q in qs])["Per sequence quality scores"]
    assert means(26, 26, 40) == "warn" and means(19, 19, 40) == "fail" and means(27, 27, 40) == "pass"
    # per base content: |A - T| of position 0 in points
    def content(n_a, n_t):
        return _status([(b"AC", _q(40, 40))] * n_a + [(b"TG", _q(40, 40))] * n_t)["Per base sequence content"]
    assert content(5, 5) == "pass" and content(11, 9) == "pass" and content(56, 44) == "warn" and content(61, 39) == "fail"
    # N content of position 0
    def ns(n_n, n_a):
        return _status([(b"NA", _q(40, 40))] * n_n + [(b"TA", _q(40, 40))] * n_a)["Per base N content"]
    assert ns(1, 19) == "pass" and ns(2, 18) == "warn" and ns(5, 15) == "fail"
    # lengths: more than one bin (warn), an empty read (fail)
    def lengths(*ls):
        return _status([(b"A" * n, _q(*[40] * n)) for n in ls])["Sequence Length Distribution"]
    assert lengths(5, 5) == "pass" and lengths(5, 6) == "warn" and lengths(5, 0) == "fail" and lengths(32, 33) == "pass"


def test_merge_is_the_table_of_the_union():
    a, b = [(b"ACGTN", b"IIII#"), (b"", b"")], [(b"GG", b"~!")]
    m = fastqc.mergeTables(_tables(a), _tables(b))
    for got, want in zip(m.arrays(), _tables(a + b).arrays()):
        assert got.tolist() == want.tolist()
    none = ReadQuality.zeros(1).group(0)
    none.totals[2:6] = -1
    for got, want in zip(fastqc.mergeTables(none, _tables(b)).arrays(), _tables(b).arrays()):
        assert got.tolist() == want.tolist()


def test_the_new_symbols_are_in_the_signature_table():
    assert "npr_read_quality" in _lib.SIGNATURES and "npr_fastq_qual_index" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["npr_read_quality"][1]) == 15 and len(_lib.SIGNATURES["npr_fastq_qual_index"][1]) == 5
    L = _lib.load()
    assert hasattr(L, "npr_read_quality") and hasattr(L, "npr_fastq_qual_index")
    assert ReadQuality.TILE == _lib.RQ_TILE == 2048 and (_lib.RQ_POS_BINS, _lib.RQ_QUAL_COLS) == (ref.POS_BINS, ref.QUAL_COLS)

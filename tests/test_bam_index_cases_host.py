"""The two SAM texts of tests/bam_index_cases.py reach what tests/test_gpu_bam_index_scale.py runs them for: conditions on the inputs,
from the sorted stream of the Python encoder and the specification's decoder (tests/bam_reference.py) alone -- every bin level, more runs
and records than two tiles of the sorts and scans, a fourth pass of the run sort, runs that only the refID separates, a bin of several
chunks, bin 4680 in front of the no-coordinate records, a one-pass record sort; the regions lie inside their references, some of them
empty, and reach every bin level -- and the sizes all that stands on are still the sources'.  No GPU."""
import os

import pytest

import bam_index_cases as cases
import bam_reference as ref

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nanopore_amd", "csrc")
SORT_TILE = SCAN_TILE = 2048
SOURCE = (("npr_device.h", "constexpr int BAM_SORT_BITS = 8, BAM_SORT_DIGITS = 1 << BAM_SORT_BITS;"), ("npr_device.h", "constexpr int BAM_SORT_ROUNDS = 8;"),
          ("npr_device.h", "constexpr int BAM_SORT_TILE = 256 * BAM_SORT_ROUNDS;"), ("npr_scan.h", "constexpr int SCAN_THREADS = 256;"),
          ("npr_scan.h", "constexpr int SCAN_PER_THREAD = 8;"), ("npr_scan.h", "constexpr int SCAN_TILE = SCAN_THREADS * SCAN_PER_THREAD;"),
          ("npr_bam.hip", "constexpr int THREADS = 256, WAVE = 64, WAVES = THREADS / WAVE;"),
          ("npr_bam_api.cpp", "sort_order(dev, d_run_key, runs, 16 + bits_of(static_cast<unsigned long long>(n_refs)), d_perm);"))


@pytest.fixture(scope="module")
def wide():
    text, refs, decoded = ref.bam_decode(cases.sorted_stream("wide"))
    assert refs == cases.case("wide")["refs"] and text == cases.header_text("wide", "coordinate")
    return decoded


@pytest.fixture(scope="module")
def single():
    return ref.bam_decode(cases.sorted_stream("single"))[2]


def _heads(decoded):
    """the places where a run of one (tid, bin) begins"""
    keys = [(r["tid"], ref.record_bin(r)) for r in decoded]
    return [j for j in range(len(keys)) if j == 0 or keys[j] != keys[j - 1]]


def test_the_size_constants_are_the_sources():
    for file, text in SOURCE:
        assert open(os.path.join(CSRC, file)).read().count(text) == 1, (file, text)


def test_the_decoder_reads_the_lines_back(wide, single):
    for name, decoded in (("wide", wide), ("single", single)):
        lines = cases.lines(name)
        assert [r["line"] for r in decoded] == [lines[i] for i in cases.key_order(name)]
        assert len({r["name"] for r in cases.case(name)["records"]}) == len(lines)


def test_every_bin_level_and_the_records_at_the_bounds(wide):
    mapped = [r for r in wide if r["tid"] >= 0]
    per_level = [sum(cases.level(ref.record_bin(r)) == lv for r in mapped) for lv in range(6)]
    print("records per bin level:", per_level)
    assert min(per_level) >= 3
    by_name = {r["line"].split("\t")[0].rsplit("_", 1)[0]: r for r in wide}
    assert by_name["at_bound"]["pos"] == cases.TOP - 1 and by_name["at_bound"]["end"] > cases.TOP and ref.record_bin(by_name["at_bound"]) == 0
    assert by_name["over_bound"]["end"] > cases.TOP and ref.record_bin(by_name["over_bound"]) == 0
    assert by_name["last4680"]["pos"] == cases.TOP - (1 << 17) + 16380 and ref.record_bin(by_name["last4680"]) == 4680
    past = by_name["past_end"]
    assert past["tid"] == cases.PAST_END and past["pos"] == 50000 and cases.case("wide")["refs"][cases.PAST_END][1] == 20000 and ref.record_bin(past) == 4681 + 3
    assert any(r["pos"] == 0 for r in mapped if r["tid"] == cases.BIG)
    for s, multiples in cases.BETWEEN.items():   # across an edge of 2^s alone, s not of SHIFTS: the bin's level is the one a shift of s could not tell from the next
        want = sum(s > v for v in cases.SHIFTS)
        for m in multiples:
            at = [r for r in mapped if r["tid"] == cases.BIG and r["pos"] == (m << s) - 5]
            assert m & 1 and at and all(cases.level(ref.record_bin(r)) == 5 - want for r in at), (s, m)
    for s in cases.SHIFTS:   # the records 5 bases before a multiple of 2^s lie one level up
        at = [r for r in mapped if r["tid"] == cases.BIG and r["pos"] == cases.EDGE[s] - 5]
        assert len(at) == 2 and {r["flag"] for r in at} == {0, 16} and all(cases.level(ref.record_bin(r)) == 4 - cases.SHIFTS.index(s) for r in at)


def test_more_than_two_tiles_of_runs_records_and_references(wide):
    heads = _heads(wide)
    print("records", len(wide), "runs", len(heads))
    assert len(heads) >= 2 * SORT_TILE + 1 and len(heads) >= 2 * SCAN_TILE + 1
    assert len(wide) > 2 * SCAN_TILE
    refs = cases.case("wide")["refs"]
    assert len(refs) >= 256 and any(r["tid"] >= 256 for r in wide)            # a fourth pass of the run sort, and keys that need it
    assert len({j // 256 for j in heads}) >= 3 and min(heads[1:]) < 2048 < max(heads)
    # one record per window on the two long references, each a run of its own
    windows = [(r["tid"], r["pos"] >> 14) for r in wide if r["line"].startswith("w_")]
    assert len(windows) == len(set(windows)) >= 3000 and all(refs[t][1] == cases.TOP for t, _ in windows)


def test_the_shapes_the_head_test_and_the_index_writer_meet(wide):
    refs = cases.case("wide")["refs"]
    mapped = [r for r in wide if r["tid"] >= 0]
    shared = [(a["tid"], b["tid"]) for a, b in zip(mapped, mapped[1:]) if a["tid"] != b["tid"] and ref.record_bin(a) == ref.record_bin(b)]
    print("reference pairs that share the bin across their boundary:", len(shared))
    assert len(shared) >= 30
    assert wide[len(mapped) - 1]["tid"] == cases.BIG2 and ref.record_bin(wide[len(mapped) - 1]) == 4680 and wide[len(mapped)]["tid"] == -1
    assert all(r["tid"] == -1 for r in wide[len(mapped):]) and len(wide) - len(mapped) >= 300 > 256
    bins = ref.expected_index(wide, [ln for _, ln in refs])[0]
    assert max(len(c) for b in bins for c in b.values()) >= 3 and len(bins[cases.BIG][585 + (cases.RECUR >> 17)]) == 7
    have = {r["tid"] for r in mapped}
    assert all(t not in have for t in cases.EMPTY) and have == set(range(cases.N_REFS)) - set(cases.EMPTY)
    assert cases.EMPTY[0] == 0 and cases.EMPTY[-1] == len(refs) - 1 and cases.EMPTY[1:4] == (150, 151, 152)
    assert sum(1 for r in mapped if r["flag"] & 4) >= 20
    at = {}
    for r in mapped:
        at.setdefault((r["tid"], r["pos"]), set()).add(r["flag"] & 16)
    assert sum(len(v) == 2 for v in at.values()) >= 100, "both strands at one position"
    keys = [ref.sort_key(r["tid"], r["pos"], r["flag"], len(refs)) for r in wide]
    assert sum(a == b for a, b in zip(keys, keys[1:])) >= 100, "equal keys"
    assert cases.counts("wide") == dict(records=len(wide), no_coordinate=len(wide) - len(mapped), unmapped=sum(1 for r in wide if r["flag"] & 4))
    per_ref = [sum(1 for r in mapped if r["tid"] == t) for t in range(len(refs)) if t not in cases.EMPTY + (cases.BIG, cases.BIG2)]
    assert len(per_ref) >= 290 and sum(4 <= c <= 16 for c in per_ref) > 0.8 * len(per_ref)
    assert {ln for _, ln in refs} == set(cases.SMALL_LENGTHS) | {cases.TOP}


def test_single_sorts_in_one_pass(single):
    assert len(single) == 2100 and cases.case("single")["refs"] == [("solo", cases.TOP)]
    keys = [(r["pos"] + 1) << 1 | (r["flag"] >> 4 & 1) for r in single]
    assert all(r["tid"] == 0 and not r["flag"] & 4 and r["pos"] < 100 for r in single) and max(keys) < 1 << 8
    assert len(set(keys)) < len(keys) // 5 and {r["flag"] & 16 for r in single} == {0, 16}
    assert cases.counts("single") == dict(records=2100, no_coordinate=0, unmapped=0)


def test_the_regions(wide):
    refs = cases.case("wide")["refs"]
    assert 50 <= len(cases.REGIONS) <= 70
    levels, hits = set(), 0
    for tid, beg, end in cases.REGIONS:
        assert 0 <= tid < len(refs) and 0 <= beg < end <= refs[tid][1], (tid, beg, end)
        found = ref.brute_overlaps(wide, tid, beg, end)
        hits += bool(found)
        bins = set(ref.reg2bins(beg, end))
        for i in found:
            b = ref.record_bin(wide[i])
            assert b in bins
            levels.add(cases.level(b))
    print("regions", len(cases.REGIONS), "non-empty", hits)
    assert len(cases.REGIONS) / 3 <= hits < len(cases.REGIONS)
    assert levels == set(range(6)), "every bin level is reached by a non-empty region"
    for s in cases.SHIFTS:
        e = cases.EDGE[s]
        assert {(cases.BIG, e - 1, e), (cases.BIG, e, e + 1), (cases.BIG, e - 20, e + 20)} <= set(cases.REGIONS)
        assert ref.brute_overlaps(wide, cases.BIG, e - 1, e) and ref.brute_overlaps(wide, cases.BIG, e, e + 1)
    assert not ref.brute_overlaps(wide, cases.BIG, *cases.FREE)
    assert any(t in cases.EMPTY for t, _, _ in cases.REGIONS) and any(refs[t][1] == e - b for t, b, e in cases.REGIONS)

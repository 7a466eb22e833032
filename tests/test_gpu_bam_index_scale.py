"""The sort and the index of Context.sam_to_bam(sort=True, index=True) past one tile (csrc/npr_bam.hip: k_bam_index_heads, the scan of the
head flags, k_bam_index_runs, the sort over (tid, bin) runs, k_bam_gather_runs; csrc/npr_bam_host.cpp: npr_bai_write, npr_bai_chunks) on
the two SAM texts of tests/bam_index_cases.py -- tests/test_bam_index_cases_host.py states what they reach: every bin level, more than
two tiles of records and of runs, 300 references (a fourth pass of the run sort), runs only the refID separates, a bin of seven chunks,
bin 4680 in front of the no-coordinate records, records past 2^29 and past their reference's end, a record sort of one pass.  The files
are read back with the specification's decoders (tests/bam_reference.py, tests/bgzf_deflate_reference.py); the index is compared with the
restated rules byte for byte and queried through the restated reader, npr_bai_chunks and the device's region reader.  Bytes and counts:
every comparison is exact."""
import numpy as np
import pytest

import bam_index_cases as cases
import bam_reference as ref
import bam_region_cases as region_cases
import bgzf_deflate_reference as dref
from nanopore_amd import bam
from nanopore_amd.realign import NprError

pytestmark = pytest.mark.gpu


def _convert(ctx, sam, path, compress=False):
    counts = ctx.sam_to_bam(sam, path, sort=True, index=True, compress=compress)
    data = open(path, "rb").read()
    stream, _ = (dref if compress else ref).bgzf_read(data)
    return dict(path=path, counts=counts, data=np.frombuffer(data, dtype=np.uint8), bai=open(path + ".bai", "rb").read(), stream=stream,
                blocks=region_cases.bgzf_blocks(data))


@pytest.fixture(scope="module")
def files(gpu_ctx, tmp_path_factory):
    """"wide" (stored), "wide_z" (compressed), "single" -> dict(path, counts, data, bai, stream, blocks; text, refs, decoded, lines, of_tid,
    head_end): converted once, never changed"""
    d = tmp_path_factory.mktemp("bamindex")
    out = {}
    for name in ("wide", "single"):
        sam = str(d / (name + ".sam"))
        with open(sam, "w") as fh:
            fh.write(cases.sam_text(name))
        out[name] = dict(_convert(gpu_ctx, sam, str(d / (name + ".bam"))), sam=sam)
    out["wide_z"] = dict(_convert(gpu_ctx, out["wide"]["sam"], str(d / "wide_z.bam"), compress=True), sam=out["wide"]["sam"])
    for name, f in out.items():
        f["text"], f["refs"], f["decoded"] = ref.bam_decode(f["stream"])
        f["lines"] = [r["line"] for r in f["decoded"]]
        f["of_tid"] = ref.records_of_tid(f["decoded"])
        f["head_end"] = region_cases.header_end(f["stream"])
        f["ref_len"] = [ln for _, ln in f["refs"]]
    return out


def _case(name):
    return "single" if name == "single" else "wide"


@pytest.mark.parametrize("name", ("wide", "wide_z", "single"))
def test_stable_key_order_bins_and_counts(files, name):
    f, case = files[name], _case(name)
    assert f["text"] == cases.header_text(case, "coordinate") and f["refs"] == cases.case(case)["refs"]
    lines = cases.lines(case)
    want = [lines[i] for i in cases.key_order(case)]      # (names are unique: records of equal keys are told apart, and must keep the file's order)
    assert len(f["lines"]) == len(want)
    for j, (g, w) in enumerate(zip(f["lines"], want)):
        assert g == w, (j, g, w)
    for r in f["decoded"]:
        assert r["bin"] == ref.record_bin(r), r["line"]
    assert {k: f["counts"][k] for k in ("records", "no_coordinate", "unmapped")} == cases.counts(case)
    assert f["counts"]["references"] == len(f["refs"]) and f["counts"]["mapped"] == f["counts"]["records"] - f["counts"]["unmapped"]


@pytest.mark.parametrize("name", ("wide", "single"))
def test_the_stored_index_is_the_restated_rules_byte_for_byte(files, name):
    f = files[name]
    want = ref.bai_bytes(*ref.expected_index(f["decoded"], f["ref_len"]))
    got = f["bai"]
    if got != want:   # say where, before the bytes are compared
        (gi, gn), (wi, wn) = ref.bai_parse(got), ref.bai_parse(want)
        assert gn == wn
        for k, (g, w) in enumerate(zip(gi, wi)):
            assert sorted(g[0]) == sorted(w[0]), ("the bins of reference", k)
            for b in w[0]:
                assert g[0][b] == w[0][b], ("reference", k, "bin", b)
            assert g[1] == w[1], ("the windows of reference", k)
    assert got == want
    assert len(files["wide"]["blocks"]) >= 5


def test_the_compressed_index_points_at_the_same_stream_bytes(files):
    s, p = files["wide"], files["wide_z"]
    assert p["stream"] == s["stream"] and len(p["data"]) < len(s["data"]) and len(p["bai"]) == len(s["bai"])
    blocks, n, file_len = dref.bgzf_read(p["data"].tobytes())[1], len(p["stream"]), len(p["data"])
    (idx_s, no_s), (idx_p, no_p) = ref.bai_parse(s["bai"]), ref.bai_parse(p["bai"])
    assert no_s == no_p == cases.NO_COOR
    seen = 0
    for (bins_s, lin_s), (bins_p, lin_p) in zip(idx_s, idx_p):
        assert sorted(bins_s) == sorted(bins_p) and len(lin_s) == len(lin_p)
        pairs = list(zip(lin_s, lin_p))
        for b in bins_s:
            assert len(bins_s[b]) == len(bins_p[b])
            if b == 37450:   # the second pseudo-chunk holds counts, not offsets
                assert bins_s[b][1] == bins_p[b][1]
                pairs += list(zip(bins_s[b][0], bins_p[b][0]))
            else:
                pairs += [(x, y) for cs, cp in zip(bins_s[b], bins_p[b]) for x, y in zip(cs, cp)]
        for vs, vp in pairs:
            us = (vs >> 16) // (ref.P + 31) * ref.P + (vs & 0xffff)
            assert dref.voffset_to_stream(blocks, vp, n, file_len) == us
            seen += 1
    assert seen > 60000


def test_a_second_conversion_gives_the_same_bytes(gpu_ctx, files, tmp_path):
    """(the index's meta, linear and no-coordinate tables are made with atomics from several workgroups)"""
    for name in ("wide", "wide_z"):
        again = _convert(gpu_ctx, files[name]["sam"], str(tmp_path / (name + ".bam")), compress=name == "wide_z")
        assert again["data"].tobytes() == files[name]["data"].tobytes() and again["bai"] == files[name]["bai"]


@pytest.mark.parametrize("name", ("wide", "wide_z"))
def test_the_reader_through_the_written_index_finds_the_brute_force_set(files, name):
    f = files[name]
    index = ref.bai_parse(f["bai"])[0]
    n = len(f["stream"])
    vo = ref.voffset if name == "wide" else (lambda u: ref.voffset_by_walking(f["blocks"], u, n))
    sizes = []
    for region in cases.REGIONS:
        want = ref.brute_overlaps(f["decoded"], *region)
        assert ref.bai_query_tid(index, f["decoded"], f["of_tid"], *region, vo=vo) == want, region
        assert region_cases.query_by_walking(f["bai"], f["decoded"], f["blocks"], n, *region) == want, region
        sizes.append(len(want))
    assert 0 in sizes and max(sizes) > 1800 and len(cases.REGIONS) / 3 <= sum(1 for v in sizes if v) < len(sizes)


@pytest.mark.parametrize("name", ("wide", "wide_z", "single"))
def test_the_host_chunk_reader_is_the_restated_rule(files, name):
    f = files[name]
    regions = cases.REGIONS if name != "single" else [(0, 0, 1), (0, 0, cases.TOP), (0, 99, 100), (0, 100, 101), (0, 16384, 20000), (0, cases.TOP - 1, cases.TOP)]
    some = 0
    for region in regions:
        got, n_ref = bam.bai_chunks(f["bai"], *region)
        want = region_cases.chunks_rule(f["bai"], *region)
        assert n_ref == len(f["refs"]) and [tuple(int(v) for v in c) for c in got] == want, region
        some += bool(want)
    assert 0 < some < len(regions) or name == "single"


def _sam(stream):
    text = stream.sam_text().tobytes().decode()
    return text[:stream.l_text], text[stream.l_text:].split("\n")[:-1]


def _device_regions(decoded):
    """about 20 of the regions: two and more per bin level of the records they find, and the ones that find nothing"""
    per_level, out = [0] * 6, []
    for region in cases.REGIONS:
        levels = {cases.level(ref.record_bin(decoded[i])) for i in ref.brute_overlaps(decoded, *region)}
        if any(per_level[lv] < 2 for lv in levels):
            out.append(region)
            for lv in levels:
                per_level[lv] += 1
    assert min(per_level) >= 2, per_level
    fixed = [(cases.BIG, cases.FREE[0] + 5, cases.FREE[1] - 5), (0, 0, cases.case("wide")["refs"][0][1]), (151, 0, 1), (cases.PAST_END, 0, 20000), (cases.BIG2, 0, cases.TOP),
             (cases.BIG, cases.TOP - 1, cases.TOP), (cases.BIG2, cases.TOP - (1 << 17), cases.TOP), (cases.BIG, cases.RECUR, cases.RECUR + (1 << 17)), (256, 0, cases.case("wide")["refs"][256][1]), (cases.BIG2, cases.EDGE[26] - 1, cases.EDGE[26] + 1)]
    assert set(fixed) <= set(cases.REGIONS)
    return out + [r for r in fixed if r not in out]


@pytest.mark.parametrize("name", ("wide", "wide_z"))
def test_the_device_region_reader_on_the_written_index(gpu_ctx, files, name):
    f = files[name]
    regions = _device_regions(f["decoded"])
    assert 15 <= len(regions) <= 30
    predicted = {r: region_cases.blocks_rule(f["blocks"], region_cases.chunks_rule(f["bai"], *r), f["head_end"]) for r in regions}
    assert all(len(need) < len(f["blocks"]) for need in predicted.values()) and len({tuple(need) for need in predicted.values()}) >= 4, "computed before anything runs"
    print(name, "blocks", len(f["blocks"]), {r: len(need) for r, need in predicted.items()})
    sizes = []
    for region in regions:
        want = ref.brute_overlaps(f["decoded"], *region)
        with gpu_ctx.bam_open(f["data"], index=f["bai"], region=region) as s:
            last, need = bam.inflate_last(gpu_ctx), predicted[region]
            assert last["blocks"] == len(need) and last["failed_block"] == -1, region
            assert s.stream_bytes == last["stream_bytes"] == sum(f["blocks"][k][2] for k in need), region
            assert s.n_records == len(want) and s.references == [n for n, _ in f["refs"]] and s.lengths.tolist() == f["ref_len"]
            header, lines = _sam(s)
            assert header == f["text"] and lines == [f["lines"][i] for i in want], region
        sizes.append(len(want))
    assert 0 in sizes and max(sizes) > 1800


def test_records_past_two_to_the_29_and_past_their_reference(files):
    """include/nprealign.h, npr_sam_bam, MEASURE and INDEX: a record that ends past 2^29 lies in bin 0 and in the last of the 32 768 windows;
    one that starts past its reference's end keeps the bin of its position and lies in the reference's last window.  Neither is refused."""
    f = files["wide"]
    index = ref.bai_parse(f["bai"])[0]
    by_label = {}
    for r in f["decoded"]:
        by_label.setdefault(r["line"].split("\t")[0].rsplit("_", 1)[0], []).append(r)
    bins, linear = index[cases.BIG]
    assert len(linear) == 1 << 15
    over, at_bound = by_label["over_bound"][0], by_label["at_bound"]
    assert over["pos"] == cases.TOP - 1000 and over["end"] > cases.TOP and over["bin"] == 0
    assert [r["pos"] for r in at_bound] == [cases.TOP - 1] * 2 and all(r["end"] == cases.TOP + 9 and r["bin"] == 0 for r in at_bound)
    assert linear[-1] == ref.voffset(over["u0"])               # the first record of the last window; no window beyond it
    for r in [over] + at_bound:
        assert any(c[0] <= ref.voffset(r["u0"]) < c[1] for c in bins[0])
    past = by_label["past_end"][0]
    bins, linear = index[cases.PAST_END]
    assert past["pos"] == 50000 and past["bin"] == 4681 + 3 and f["ref_len"][cases.PAST_END] == 20000
    assert len(linear) == 2 and bins[4684] == [(ref.voffset(past["u0"]), ref.voffset(past["u1"]))]
    in_last = [r for r in f["decoded"] if r["tid"] == cases.PAST_END and (max(r["end"], r["pos"] + 1) - 1) >> 14 >= 1]
    assert past in in_last and linear[1] == min(ref.voffset(r["u0"]) for r in in_last)


def test_a_reference_longer_than_two_to_the_29_is_accepted(gpu_ctx, tmp_path):
    """include/nprealign.h, npr_sam_bam: an @SQ length above 2^29 is fine, because the parser keeps POS at or below 2^29 -- every record
    begins where a BAI can address it; what reaches further lies in bin 0 and in windows past the 32 768th, which no query consults."""
    top = cases.TOP
    refs = [("long", (1 << 31) - 1), ("edge", top + 1), ("short", 1000)]
    rows = [("a", 0, "long", 1000, "10M"), ("b", 16, "long", top - 100, "5M300000N5M"), ("c", 0, "long", top, "10M"), ("d", 0, "edge", top, "10M"), ("e", 0, "edge", top, "1M9S"),
            ("f", 0, "short", 5, "10M"), ("g", 0, "long", top - 20000, "10M")]
    rng = np.random.default_rng(3)
    sam, path = str(tmp_path / "long.sam"), str(tmp_path / "long.bam")
    with open(sam, "w") as fh:
        fh.write("@HD\tVN:1.4\tSO:unsorted\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % r for r in refs))
        for name, flag, rname, pos, cigar in rows:
            fh.write("\t".join([name, str(flag), rname, str(pos), "30", cigar, "*", "0", "0", "".join("ACGT"[c] for c in rng.integers(0, 4, 10)), "*"]) + "\n")
    f = _convert(gpu_ctx, sam, path)
    text, got_refs, decoded = ref.bam_decode(f["stream"])
    assert got_refs == refs and [r["line"].split("\t")[0] for r in decoded] == ["a", "g", "b", "c", "d", "e", "f"]
    assert [r["bin"] for r in decoded] == [ref.record_bin(r) for r in decoded] == [4681, 4681 + 32766, 0, 0, 0, 4681 + 32767, 4681]
    assert f["bai"] == ref.bai_bytes(*ref.expected_index(decoded, [ln for _, ln in refs]))
    index = ref.bai_parse(f["bai"])[0]
    assert len(index[0][1]) == ((top - 101 + 300010 - 1) >> 14) + 1 > 1 << 15 and len(index[1][1]) == (1 << 15) + 1
    with open(sam, "a") as fh:
        fh.write("\t".join(["h", "0", "long", str(top + 1), "30", "4M", "*", "0", "0", "ACGT", "*"]) + "\n")   # POS 2^29 + 1: the parser's refusal
    with pytest.raises(NprError):
        gpu_ctx.sam_to_bam(sam, str(tmp_path / "refused.bam"))
    for region, names in (((0, top - 1, top), ["b", "c"]), ((0, top - 20001, top - 19999), ["g"]), ((1, top - 1, top), ["d", "e"]), ((2, 0, 1000), ["f"])):
        want = ref.brute_overlaps(decoded, *region)
        assert [decoded[i]["line"].split("\t")[0] for i in want] == names
        assert ref.bai_query_tid(index, decoded, ref.records_of_tid(decoded), *region) == want
        with gpu_ctx.bam_open(f["data"], index=f["bai"], region=region) as s:
            assert _sam(s)[1] == [decoded[i]["line"] for i in want], region

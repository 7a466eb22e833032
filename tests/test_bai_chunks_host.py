"""npr_bai_chunks (include/nprealign.h, "region queries"; csrc/npr_bam_host.cpp) without a GPU: the chunks of a few hundred regions equal
the rule restated on bam_reference.bai_parse and reg2bins (tests/bam_region_cases.py chunks_rule) on the indices of two files -- this
project's stored layout and another writer's 4 KB blocks, both indexed by the specification's rules in Python --, every record that overlaps
lies in a returned chunk, and malformed and truncated images are refused.  The same cases go through csrc/npr_bam_host.cpp built as a
stand-alone program with AddressSanitizer and UBSan (tests/native/bai_chunks_check.cpp).  Nothing is loaded into Python under a sanitizer."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import bam_reference as ref
import bam_region_cases as cases
from nanopore_amd import _lib, bam

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = [ln for _, ln in cases.REFS]


@pytest.fixture(scope="module")
def files():
    """name -> dict(bai, decoded, blocks, stream_len): computed once and never changed"""
    stream = cases.sorted_stream()
    assert len(stream) > 4 * ref.P
    _, refs, decoded = ref.bam_decode(stream, any_writer=True)
    assert refs == cases.REFS and len(decoded) >= 400
    out = {}
    for name, blocks in (("stored", cases.stored_blocks(len(stream))), ("foreign", cases.bgzf_blocks(cases.rebgzf(stream)))):
        out[name] = dict(bai=cases.spec_index(decoded, REF_LEN, blocks, len(stream)), decoded=decoded, blocks=blocks, stream_len=len(stream))
    index, _ = ref.bai_parse(out["stored"]["bai"])
    levels = {next(lv for lv, first in enumerate((0, 1, 9, 73, 585, 4681, 37450)) if b < first) for b in index[0][0] if b != 37450}
    assert {4, 5, 6} <= levels, "bins of three levels"   # (of 2^20, 2^17 and 2^14 positions)
    assert not index[2][0] and not index[2][1], "the last reference has no record"
    assert sum(r["u0"] // ref.P != (r["u1"] - 1) // ref.P for r in decoded) >= 4, "records straddle block boundaries"
    return out


def _call(bai, tid, beg, end, cap=None):
    """-> (return value, n_ref or -1, the chunks written)"""
    L = _lib.load()
    bai = np.frombuffer(bytes(bai), dtype=np.uint8)
    n_ref = C.c_int64(-1)
    if cap is None:
        return int(L.npr_bai_chunks(_lib.ptr(bai), len(bai), tid, beg, end, None, None, 0, C.byref(n_ref))), n_ref.value, []
    cb, ce = np.full(cap + 1, 7, dtype=np.uint64), np.full(cap + 1, 7, dtype=np.uint64)
    rc = int(L.npr_bai_chunks(_lib.ptr(bai), len(bai), tid, beg, end, _lib.ptr(cb), _lib.ptr(ce), cap, C.byref(n_ref)))
    return rc, n_ref.value, list(zip(cb[:max(rc, 0)].tolist(), ce[:max(rc, 0)].tolist()))


@pytest.mark.parametrize("name", ("stored", "foreign"))
def test_chunks_equal_the_restated_rule_and_hold_every_overlapping_record(files, name):
    f = files[name]
    regions = cases.host_regions()
    assert len(regions) > 300
    merged = dropped = 0
    for tid, beg, end in regions:
        want = cases.chunks_rule(f["bai"], tid, beg, end)
        got, n_ref = bam.bai_chunks(f["bai"], tid, beg, end)
        assert n_ref == 3 and [tuple(int(v) for v in c) for c in got] == want, (tid, beg, end)
        assert all(a[1] < b[0] for a, b in zip(want, want[1:])), "disjoint and ascending"
        for i in ref.brute_overlaps(f["decoded"], tid, beg, end):
            v0 = ref.voffset_by_walking(f["blocks"], f["decoded"][i]["u0"], f["stream_len"])
            assert any(c[0] <= v0 < c[1] for c in want), (tid, beg, end, i)
        index, _ = ref.bai_parse(f["bai"])
        raw = [c for b in ref.reg2bins(beg, end) if b in index[tid][0] for c in index[tid][0][b]]
        linear = index[tid][1]
        low = linear[min(beg >> 14, len(linear) - 1)] if linear else 0
        kept = [c for c in raw if c[1] > low]
        merged += len(kept) > len(want)
        dropped += len(raw) > len(kept)
    assert merged > 10 and dropped > 10, "the merge and the lower bound are in play"
    assert bam.bai_chunks(f["bai"], 2, 0, 5000)[0].shape == (0, 2) and bam.bai_chunks(f["bai"], 0, 290000, 300000)[0].shape[1] == 2


def test_the_count_the_capacity_and_the_arguments(files):
    bai = files["stored"]["bai"]
    region = (0, 100000, 103000)   # (the bins of its windows, and those of the records with an N run that reach it from far before)
    want = cases.chunks_rule(bai, *region)
    assert len(want) >= 2
    assert _call(bai, *region) == (len(want), 3, [])
    assert _call(bai, *region, cap=len(want)) == (len(want), 3, want)
    assert _call(bai, *region, cap=len(want) - 1) == (_lib.ERR_CAPACITY, 3, [])
    for tid, beg, end in ((-1, 0, 10), (3, 0, 10), (0, -1, 10), (0, 10, 10), (0, 11, 10), (0, 0, (1 << 29) + 1)):
        assert _call(bai, tid, beg, end, cap=64) == (_lib.ERR_INVALID, 3, []), (tid, beg, end)   # (n_ref is set: the header was read)
    assert _call(bai, 0, (1 << 29) - 1, 1 << 29, cap=64)[0] >= 0
    assert _call(b"BAJ\1" + bai[4:], 0, 0, 10, cap=64) == (_lib.ERR_INVALID, -1, [])


# ---------------------------------------------------------------- malformed images
def small_index():
    """a few records on three references: every length of its image can be tried"""
    recs = [dict(tid=0, pos=100, end=400, flag=0), dict(tid=0, pos=16000, end=17000, flag=0), dict(tid=0, pos=40000, end=40300, flag=16),
            dict(tid=1, pos=5, end=300, flag=0), dict(tid=1, pos=20000, end=20300, flag=4), dict(tid=-1, pos=-1, end=0, flag=4)]
    at = 200
    for r in recs:
        r["u0"], r["u1"] = at, at + 350
        at += 350
    return cases.spec_index(recs, REF_LEN, [(0, 0, at)], at)


def malformed():
    """-> [(what, image, accepted)]: every prefix of the small index, and the image with one count bent"""
    bai = small_index()
    index, no_coor = ref.bai_parse(bai)
    assert no_coor == 1 and len(bai) < 600
    out = [("cut at %d" % n, bai[:n], n in (len(bai) - 8, len(bai))) for n in range(len(bai) + 1)]
    # where the counts lie: n_ref at 4, then per reference n_bin, (bin, n_chunk, chunks), n_intv
    at, places = 8, []
    for bins, linear in index:
        places.append(("n_bin", at))
        at += 4
        for b in bins:
            places.append(("n_chunk", at + 4))
            places.append(("chunk", at + 8) if b != 37450 else ("pseudo", at + 8))
            at += 8 + 16 * len(bins[b])
        places.append(("n_intv", at))
        at += 4 + 8 * len(linear)
    assert at + 8 == len(bai)
    for what, p in [("n_ref", 4)] + places:
        if what in ("chunk", "pseudo"):
            beg, end = struct.unpack_from("<QQ", bai, p)
            bent = bai[:p] + struct.pack("<QQ", end + 1, beg) + bai[p + 16:]      # end < beg: refused in a bin, nothing in the pseudo-bin
            out.append(("%s at %d with end < beg" % (what, p), bent, what == "pseudo"))
            continue
        for v in (-1, -(1 << 31), (1 << 31) - 1, 1 << 20):
            out.append(("%s at %d = %d" % (what, p, v), bai[:p] + struct.pack("<i", v) + bai[p + 4:], False))
    return bai, out


def test_truncated_and_bent_images_are_refused(files):
    bai, items = malformed()
    assert len(items) > len(bai) + 40
    want = cases.chunks_rule(bai, 0, 0, 20000)
    assert len(want) >= 1
    for what, image, accepted in items:
        rc, n_ref, chunks = _call(image, 0, 0, 20000, cap=16)
        if accepted:
            assert (rc, n_ref, chunks) == (len(want), 3, want), what
        else:
            assert rc == _lib.ERR_INVALID and chunks == [], what
    big = files["foreign"]["bai"]
    for n in list(range(0, 64)) + list(range(len(big) - 40, len(big))) + list(range(64, len(big), 97)):   # a large image cut in many places
        assert _call(big[:n], 0, 0, 300000, cap=4096)[0] == (_lib.ERR_INVALID if n != len(big) - 8 else len(cases.chunks_rule(big, 0, 0, 300000))), n


# ---------------------------------------------------------------- the same under a sanitizer, as a program of its own
@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("baichunks") / "bai_chunks_check")
    csrc = os.path.join(ROOT, "nanopore_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           "-I", csrc, os.path.join(ROOT, "tests", "native", "bai_chunks_check.cpp"), os.path.join(csrc, "npr_bam_host.cpp"), "-o", exe, "-lpthread"])

    def run(items):
        """items: [(tid, beg, end, image)] -> [(return value, n_ref, [(beg, end)])]"""
        path = exe + ".cases"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<I", len(items)))
            for tid, beg, end, image in items:
                fh.write(struct.pack("<iqqI", tid, beg, end, len(image)) + bytes(image))
        out = subprocess.run([exe, path], capture_output=True, text=True)
        lines = out.stdout.split("\n")
        assert out.returncode == 0 and lines[len(items)] == "bai_chunks_check ok", out.stdout[-2000:] + out.stderr[-4000:]
        rows = [[int(v) for v in line.split()] for line in lines[:len(items)]]
        assert [r[0] for r in rows] == list(range(len(items)))
        return [(r[1], r[2], list(zip(r[3::2], r[4::2]))) for r in rows]
    return run


def test_the_program_under_the_sanitizers_agrees(files, check):
    items, want = [], []
    for name in ("stored", "foreign"):
        for tid, beg, end in cases.host_regions():
            items.append((tid, beg, end, files[name]["bai"]))
            chunks = cases.chunks_rule(files[name]["bai"], tid, beg, end)
            want.append((len(chunks), 3, chunks))
    bai, bent = malformed()
    good = cases.chunks_rule(bai, 0, 0, 20000)
    for what, image, accepted in bent:
        items.append((0, 0, 20000, image))
        want.append((len(good), 3, good) if accepted else (_lib.ERR_INVALID, None, []))
    for tid, beg, end in ((-1, 0, 10), (3, 0, 10), (0, 10, 10), (0, 0, (1 << 29) + 1)):
        items.append((tid, beg, end, bai))
        want.append((_lib.ERR_INVALID, 3, []))
    got = check(items)
    assert len(items) > 700
    for g, w, item in zip(got, want, items):
        assert g[0] == w[0] and g[2] == w[2] and (w[1] is None or g[1] == w[1]), item[:3]

"""csrc/npr_inflate.h (the inflate core the device kernel k_bgzf_inflate runs) on the host: tests/native/inflate_check.cpp, a stand-alone
program built with AddressSanitizer and UBSan, on a case file written here (tests/inflate_cases.py).  Accepted: every payload compressed by
zlib every way, and hand-made deflate data zlib accepts.  Refused: one case for every refusal the core lists, each first shown to be
refused by zlib.decompressobj(-15) itself -- it raises or does not end exactly there -- so no case is one zlib would accept.  No GPU."""
import os
import struct
import subprocess
import zlib

import pytest

import inflate_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("inflate") / "inflate_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "nanopore_amd", "csrc"), os.path.join(ROOT, "tests", "native", "inflate_check.cpp"), "-o", exe])

    def run(items):
        """items: [(body, isize, crc)] -> [(status name, produced, crc)]"""
        path = exe + ".cases"
        with open(path, "wb") as fh:
            fh.write(struct.pack("<I", len(items)))
            for body, isize, crc in items:
                fh.write(struct.pack("<III", len(body), isize, crc & 0xffffffff) + body)
        out = subprocess.run([exe, path], capture_output=True, text=True)
        lines = out.stdout.split("\n")
        assert out.returncode == 0 and lines[len(items)] == "inflate_check ok", out.stdout[-2000:] + out.stderr[-4000:]
        rows = [tuple(int(v) for v in line.split()) for line in lines[:len(items)]]
        assert [r[0] for r in rows] == list(range(len(items)))
        return [(cases.STATUS[r[1]], r[2], r[3]) for r in rows]
    return run


def test_accepts_what_zlib_writes_and_what_it_accepts(check):
    items = cases.accepted()
    assert len(items) == 14 * 9 + 6
    for name, body, payload in items:
        assert cases.zlib_accepts(body, len(payload), zlib.crc32(payload)), name
    kinds = set()
    for name, body, payload in items:   # (what the cases are meant to hold is in them)
        kinds.add((body[0] >> 1) & 3)
    assert kinds == {0, 1, 2}
    got = check([(body, len(payload), zlib.crc32(payload)) for _, body, payload in items])
    for (name, body, payload), (status, produced, crc) in zip(items, got):
        assert (status, produced, crc) == ("OK", len(payload), zlib.crc32(payload)), name


def test_refuses_what_zlib_refuses(check):
    items = cases.refusals()
    assert {v[3] for v in items.values()} == set(cases.STATUS) - {"OK", "BOUND"}   # every refusal of the core has a case
    for name, (body, isize, crc, _) in items.items():
        assert not cases.zlib_accepts(body, isize, crc), name
    got = check([(body, isize, crc) for body, isize, crc, _ in items.values()])
    for (name, (body, isize, crc, want)), (status, produced, _) in zip(items.items(), got):
        assert status == want, (name, status)
        assert produced <= isize, name


def test_refuses_a_stream_cut_anywhere(check):
    """The BAM-like payload at level 6 (dynamic blocks) and as fixed blocks, cut after every one of its first 700 bytes (inside the dynamic
    header, the code lengths and the symbols) and a few places later: zlib does not end on any of them, and neither does the core."""
    payload = cases.payloads()["bam-like"][:20000]
    items = []
    for way in ("level 6", "fixed", "level 0"):
        body = cases.WAYS[way](payload)
        for cut in list(range(0, 700)) + [len(body) // 2, len(body) - 2, len(body) - 1]:
            items.append((body[:cut], len(payload), zlib.crc32(payload)))
    for body, isize, crc in items[::97]:
        assert not cases.zlib_accepts(body, isize, crc)
    for status, produced, _ in check(items):
        assert status == "INPUT" and produced <= len(payload)

"""Chaining of seed rows on the device (csrc/npr_seedchain.hip behind npr_seed_chains) and the SeedMapper classes that use it.
The expectation is tests/seed_chain_reference.py (pinned without a device by test_seed_chain_host.py); everything is compared as
exact integers or bytes."""
import os
import random

import numpy as np
import pytest

from helpers import ROOT
from seed_chain_reference import M, as_chains, chains_by_host, chains_by_rule, hand_made_cases, pack, spans
from seed_mapper import revcomp

pytestmark = pytest.mark.gpu

C1 = os.path.join(ROOT, "tests", "golden", "c1")
GUARD = 0x5a5a5a5a
NAMES = ["tile_edges", "two_long_runs", "gap_exact", "gap_zero", "long_early_block", "equal_predecessors", "equal_ends", "adjacent_on_a_diagonal",
         "touching_the_ends", "overlapping", "three_references", "strand_choice", "no_reads", "no_rows"]


@pytest.fixture(scope="module")
def cases():
    made = hand_made_cases()
    assert sorted(made) == sorted(NAMES)
    return made


def _check(got, want, read_len, ref_len):
    assert got == want
    for i, mine in enumerate(got):
        for r, strand, score, rows, guide in mine:
            assert spans(guide) == (ref_len[r], read_len[i]) and score == sum(n for op, n in guide if op == M)


@pytest.mark.parametrize("name", NAMES)
def test_hand_made_rows(gpu_ctx, cases, name):
    """What each case is for: hand_made_cases and test_seed_chain_host.test_the_cases_show_what_they_were_made_for."""
    read_len, ref_len, hit_off, hits, max_gap = cases[name]
    out = gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, max_gap)
    assert len(out[0]) == len(read_len) + 1 and out[0][-1] == len(out[1]) == len(out[2]) - 1 and out[2][-1] == len(out[3]) and out[2][0] == 0
    _check(as_chains(*out), chains_by_rule(read_len, ref_len, hit_off, hits, max_gap), read_len, ref_len)


def test_all_cases_in_one_call(gpu_ctx, cases):
    """The reads of every case with max_gap 200 as one call: hundreds of wavefronts, chains of every length side by side."""
    reads, ref_len, want = [], [], []
    for name in NAMES:
        read_len, rl, hit_off, hits, max_gap = cases[name]
        if max_gap != 200:
            continue
        for i in range(len(read_len)):
            rows = hits[hit_off[i]:hit_off[i + 1]].copy()
            rows[:, 0] += len(ref_len)
            reads.append((read_len[i], rows))
        want += [[(c[0] + len(ref_len),) + tuple(c[1:]) for c in mine] for mine in chains_by_rule(read_len, rl, hit_off, hits, 200)]
        ref_len += list(rl)
    read_len = np.array([n for n, _ in reads], dtype=np.int64)
    hit_off = np.zeros(len(reads) + 1, dtype=np.int64)
    np.cumsum([len(rows) for _, rows in reads], out=hit_off[1:])
    hits = np.concatenate([rows for _, rows in reads])
    got = as_chains(*gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, 200))
    assert sum(len(m) for m in got) >= 30
    _check(got, want, read_len, ref_len)


def _spans(reads):
    text, begin, end = b"", [], []
    for r in reads:
        text += b"\n@x\n"
        begin.append(len(text))
        text += r.encode()
        end.append(len(text))
    return np.frombuffer(text + b"\n", dtype=np.uint8), np.array(begin, dtype=np.int64), np.array(end, dtype=np.int64)


def test_a_homopolymer_run_of_a_thousand_rows(gpu_ctx):
    """A * 40 against A * 1000: every position of the run starts a match, the real index makes about a thousand rows of one run (16
    tiles), nearly all overlapping one another."""
    refs, reads = ["C" + "A" * 1000 + "G"], ["A" * 40, "ACGTACGTAGCTAGCTAGGATCGATCGAT"]
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index(refs, 12)
    try:
        hit_off, hits = index.matches(text, begin, end, 20, 3)
    finally:
        index.close()
    assert 900 <= hit_off[1] <= 1100 and hit_off[2] == hit_off[1]
    read_len, ref_len = end - begin, [len(refs[0])]
    want = chains_by_rule(read_len, ref_len, hit_off, hits, 200)
    assert want == chains_by_host(read_len, ref_len, hit_off, hits, 200)
    _check(as_chains(*gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, 200)), want, read_len, ref_len)


def test_200_reads_against_a_megabase(gpu_ctx):
    """Reads of about 2 kb through an error channel, either strand, against a random megabase (as test_gpu_seed's megabase fixture makes
    them): SeedIndex.matches, then seed_chains; every chain is the helper's."""
    rng = random.Random(23)
    ref = "".join(rng.choice("ACGT") for _ in range(1000000))
    reads = []
    for i in range(200):
        s = rng.randrange(0, len(ref) - 2100)
        out = []
        for c in ref[s:s + rng.randrange(1800, 2200)]:
            r = rng.random()
            if r < 0.05:
                out.append(rng.choice("ACGT"))
            elif r < 0.08:
                continue
            elif r < 0.11:
                out.append(c)
                out.append(rng.choice("ACGT"))
            else:
                out.append(c)
        reads.append(revcomp("".join(out)) if i % 2 else "".join(out))
    text, begin, end = _spans(reads)
    index = gpu_ctx.seed_index([ref], 16)
    try:
        hit_off, hits = index.matches(text, begin, end, 20, 3)
    finally:
        index.close()
    assert len(hits) >= 1000
    read_len, ref_len = end - begin, [len(ref)]
    got = as_chains(*gpu_ctx.seed_chains(read_len, ref_len, hit_off, hits, 200))
    _check(got, chains_by_rule(read_len, ref_len, hit_off, hits, 200), read_len, ref_len)
    assert sum(len(m) for m in got) >= 190 and sum(1 for i, m in enumerate(got) if m and m[0][1] == i % 2) >= 190 and max(m[0][3] for m in got if m) >= 5


def _raw(ctx, case, cap_chains, cap_ops, max_gap=None):
    """npr_seed_chains as it stands: (return value, chain_off, chains, ops_off, ops), a guard row behind every buffer"""
    from nanopore_amd._lib import ptr
    read_len, ref_len, hit_off, hits, gap = case
    chain_off = np.full(len(read_len) + 1, -7, dtype=np.int64)
    chains = np.full((cap_chains + 1, 4), GUARD, dtype=np.int32)
    ops_off = np.full(cap_chains + 2, -7, dtype=np.int64)
    ops = np.full((cap_ops + 1, 2), GUARD, dtype=np.int32)
    rc = ctx._L.npr_seed_chains(ctx._h, gap if max_gap is None else max_gap, len(read_len), ptr(read_len), len(ref_len), ptr(ref_len), ptr(hit_off), ptr(hits),
                                ptr(chain_off), ptr(chains), cap_chains, ptr(ops_off), ptr(ops), cap_ops)
    return rc, chain_off, chains, ops_off, ops


def test_capacity(gpu_ctx, cases):
    from nanopore_amd import _lib
    case = cases["tile_edges"]
    want_off, want_chains, want_ops_off, want_ops = gpu_ctx.seed_chains(*case)
    m, p = len(want_chains), len(want_ops)
    assert m == 9 and p > 50 and p <= 3 * len(case[3]) + 2 * m
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, case, m - 1, p)            # one chain too few: the chain offsets and nothing else
    assert rc == _lib.ERR_CAPACITY and (off == want_off).all() and (chains == GUARD).all() and (ops_off == -7).all() and (ops == GUARD).all()
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, case, m, p - 1)            # one op pair too few: ops_off[0] says how many
    assert rc == _lib.ERR_CAPACITY and (off == want_off).all() and (chains == GUARD).all() and ops_off[0] == p and (ops_off[1:] == -7).all() and (ops == GUARD).all()
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, case, m, p)                # exact
    assert rc == m and (off == want_off).all() and (chains[:m] == want_chains).all() and (chains[m] == GUARD).all()
    assert (ops_off[:m + 1] == want_ops_off).all() and ops_off[m + 1] == -7 and (ops[:p] == want_ops).all() and (ops[p] == GUARD).all()
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, case, 3 * m, 3 * p)        # generous
    assert rc == m and (off == want_off).all() and (chains[:m] == want_chains).all() and (chains[m:] == GUARD).all()
    assert (ops_off[:m + 1] == want_ops_off).all() and (ops_off[m + 1:] == -7).all() and (ops[:p] == want_ops).all() and (ops[p:] == GUARD).all()
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, cases["no_rows"], 4, 4)     # no chain at all: 0, and the offsets say so
    assert rc == 0 and (off == 0).all() and ops_off[0] == 0 and (ops_off[1:] == -7).all() and (chains == GUARD).all() and (ops == GUARD).all()


def test_invalid_rows_are_refused_before_anything_is_written(gpu_ctx):
    """Refused inputs, validated on the host before any kernel indexes with them: the call returns NPR_ERR_INVALID and leaves every
    output as it was."""
    from nanopore_amd import _lib
    good = [(0, 5, 5, 0, 10), (0, 30, 30, 0, 10), (1, 2, 2, 0, 4), (0, 7, 7, 1, 3)]
    read_len, hit_off, hits = pack([(50, good), (20, [])])
    ref_len = np.array([60, 40], dtype=np.int64)
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, (read_len, ref_len, hit_off, hits, 200), 8, 64)
    assert rc == 2 and list(off) == [0, 2, 2]

    def refused(rows=hits, rl=read_len, fl=ref_len, ho=hit_off, max_gap=200):
        rc, off, chains, ops_off, ops = _raw(gpu_ctx, (rl, fl, ho, np.ascontiguousarray(rows), max_gap), 8, 64)
        return rc == _lib.ERR_INVALID and (off == -7).all() and (chains == GUARD).all() and (ops_off == -7).all() and (ops == GUARD).all()

    def changed(row, col, value):
        rows = hits.copy()
        rows[row, col] = value
        return rows

    assert refused(rows=hits[[1, 0, 2, 3]])              # out of (a, b) order
    assert refused(rows=hits[[0, 1, 3, 2]])              # the reverse strand before the forward one
    assert refused(rows=hits[[2, 0, 1, 3]])              # references out of order
    assert refused(rows=changed(1, 3, 21))               # past its read's end (30 + 21 > 50)
    assert refused(rows=changed(2, 3, 39))               # past its reference's end (2 + 39 > 40) though inside the read
    assert refused(rows=changed(3, 3, 44))               # the same on the reverse strand (7 + 44 > 50)
    assert refused(rows=changed(0, 3, 0))                # L = 0
    assert refused(rows=changed(0, 3, -3))
    assert refused(rows=changed(0, 1, -1))               # a < 0
    assert refused(rows=changed(2, 0, 2))                # a reference the call does not have
    assert refused(rows=changed(0, 0, -1))
    assert refused(max_gap=-1)
    assert refused(ho=np.array([1, 4, 4], dtype=np.int64))                                     # offsets that do not start at 0
    assert refused(ho=np.array([0, 4, 3], dtype=np.int64))                                     # ... or decrease
    assert refused(rl=np.array([50, -1], dtype=np.int64))
    assert refused(fl=np.array([60, 1 << 31], dtype=np.int64))
    rc, off, chains, ops_off, ops = _raw(gpu_ctx, (read_len, ref_len, hit_off, hits, 200), 8, 64)   # and the context is as good as before
    assert rc == 2 and list(off) == [0, 2, 2]


# ---- end to end: the SeedMapper classes ----

def _chain_both_ways(tmp, fq, fa, k, min_len, monkeypatch):
    """(what utils.chainSamFile makes of plain SeedMapper's output, what SeedMapperChain writes) with the record-at-a-time chainSamFile out of
    SeedMapperChain's reach"""
    from nanopore_amd.analyses import utils
    from nanopore_amd.mappers import abstractMapper
    from nanopore_amd.mappers import variants as V
    plain, want, out = str(tmp / "plain.sam"), str(tmp / "want.sam"), str(tmp / "chained.sam")
    mapper = V.SeedMapper(fq, "2D", fa, plain)
    mapper.k, mapper.minLength = k, min_len
    mapper.run()
    mapper.cleanup()
    utils.chainSamFile(plain, want, fq, fa)

    def never(*args, **kwargs):
        raise AssertionError("SeedMapperChain went through the record-at-a-time chainSamFile")

    monkeypatch.setattr(abstractMapper, "chainSamFile", never)
    mapper = V.SeedMapperChain(fq, "2D", fa, out)
    mapper.k, mapper.minLength = k, min_len
    mapper.run()
    mapper.cleanup()
    return open(want, "rb").read(), open(out, "rb").read()


def test_seed_mapper_chain_on_c1(gpu_ctx, tmp_path, monkeypatch):
    from nanopore_amd import bioio
    fq = str(tmp_path / "reads.fq")
    with open(fq, "w") as fh:
        for n, s, _ in bioio.fastqRead(os.path.join(C1, "reads.fq")):
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    want, got = _chain_both_ways(tmp_path, fq, os.path.join(C1, "reference.fa"), 18, 24, monkeypatch)
    assert got == want and got.count(b"\n") >= 3


def test_seed_mapper_chain_on_two_references_and_both_strands(gpu_ctx, tmp_path, monkeypatch):
    rng = random.Random(41)
    refs = ["".join(rng.choice("ACGT") for _ in range(n)) for n in (3000, 1800)]
    reads = []
    for i in range(12):
        ref = refs[i % 2]
        s = rng.randrange(0, len(ref) - 700)
        piece = list(ref[s:s + rng.randrange(400, 700)])
        for q in range(rng.randrange(5, 30), len(piece), rng.randrange(25, 60)):   # a substitution, a deletion or an insertion every few dozen bases
            kind = rng.randrange(3)
            piece[q] = "ACGT"[("ACGT".index(piece[q]) + 1) % 4] if kind == 0 else ("" if kind == 1 else piece[q] + rng.choice("ACGT"))
        read = "".join(piece)
        if i == 5:
            read = read.lower()
        if i == 7:
            read = read[:200] + refs[0][100:400]                                     # a read with chains on both references
        reads.append(revcomp(read) if i % 3 == 1 else read)
    reads.append("".join(rng.choice("ACGT") for _ in range(300)))                    # a read that matches nothing
    fa, fq = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq")
    with open(fa, "w") as fh:
        for k, ref in enumerate(refs):
            fh.write(">contig_%d some description\n%s\n" % (k, ref))
    with open(fq, "w") as fh:
        for i, r in enumerate(reads):
            fh.write("@r%02d extra words\n%s\n+\n%s\n" % ((7 * i) % 13, r, "I" * len(r)))
    want, got = _chain_both_ways(tmp_path, fq, fa, 12, 14, monkeypatch)
    assert got == want
    flags = [rec.split(b"\t")[1] for rec in got.split(b"\n")[2:-1]]
    assert len(flags) >= 13 and flags.count(b"16") >= 4 and flags.count(b"0") >= 8

"""The chain stage of the seed mapper without a device: the new entry points exist, the expectation the GPU tests compare against is
pinned (its two independent statements agree, and say what each hand-made case was made to show), and the host formatter
npr_seed_chain_sam_text writes, byte for byte, what utils.chainSamFile writes from the equivalent local-hit records."""
import numpy as np
import pytest

from seed_chain_reference import D, I, M, chains_by_host, chains_by_rule, hand_made_cases, pack, spans


def test_the_new_symbols_exist_and_are_bound():
    from nanopore_amd import _lib
    L = _lib.load()
    for name in ("npr_seed_chains", "npr_seed_chain_sam_text"):
        assert name in _lib.EXPORTS and hasattr(L, name)
        assert getattr(L, name).restype is _lib.C.c_int64
    assert len(L.npr_seed_chains.argtypes) == 14 and len(L.npr_seed_chain_sam_text.argtypes) == 15
    from nanopore_amd import realign
    assert callable(realign.Context.seed_chains) and callable(realign.seed_chain_sam_text)


@pytest.fixture(scope="module")
def cases():
    return hand_made_cases()


def test_the_two_statements_of_the_rule_agree(cases):
    n_chains = 0
    for name, (read_len, ref_len, hit_off, hits, max_gap) in cases.items():
        want = chains_by_rule(read_len, ref_len, hit_off, hits, max_gap)
        assert want == chains_by_host(read_len, ref_len, hit_off, hits, max_gap), name
        for i, mine in enumerate(want):
            assert [c[0] for c in mine] == sorted(set(int(r) for r in hits[hit_off[i]:hit_off[i + 1], 0])), name
            for r, strand, score, rows, guide in mine:
                assert spans(guide) == (ref_len[r], read_len[i]) and score == sum(n for op, n in guide if op == M), name
                assert all(n > 0 for _, n in guide) and all(x[0] != y[0] for x, y in zip(guide, guide[1:])), name
                n_chains += 1
    assert n_chains >= 30


def test_the_cases_show_what_they_were_made_for(cases):
    def of(name):
        read_len, ref_len, hit_off, hits, max_gap = cases[name]
        return chains_by_rule(read_len, ref_len, hit_off, hits, max_gap)

    assert [len(mine) for mine in of("tile_edges")] == [2, 0, 1, 2, 1, 1, 2]
    assert [mine[0][3] for mine in of("gap_exact")] == [2, 1, 2, 1]      # a gap sum of max_gap chains, one more does not
    assert of("gap_zero")[0][0][2:4] == (10, 1)
    assert of("long_early_block")[0][0][2:] == (5010, 2, [(M, 5000), (D, 50), (I, 50), (M, 10), (D, 940), (I, 1940)])
    for mine in of("equal_predecessors"):                                  # the block at a = 0, b = 10 precedes, not the one at a = 2, b = 0
        assert mine[0][2:4] == (10, 2) and mine[0][4][:3] == [(I, 10), (M, 5), (D, 15)]
    ends = of("equal_ends")
    assert [(m[0][1], m[0][4][0]) for m in ends] == [(0, (D, 900)), (1, (D, 10)), (0, (D, 20)), (1, (D, 20)), (0, (D, 10))]
    assert of("adjacent_on_a_diagonal")[0][0][2:] == (14, 2, [(D, 5), (I, 7), (M, 14), (D, 21), (I, 29)])
    assert of("adjacent_on_a_diagonal")[1][0][2:] == (16, 3, [(D, 5), (I, 7), (M, 16), (D, 19), (I, 27)])
    touching = of("touching_the_ends")
    assert touching[0][0][4] == [(M, 30)] and touching[1][0][4] == [(M, 10), (D, 10), (I, 10), (M, 10)]
    assert touching[2][0][4] == [(M, 1), (D, 62), (I, 62), (M, 1)] and touching[3][0][4] == [(I, 10), (M, 30)] and touching[4][0][4] == [(D, 10), (M, 20)]
    assert [mine[0][3] for mine in of("overlapping")] == [1, 1, 1, 1, 1]
    assert [(c[0], c[1]) for c in of("three_references")[0]] == [(0, 1), (2, 1), (3, 0)]
    assert [(m[0][1], m[0][2]) for m in of("strand_choice")] == [(1, 18), (0, 18)]
    assert of("no_reads") == [] and of("no_rows") == [[], [], []]


# ---- the formatter ----

REFS = [("chrA", "ACGTTGCAAGGCTAGGATCCATGCAATCGGAGCTTAGCATCGATCGGATATCGCGCTAGCATCGAGGCTAGCTAGGCTATAGCGCTAGAGCTCTAGGATC"),
        ("chrB some words", "ttagcatcgatcggatatcgcgcGATTACAGATTACAGATTACATTTTGCGC")]
READS = [("zeta", "ACGTTGCAAGGCTAGGATCCATGCAATCGGAGCTTNGCATCGATC"),
         ("alpha with a description", "acgttgcaaggctaggatccATGCAATCGGAGCTTAGCATCGATCGGATATCGCG"),
         ("nothing_here", "GGGGGGGGGGGGGGGGGGGGGGGGGGG"),
         ("alph", "GATCCTAGAGCTCTAGCGCTATAGCCTAGCTAGCCTCGATGCTAGCGCGATATCC"),
         ("beta", "TTAGCATCGATCGGATATCGCGCGATTACAGATTACA")]
# rows (r, a, b, strand, L) per read: two references, both strands, a read on both references, a read without any
ROWS = [[(0, 0, 0, 0, 20), (0, 24, 24, 0, 11), (0, 36, 36, 0, 9)],
        [(0, 0, 0, 0, 20), (0, 20, 20, 0, 30), (1, 0, 32, 0, 12), (0, 60, 3, 1, 8)],
        [],
        [(0, 45, 0, 1, 25), (0, 72, 27, 1, 20), (0, 2, 2, 0, 4)],
        [(1, 0, 0, 1, 37), (1, 30, 1, 0, 6)]]


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from nanopore_amd import ingest
    d = tmp_path_factory.mktemp("seed_chain_text")
    fa, fq = str(d / "ref.fa"), str(d / "reads.fq")
    with open(fa, "w") as fh:
        for name, seq in REFS:
            fh.write(">%s\n%s\n" % (name, seq))
    with open(fq, "w") as fh:
        for name, seq in READS:
            fh.write("@%s\n%s\n+\n%s\n" % (name, seq, "I" * len(seq)))
    fat, fqt = ingest.FastaTable(fa), ingest.FastqTable(fq)
    assert fat.names == ["chrA", "chrB"] and [fqt.name(i) for i in range(len(fqt))] == [n.split()[0] for n, _ in READS]
    read_len, hit_off, hits = pack([(len(seq), rows) for (_, seq), rows in zip(READS, ROWS)])
    return d, fa, fq, fat, fqt, read_len, hit_off, hits


def _header(fat):
    return b"".join(("@SQ\tSN:%s\tLN:%d\n" % (name, n)).encode() for name, n in zip(fat.names, np.diff(fat.off)))


def _arrays(want):
    """chains_by_rule's lists -> (chain_off, chains, ops_off, ops)"""
    chain_off, chains, ops_off, ops = [0], [], [0], []
    for mine in want:
        for r, strand, score, rows, guide in mine:
            chains.append((r, strand, score, rows))
            ops += guide
            ops_off.append(len(ops))
        chain_off.append(len(chains))
    return (np.array(chain_off, dtype=np.int64), np.array(chains, dtype=np.int32).reshape(-1, 4), np.array(ops_off, dtype=np.int64),
            np.array(ops, dtype=np.int32).reshape(-1, 2))


def test_formatter_writes_what_chainSamFile_writes(files):
    from nanopore_amd import realign
    from nanopore_amd.analyses import utils
    d, fa, fq, fat, fqt, read_len, hit_off, hits = files
    begin, end = np.ascontiguousarray(fqt.seq_span[:, 0]), np.ascontiguousarray(fqt.seq_span[:, 1])
    names = [n.encode() for n in fat.names]
    local, _ = realign.seed_sam_text(fqt.text, fqt.name_span, begin, end, names, hit_off, hits)
    with open(str(d / "local.sam"), "wb") as fh:
        fh.write(_header(fat) + local.tobytes())
    utils.chainSamFile(str(d / "local.sam"), str(d / "chained.sam"), fq, fa)
    want = open(str(d / "chained.sam"), "rb").read()
    chains = chains_by_rule(read_len, np.diff(fat.off), hit_off, hits, 200)
    assert [len(mine) for mine in chains] == [1, 2, 0, 1, 1] and sorted(c[1] for mine in chains for c in mine) == [0, 0, 0, 1, 1]
    chain_off, rows, ops_off, ops = _arrays(chains)
    text, rec_off = realign.seed_chain_sam_text(fqt.text, fqt.name_span, begin, end, names, chain_off, rows, ops_off, ops)
    assert _header(fat) + text.tobytes() == want
    records = want[len(_header(fat)):].split(b"\n")[:-1]
    assert [rec.split(b"\t")[0] for rec in records] == [b"alph", b"alpha", b"zeta", b"alpha", b"beta"]   # by (reference, name as bytes)
    assert [int(rec_off[k + 1] - rec_off[k]) for k in range(len(records))] == [len(rec) + 1 for rec in records] and rec_off[0] == 0


def _raw(files, chain_off, chains, ops_off, ops, cap, name_span=None, guard=0x5a):
    from nanopore_amd import _lib
    from nanopore_amd.realign import _ragged
    d, fa, fq, fat, fqt, read_len, hit_off, hits = files
    begin, end = np.ascontiguousarray(fqt.seq_span[:, 0]), np.ascontiguousarray(fqt.seq_span[:, 1])
    rn, roff = _ragged([n.encode() for n in fat.names])
    rec_off = np.full(len(chains) + 1, -7, dtype=np.int64)
    out = np.full(max(cap, 0) + 8, guard, dtype=np.uint8)
    span = np.ascontiguousarray(fqt.name_span if name_span is None else name_span)
    p = _lib.ptr
    rc = _lib.load().npr_seed_chain_sam_text(len(begin), p(fqt.text), p(span), p(begin), p(end), p(rn), p(roff), len(fat.names), p(chain_off), p(chains), p(ops_off), p(ops),
                                             p(rec_off), p(out) if cap >= 0 else None, max(cap, 0))
    return rc, rec_off, out


def test_formatter_capacity_and_invalid_arguments(files):
    from nanopore_amd import _lib
    d, fa, fq, fat, fqt, read_len, hit_off, hits = files
    chain_off, chains, ops_off, ops = _arrays(chains_by_rule(read_len, np.diff(fat.off), hit_off, hits, 200))
    total, rec_off, _ = _raw(files, chain_off, chains, ops_off, ops, -1)          # out == NULL: the offsets and the length
    assert total > 0 and rec_off[0] == 0 and rec_off[-1] == total and (np.diff(rec_off) > 0).all()
    rc, off, out = _raw(files, chain_off, chains, ops_off, ops, total - 1)
    assert rc == _lib.ERR_CAPACITY and (off == rec_off).all() and (out == 0x5a).all()  # nothing written
    rc, off, out = _raw(files, chain_off, chains, ops_off, ops, total)
    assert rc == total and (out[total:] == 0x5a).all() and out[total - 1] == 10
    exact = out[:total].tobytes()
    rc, off, out = _raw(files, chain_off, chains, ops_off, ops, 2 * total)
    assert rc == total and out[:total].tobytes() == exact and (out[total:] == 0x5a).all()

    def refused(chain_off=chain_off, chains=chains, ops_off=ops_off, ops=ops, name_span=None):
        rc, off, out = _raw(files, chain_off, chains, ops_off, ops, total, name_span)
        return rc == _lib.ERR_INVALID and (out == 0x5a).all()

    twice = fqt.name_span.copy()
    twice[4] = twice[0]                                                            # two reads of one name
    assert refused(name_span=twice)
    bad = chains.copy()
    bad[0, 0] = 2                                                                  # a reference the list does not have
    assert refused(chains=bad)
    bad = chains.copy()
    bad[1, 1] = 2                                                                  # a strand that is neither
    assert refused(chains=bad)
    bad = ops.copy()
    bad[2, 0] = 9                                                                  # an operation outside MIDNSHP=X
    assert refused(ops=bad)
    bad = ops.copy()
    bad[2, 1] = -1
    assert refused(ops=bad)
    bad = ops_off.copy()
    bad[2] = bad[1] - 1
    assert refused(ops_off=bad)
    bad = chain_off.copy()
    bad[0] = 1
    assert refused(chain_off=bad)
    # no reads, and reads without a chain: legal, no records
    none = np.zeros(len(READS) + 1, dtype=np.int64)
    rc, off, out = _raw(files, none, chains[:0], ops_off[:1], ops[:0], 16)
    assert rc == 0 and off[0] == 0 and (out == 0x5a).all()


def test_without_a_run_the_inherited_chain_is_used(tmp_path):
    """A SeedMapper object whose run() was not called (the SAM came from elsewhere) chains through the inherited method."""
    from nanopore_amd.mappers import variants as V
    read_len, hit_off, hits = pack([(40, [(0, 0, 0, 0, 10), (0, 20, 20, 0, 10)])])
    fa, fq, out = str(tmp_path / "ref.fa"), str(tmp_path / "reads.fq"), str(tmp_path / "mapping.sam")
    open(fa, "w").write(">chr\n%s\n" % ("ACGT" * 10))
    open(fq, "w").write("@q\n%s\n+\n%s\n" % ("ACGT" * 10, "I" * 40))
    open(out, "w").write("@SQ\tSN:chr\tLN:40\nq\t0\tchr\t1\t255\t10M30H\t*\t0\t0\tACGTACGTAC\t*\nq\t0\tchr\t21\t255\t20H10M10H\t*\t0\t0\tACGTACGTAC\t*\n")
    mapper = V.SeedMapper(fq, "2D", fa, out)
    mapper.chainSamFile()
    mapper.cleanup()
    assert open(out).read().split("\n")[1].split("\t")[:6] == ["q", "0", "chr", "1", "255", "10M10D10I10M10D10I"]

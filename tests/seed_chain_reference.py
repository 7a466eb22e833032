"""What npr_seed_chains must return, stated twice and independently of the code under test (include/nprealign.h, "chaining of seed
rows"):

  chains_by_rule   the chaining rule and the guide as the header words them, all pairs, plain Python;
  chains_by_host   the host functions the record-at-a-time path uses, npr_chain_hits + npr_chain_merge, per (read, reference), fed
                   the signed read coordinates of utils._blockCoordinates.

Both give, per read, a list of (reference index, strand, score, rows in the chain, [(op, length), ...]) in ascending reference index;
as_chains() brings the arrays of the device call into the same form.  The hand-made row sets the CPU and the GPU tests share are
built here as well (hand_made_cases)."""
import random

import numpy as np

M, I, D = 0, 1, 2


def unpack(row):
    r, a, bs, n = (int(v) for v in row)
    bs &= 0xffffffff
    return r, a, bs & 0x7fffffff, bs >> 31, n


def pack(reads):
    """[(read length, [(r, a, b, strand, L), ...]), ...] -> (read_len, hit_off, hits) with every read's rows sorted by (strand, r, a, b)"""
    read_len = np.array([n for n, _ in reads], dtype=np.int64)
    hit_off = np.zeros(len(reads) + 1, dtype=np.int64)
    rows = []
    for i, (_, rs) in enumerate(reads):
        rs = sorted(rs, key=lambda t: (t[3], t[0], t[1], t[2]))
        rows += [(r, a, b | (s << 31), n) for r, a, b, s, n in rs]
        hit_off[i + 1] = len(rows)
    hits = np.array(rows, dtype=np.int64).reshape(-1, 4).astype(np.uint32).view(np.int32)
    return read_len, hit_off, np.ascontiguousarray(hits)


def _guide(blocks, ref_len, read_len):
    """a D then an I before every block, between blocks and after the last; zero lengths dropped; neighbours of one kind merged"""
    raw, x, y = [], 0, 0
    for a, b, n in blocks:
        raw += [(D, a - x), (I, b - y), (M, n)]
        x, y = a + n, b + n
    raw += [(D, ref_len - x), (I, read_len - y)]
    out = []
    for op, n in raw:
        assert n >= 0
        if n == 0:
            continue
        if out and out[-1][0] == op:
            out[-1] = (op, out[-1][1] + n)
        else:
            out.append((op, n))
    return out


def _by_reference(hits, lo, hi):
    """rows lo .. hi of one read -> {reference index: [(row number, a, b, strand, L), ...] in row order}"""
    groups = {}
    for q in range(lo, hi):
        r, a, b, s, n = unpack(hits[q])
        groups.setdefault(r, []).append((q, a, b, s, n))
    return groups


def chains_by_rule(read_len, ref_len, hit_off, hits, max_gap=200):
    out = []
    for i in range(len(read_len)):
        mine = []
        groups = _by_reference(hits, int(hit_off[i]), int(hit_off[i + 1]))
        for r in sorted(groups):
            rows = sorted(groups[r], key=lambda t: (t[1], t[3], t[2]))  # (a, strand, b); Python's sort is stable: row order among equals
            best, back = [], []
            for k, (_, a, b, s, n) in enumerate(rows):
                top, pick = 0, -1
                for j in range(k):  # every row that sorts before it
                    _, aj, bj, sj, nj = rows[j]
                    ej, fj = aj + nj - 1, bj + nj - 1
                    if sj == s and a > ej and b > fj and (a - ej) + (b - fj) <= max_gap and best[j] > top:
                        top, pick = best[j], j  # (strictly better only: the first-sorting one of equals stays)
                best.append(n + top)
                back.append(pick)
            end = 0
            for k in range(len(rows)):
                if best[k] >= best[end]:  # the last-sorting one of equals
                    end = k
            chain, k = [], end
            while k >= 0:
                chain.append(rows[k])
                k = back[k]
            chain.reverse()
            mine.append((r, chain[0][3], best[end], len(chain), _guide([(a, b, n) for _, a, b, _, n in chain], int(ref_len[r]), int(read_len[i]))))
        out.append(mine)
    return out


def chains_by_host(read_len, ref_len, hit_off, hits, max_gap=200):
    from nanopore_amd import _lib
    L = _lib.load()
    out = []
    for i in range(len(read_len)):
        mine = []
        groups = _by_reference(hits, int(hit_off[i]), int(hit_off[i + 1]))
        for r in sorted(groups):
            rows = groups[r]
            n = len(rows)
            a = np.array([t[1] for t in rows], dtype=np.int64)
            b = np.array([t[2] for t in rows], dtype=np.int64)
            rev = np.array([t[3] for t in rows], dtype=np.uint8)
            length = np.array([t[4] for t in rows], dtype=np.int64)
            signed = np.where(rev == 1, b - (int(read_len[i]) - 1), b)  # utils._blockCoordinates on a FLAG 16 record
            a_end, s_end = a + length - 1, signed + length - 1
            chain = np.zeros(n, dtype=np.int64)
            m = L.npr_chain_hits(n, _lib.ptr(a), _lib.ptr(signed), _lib.ptr(a_end), _lib.ptr(s_end), _lib.ptr(rev), _lib.ptr(length), max_gap, _lib.ptr(chain))
            assert m >= 1
            picked = chain[:m]
            ref_pos, read_pos = np.ascontiguousarray(a[picked]), np.ascontiguousarray(b[picked])
            ops_off = np.arange(m + 1, dtype=np.int64)
            ops = np.ascontiguousarray(np.stack([np.zeros(m, dtype=np.int32), length[picked].astype(np.int32)], axis=1))
            guide = np.zeros((3 * m + 2, 2), dtype=np.int32)
            k = L.npr_chain_merge(m, _lib.ptr(ref_pos), _lib.ptr(read_pos), _lib.ptr(ops_off), _lib.ptr(ops), int(ref_len[r]), int(read_len[i]), _lib.ptr(guide), len(guide))
            assert k >= 1
            mine.append((r, int(rev[picked[0]]), int(length[picked].sum()), int(m), [(int(op), int(v)) for op, v in guide[:k]]))
        out.append(mine)
    return out


def as_chains(chain_off, chains, ops_off, ops):
    out = []
    for i in range(len(chain_off) - 1):
        out.append([(int(chains[c, 0]), int(chains[c, 1]), int(chains[c, 2]), int(chains[c, 3]),
                     [(int(op), int(v)) for op, v in ops[int(ops_off[c]):int(ops_off[c + 1])]]) for c in range(int(chain_off[i]), int(chain_off[i + 1]))])
    return out


def spans(guide):
    return sum(n for op, n in guide if op != I), sum(n for op, n in guide if op != D)


def noisy_run(rng, n, r, strand, step=9):
    """n rows of reference r along a jittered diagonal, a few of them thrown far off it: most rows see a dozen candidates, equal
    scores are common (lengths 1 .. 6).  Returns (rows, reference positions used, read positions used)."""
    rows, a = [], 3
    for _ in range(n):
        a += rng.randrange(0, 2 * step)
        b = a + rng.randrange(-12, 13) + (rng.randrange(300, 900) if rng.random() < 0.1 else 0)
        rows.append((r, a, max(b, 0), strand, rng.randrange(1, 7)))
    return rows, a + 8, max(t[2] for t in rows) + 8 if rows else 8


def hand_made_cases():
    """{name: (read_len, ref_len, hit_off, hits, max_gap)}.  Every shape the device code treats differently: see the tests that name them."""
    cases = {}
    rng = random.Random(5)

    def one(name, ref_len, reads, max_gap=200):
        rl, off, hits = pack(reads)
        cases[name] = (rl, np.array(ref_len, dtype=np.int64), off, hits, max_gap)

    # runs of 0, 1, 2, 63, 64, 65 and 129 rows (a tile is 64 rows), one read each, on alternating strands; the read without rows lies between
    # reads that have some; a second reference carries a short run of the other strand for every third read
    reads, need_ref = [], [8, 8]
    for k, n in enumerate((1, 0, 2, 63, 64, 65, 129)):
        rows, ref_need, read_need = noisy_run(rng, n, 0, k & 1)
        if n and k % 3 == 0:
            more, ref1, read1 = noisy_run(rng, 5, 1, 1 - (k & 1))
            rows, read_need = rows + more, max(read_need, read1)
            need_ref[1] = max(need_ref[1], ref1)
        need_ref[0] = max(need_ref[0], ref_need)
        reads.append((read_need, rows))
    one("tile_edges", need_ref, reads)
    # both runs of one (read, reference) long enough to cross tiles, so that the choice between them sees ends in later tiles
    rows0, ref0, read0 = noisy_run(rng, 150, 0, 0)
    rows1, ref1, read1 = noisy_run(rng, 140, 0, 1)
    one("two_long_runs", [max(ref0, ref1)], [(max(read0, read1), rows0 + rows1)])

    # the second block starts 1 + g1 after the first ends in the reference and 1 + g2 in the read: gap sum exactly max_gap, and one more
    one("gap_exact", [400], [(400, [(0, 0, 0, 0, 10), (0, 9 + 30, 9 + 20, 0, 7)]), (400, [(0, 0, 0, 0, 10), (0, 9 + 31, 9 + 20, 0, 7)]),
                             (400, [(0, 0, 0, 1, 10), (0, 9 + 1, 9 + 49, 1, 7)]), (400, [(0, 0, 0, 1, 10), (0, 9 + 1, 9 + 50, 1, 7)])], max_gap=50)
    one("gap_zero", [100], [(100, [(0, 0, 0, 0, 10), (0, 10, 10, 0, 7)])], max_gap=0)
    # a block of 5000 that starts first and ends 51 before the last row starts; 100 rows that start later, end early and lie elsewhere in the
    # read come between: the last row (second tile) finds the long block only through the prefix maximum of the block ends
    one("long_early_block", [6000], [(7000, [(0, 0, 0, 0, 5000)] + [(0, 1 + k, 6000 + 2 * k, 0, 1) for k in range(100)] + [(0, 5050, 5050, 0, 10)])])
    # two predecessors of equal score: the one that sorts first wins; then the same with 64 rows of no consequence between them and the row that chooses
    one("equal_predecessors", [100, 100], [(1200, [(0, 0, 10, 0, 5), (0, 2, 0, 0, 5), (0, 20, 20, 0, 5)]),
                                           (1200, [(1, 0, 10, 0, 5), (1, 2, 0, 0, 5)] + [(1, 3, 1000 + 2 * k, 0, 1) for k in range(64)] + [(1, 20, 20, 0, 5)])])
    # equal chain ends: within a strand the later row; across strands the reverse row at the same a, the forward row when it starts later, the reverse row when it does
    one("equal_ends", [2000], [(2000, [(0, 10, 10, 0, 5), (0, 900, 900, 0, 5)]), (2000, [(0, 10, 10, 0, 5), (0, 10, 30, 1, 5)]),
                               (2000, [(0, 20, 10, 0, 5), (0, 10, 30, 1, 5)]), (2000, [(0, 10, 10, 0, 5), (0, 20, 30, 1, 5)]),
                               (2000, [(0, 10, 10, 0, 5), (0, 10, 10, 0, 5)])])
    one("adjacent_on_a_diagonal", [40], [(50, [(0, 5, 7, 0, 10), (0, 15, 17, 0, 4)]), (50, [(0, 5, 7, 1, 10), (0, 15, 17, 1, 4), (0, 19, 21, 1, 2)])])
    # blocks at position 0 and at the last base of read and reference: no empty D or I
    one("touching_the_ends", [30, 64], [(30, [(0, 0, 0, 0, 30)]), (30, [(0, 0, 0, 1, 10), (0, 20, 20, 1, 10)]), (64, [(1, 0, 0, 0, 1), (1, 63, 63, 0, 1)]),
                                        (40, [(0, 0, 10, 0, 30)]), (20, [(0, 10, 0, 0, 20)])])
    # overlapping blocks never chain: in both sequences, in the read only, in the reference only, one inside the other
    one("overlapping", [100], [(100, [(0, 0, 0, 0, 10), (0, 5, 5, 0, 10)]), (100, [(0, 0, 0, 0, 10), (0, 20, 5, 0, 10)]), (100, [(0, 0, 0, 0, 10), (0, 5, 20, 0, 10)]),
                               (100, [(0, 0, 0, 0, 30), (0, 10, 10, 0, 5)]), (100, [(0, 0, 0, 0, 10), (0, 10, 9, 0, 10)])])
    one("three_references", [300, 50, 300, 300], [(300, [(3, 10, 10, 0, 8), (3, 30, 30, 0, 8), (0, 100, 5, 1, 9), (2, 7, 7, 0, 3), (2, 50, 50, 1, 3), (0, 5, 100, 0, 4)])])
    # both strand runs present: the reverse chain scores more, then the forward one
    one("strand_choice", [500], [(500, [(0, 10, 10, 0, 8), (0, 30, 30, 0, 8), (0, 5, 5, 1, 9), (0, 40, 40, 1, 9)]),
                                 (500, [(0, 10, 10, 0, 9), (0, 30, 30, 0, 9), (0, 5, 5, 1, 8), (0, 40, 40, 1, 8)])])
    one("no_reads", [10], [])
    one("no_rows", [10], [(5, []), (0, []), (7, [])])
    return cases

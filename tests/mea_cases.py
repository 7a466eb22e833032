"""Constructed posterior pair lists for the MEA finish (csrc/npr_mea.hip, npr_host.cpp mea_cigar): every corner the kernels'
comments name, which the posteriors of real reads never reach.  A plain module (no conftest, nothing read from outside the
repository): cases() yields (name, lX, lY, x, y, p_float32, gap_gamma, match_gamma); tests/test_mea_cases_host.py runs them
through the host stage and the oracle, tests/test_gpu_mea_cases.py through the device stage.

The rule (oracle/realign_oracle.c orc_mea_cigar): q = floor(p * 1e7); weight w = q - floor(gap_gamma * (max(1e7 - rowsum, 0) +
max(1e7 - colsum, 0))); pairs with w > floor(match_gamma * 1e7) are kept; the heaviest chain of kept pairs strictly increasing in
x and y, ties to the pair that sorts last in (x, y) order, the empty chain first of all.

Every case: no (x, y) twice; at most 64 pairs on one read position (64 * 1.0000001e7 stays far inside the int32 the device sums a
column in); at most 64 pairs on one reference position, except e_group65.  Each case asserts AT GENERATION TIME, on replay() --
a walk in the kernels' visit order -- the property it is named for, so a case that stops hitting its corner fails loudly.
"""
import functools
import math

import numpy as np

# ---- the kernel constants the cases aim at, and where each lives ----
P1 = 10000000          # PROB_ONE (csrc/npr_internal.h): quanta per unit of probability
LWIN = 64              # npr_mea.hip k_mea_chain_lanes: read positions below ymax a lane's window holds
GROUP_LIMIT = 64       # npr_mea.hip k_mea_weigh WEIGH_HALO / prep_chunk: pairs on one reference position the device takes
WEIGH_CHUNK = 128      # npr_mea.hip k_mea_weigh: sorted positions per round (two per lane)
RING = 8192            # npr_finish.cpp upload_tables a.ring: read positions the LDS ring of k_mea_chain holds
PIECE_PAIRS = 128      # npr_finish.cpp plan_mea kPiecePairs = clamp(total / 81920, 128, 2048): 128 in any small batch
MAX_PIECES = 64        # npr_finish.cpp plan_mea kMaxPieces / npr_mea.hip MEA_MAX_PIECES
CUT_BLOCK = 64         # npr_mea.hip k_mea_cuts: a cut is looked for inside the 64-pair block at each planned boundary
LDS_SPAN = 16384       # npr_finish.cpp plan_mea lds_span: longer spans sort through global memory
RUN_BITS = 14          # npr_finish.cpp hand_over_words: runs below 1 << 14 cross as 16-bit words

OP_M, OP_I, OP_D = 0, 1, 2  # include/nprealign.h NPR_OP_*

# cases whose batch the device stage must hand to the host stage (they go in batches of their own: BATCH_TAG)
EXPECT_HOST = {"e_group65", "h_query_8192", "h_insert_8192"}
# cases the staging refuses (NPR_ERR_INVALID): gammas outside [0, 1] / [-1, 1] (include/nprealign.h npr_params)
EXPECT_REFUSED = {"g_wild_gammas"}
# a batch of its own for: the fall-back cases, and the run of 16384 (it makes its whole batch cross as whole words)
BATCH_TAG = {"e_group65": "host_a", "h_query_8192": "host_b", "h_insert_8192": "host_c", "f_del_16384": "wide"}
# the batches that are also run with mea_wide_ops
WIDE_OPS_CASES = {"f_del_16383", "f_del_16384"}


def quantum(p):
    return int(math.floor(float(np.float32(p)) * float(P1)))


def weigh(case):
    """-> (kept, dropped, floor_w): kept pairs (x, y, q, w) in (x, y) order -- their index is their id --, the dropped ones likewise."""
    _, lX, lY, xs, ys, ps, gg, mg = case
    q = [quantum(p) for p in ps]
    row, col = {}, {}
    for x, y, v in zip(xs, ys, q):
        row[int(x)] = row.get(int(x), 0) + v
        col[int(y)] = col.get(int(y), 0) + v
    floor_w = int(math.floor(mg * float(P1)))
    kept, dropped = [], []
    for x, y, v in sorted(zip((int(a) for a in xs), (int(b) for b in ys), q)):
        gap = max(P1 - row[x], 0) + max(P1 - col[y], 0)
        w = v - int(math.floor(gg * float(gap)))
        (kept if w > floor_w else dropped).append((x, y, v, w))
    return kept, dropped, floor_w


def replay(case):
    """The chain in the kernels' visit order: reference positions ascending, inside a position from the highest read position down;
    a prefix maximum over the read positions, (score, id) with ties to the larger id.  Per kept pair (by id):
      qdist  ymax - key of its query (key = y - 1), when 0 <= key <= ymax        idist  ymax - y of its insert, when y <= ymax
      jump   y - ymax of its insert, when y > ymax                               total, back, w
    and the best chain (ids), its cigar and score.  ymax: the largest read position inserted so far (k_mea_chain_lanes' ymax of an
    uncut read, k_mea_chain's ytop)."""
    _, lX, lY, _, _, _, _, _ = case
    kept, dropped, floor_w = weigh(case)
    order = sorted(range(len(kept)), key=lambda i: (kept[i][0], -kept[i][1]))
    arr = [(0, -1)] * lY
    top, ymax = (0, -1), -1
    qdist, idist, jump, total, back = {}, {}, {}, {}, {}
    for i in order:
        x, y, _, w = kept[i]
        key = y - 1
        if key < 0:
            best = (0, -1)
        elif key > ymax:
            best = top
        else:
            best, qdist[i] = arr[key], ymax - key
        total[i], back[i] = w + best[0], best[1]
        if total[i] < 0:
            continue  # a chain of negative weight beats nothing, the empty chain included
        v = (total[i], i)
        if y > ymax:
            for p in range(ymax + 1, y):
                arr[p] = top
            jump[i] = y - ymax
            top = max(top, v)
            arr[y], ymax = top, y
        else:
            idist[i] = ymax - y
            p = y
            while p <= ymax and arr[p] < v:
                arr[p] = v
                p += 1
            top = max(top, v)
    chain = []
    i = top[1]
    while i >= 0:
        chain.append(i)
        i = back[i]
    chain.reverse()
    ops = []

    def emit(op, n):
        if n <= 0:
            return
        if ops and ops[-1][0] == op:
            ops[-1] = (op, ops[-1][1] + n)
        else:
            ops.append((op, n))
    px, py, mass = -1, -1, 0
    for i in chain:
        x, y, q, _ = kept[i]
        emit(OP_D, x - px - 1), emit(OP_I, y - py - 1), emit(OP_M, 1)
        px, py, mass = x, y, mass + q
    emit(OP_D, lX - 1 - px), emit(OP_I, lY - 1 - py)
    score = float(mass) / (float(len(chain)) * float(P1)) if chain else 0.0
    return dict(kept=kept, dropped=dropped, floor_w=floor_w, order=order, qdist=qdist, idist=idist, jump=jump, total=total, back=back,
                chain=chain, ops=ops, score=score)


def legal_cuts(kept):
    """ids i after which a read's chain may be cut (k_mea_cuts' rule, stated on its own): every kept pair up to i lies strictly below
    every pair from i + 1 on, and x[i] != x[i + 1]."""
    m = len(kept)
    pre, suf = [0] * m, [0] * (m + 1)
    run = -1
    for i in range(m):
        run = max(run, kept[i][1])
        pre[i] = run
    suf[m] = 1 << 30
    for i in range(m - 1, -1, -1):
        suf[i] = min(suf[i + 1], kept[i][1])
    return [i for i in range(m - 1) if pre[i] < suf[i + 1] and kept[i][0] != kept[i + 1][0]], pre, suf


def plan_cuts(case):
    """-> (np, target blocks, pb): the pieces a SMALL batch cuts the read into.  np from the length of the whole list, a cut per planned
    boundary inside its 64-pair block of the kept pairs: the lowest legal one in the block's upper half, else the highest in its lower
    half, else none (the piece stays empty)."""
    kept = weigh(case)[0]
    n, m = len(case[3]), len(kept)
    np_ = min(MAX_PIECES, max(1, -(-n // PIECE_PAIRS)))
    nb = -(-m // CUT_BLOCK)
    if np_ <= 1 or nb < 2:
        return np_, [], [0] + [m] * np_
    legal = set(legal_cuts(kept)[0])
    targets = [j * nb // np_ for j in range(1, np_)]
    pb = [0] * (np_ + 1)
    pb[np_] = m
    for j, b in enumerate(targets, 1):
        lanes = [l for l in range(CUT_BLOCK) if b * CUT_BLOCK + l in legal]
        upper = [l for l in lanes if l >= 32]
        at = min(upper) if upper else (max(lanes) if lanes else -1)
        pb[j] = -1 if at < 0 else b * CUT_BLOCK + at + 1
    for k in range(1, np_):
        pb[k] = max(pb[k], pb[k - 1])
    return np_, targets, pb


def has_decisive_tie(rep):
    """some pair of the best chain had two candidates of the SAME total to follow, and took the one that sorts last"""
    kept, total = rep["kept"], rep["total"]
    for i in rep["chain"]:
        b = rep["back"][i]
        if b < 0:
            continue
        for j in range(len(kept)):
            if j != b and kept[j][0] < kept[i][0] and kept[j][1] < kept[i][1] and total[j] == total[b]:
                assert j < b, "the tie went to the pair that sorts first"
                return True
    return False


# ---------------------------------------------------------------------------------------------------------------------------
def _case(name, lX, lY, pairs, gg, mg):
    pairs = list(pairs)
    x = np.array([a for a, _, _ in pairs], dtype=np.int32)
    y = np.array([b for _, b, _ in pairs], dtype=np.int32)
    p = np.array([c for _, _, c in pairs], dtype=np.float32)
    return (name, int(lX), int(lY), x, y, p, float(gg), float(mg))


def _validate(case):
    name, lX, lY, x, y, p = case[:6]
    assert lX >= 1 and lY >= 1, name
    if len(x):
        assert x.min() >= 0 and x.max() < lX and y.min() >= 0 and y.max() < lY, name
    assert len(set(zip(x.tolist(), y.tolist()))) == len(x), "%s: a pair twice" % name
    if len(x):
        assert np.bincount(y).max() <= 64, "%s: more than 64 pairs on a read position" % name
        assert np.bincount(x).max() <= (65 if name == "e_group65" else 64), "%s: more than 64 pairs on a reference position" % name


def _on_chain(rep, x, y):
    return any(rep["kept"][i][0] == x and rep["kept"][i][1] == y for i in rep["chain"])


def _id_of(rep, x, y):
    return [i for i, k in enumerate(rep["kept"]) if k[0] == x and k[1] == y][0]


# ---- a. the window of the lane kernel ----
def _window_query(d):
    """a light diagonal up to ymax, then a heavy continuation whose first query has key = ymax - d: it must find the diagonal's chain
    up to that read position (62, 63: inside the lane's window; 64, 65: the read goes to the ring kernel)"""
    L = d + 4
    ymax = L - 1
    pairs = [(i, i, 0.01) for i in range(L)] + [(L + j, ymax - d + 1 + j, 0.9) for j in range(4)]
    c = _case("a_query_%d" % d, L + 6, L + 2, pairs, 0.0, 0.0)
    rep = replay(c)
    first = _id_of(rep, L, ymax - d + 1)
    assert len(pairs) <= PIECE_PAIRS and rep["qdist"][first] == d and max(rep["qdist"].values()) == d
    assert first in rep["chain"] and rep["back"][first] == _id_of(rep, ymax - d, ymax - d) and _on_chain(rep, 0, 0)
    return c


def _window_insert(d):
    """an insert at y = ymax - d that decides the chain.  A pair's query lies one position below its insert, so the only insert that can be
    d >= 64 below ymax without its own query having handed the read over first is one at read position 0 (key -1: no query).  The diagonal
    above it is heavy enough that the new chain beats only the entries up to read position 8: an insert that wraps around the window
    meets the entry of ymax first and stops."""
    pairs = [(i, i + 1, 0.1) for i in range(d)] + [(d, 0, 0.9)] + [(d + 1 + j, 3 + j, 0.9) for j in range(8)]
    c = _case("a_insert_%d" % d, d + 10, d + 2, pairs, 0.0, 0.0)
    rep = replay(c)
    ins = _id_of(rep, d, 0)
    assert len(pairs) <= PIECE_PAIRS and rep["idist"][ins] == d and ins not in rep["qdist"]
    assert max(rep["qdist"].values()) < LWIN, "no query hands the read over: the insert alone does"
    assert rep["chain"][0] == ins and len(rep["chain"]) == 9
    return c


def _window_jump(J, probe):
    """a forward jump of ymax by J, then a query `probe` positions below the new ymax: in the stretch the jump filled it must see the chain
    that was `top` before the jump"""
    y1 = 9 + J
    yq = y1 - probe + 1  # key = yq - 1 = y1 - probe
    pairs = [(i, i, 0.5) for i in range(10)] + [(10, y1, 0.3), (11, yq, 0.9)]
    if yq < y1:
        pairs.append((12, y1 + 1, 0.9))
    c = _case("a_jump_%d_probe_%d" % (J, probe), 14, y1 + 3, pairs, 0.0, 0.0)
    rep = replay(c)
    j, q = _id_of(rep, 10, y1), _id_of(rep, 11, yq)
    assert rep["jump"][j] == J and rep["qdist"][q] == probe and q in rep["chain"]
    if y1 - probe > 9:
        assert rep["back"][q] == _id_of(rep, 9, 9), "the filled stretch holds the diagonal's chain"
    return c


# ---- b. ties ----
def _ties_parallel(n):
    pairs = [(i, i, 0.5) for i in range(n)] + [(i, i + 1, 0.5) for i in range(n)]
    c = _case("b_parallel_diagonals_%d" % (2 * n), n + 1, n + 2, pairs, 0.0, 0.0)
    rep = replay(c)
    np_, _, pb = plan_cuts(c)
    # (no pair of one diagonal lies strictly below the next pair of the other: three planned boundaries inside, not one legal cut)
    assert np_ == 4 and pb == [0, 0, 0, 0, 2 * n] and has_decisive_tie(rep) and len(set(k[3] for k in rep["kept"])) == 1
    return c


def _ties_block(ny):
    """a full block of equal pairs (every row and column sums above one: no gap mass).  12 x 12: one heaviest chain, the ties are among the pairs
    beside it; 12 x 13: two chain ends of the same weight, and two candidates before every pair of the chain"""
    pairs = [(10 + i, 14 + j, 0.25) for i in range(12) for j in range(ny)]
    c = _case("b_block_12x%d" % ny, 40, 44, pairs, 0.5, 0.0)
    rep = replay(c)
    assert len(set(k[3] for k in rep["kept"])) == 1 and len(rep["chain"]) == 12 and has_decisive_tie(rep) == (ny != 12)
    return c


def _ties_lengths():
    """two alternatives of the same weight and different lengths (2 pairs of 0.5, 4 pairs of 0.25) between a common head and tail; once the
    long one sorts last, once the short one"""
    pairs = [(0, 0, 0.5), (1, 5, 0.5), (2, 6, 0.5), (3, 1, 0.25), (4, 2, 0.25), (5, 3, 0.25), (6, 4, 0.25), (7, 7, 0.5), (8, 8, 0.5)]
    o = 10
    pairs += [(o + 1, o + 1, 0.25), (o + 2, o + 2, 0.25), (o + 3, o + 3, 0.25), (o + 4, o + 4, 0.25), (o + 5, o - 1, 0.5), (o + 6, o, 0.5),
              (o + 7, o + 7, 0.5)]
    c = _case("b_equal_weight_lengths", 20, 20, pairs, 0.0, 0.0)
    rep = replay(c)
    assert has_decisive_tie(rep) and _on_chain(rep, 6, 4) and not _on_chain(rep, 2, 6)
    return c


# ---- c. zero and negative weights ----
def _zero(name, pairs, lX, lY):
    """gap_gamma 0.5: an isolated pair of p = 0.5 weighs exactly 0, and belongs to the chain (it beats the empty chain: it sorts later)"""
    c = _case(name, lX, lY, pairs, 0.5, -0.1)
    rep = replay(c)
    zero = [i for i, k in enumerate(rep["kept"]) if k[3] == 0]
    assert zero and all(i in rep["chain"] for i in zero) and len(rep["chain"]) == len(pairs)
    return c


def _negative_piece():
    """384 pairs on a diagonal, three pieces; the middle piece's pairs all weigh less than nothing (its pbest is -1)"""
    pairs = [(i, i, 0.1 if 150 <= i <= 300 else 0.9) for i in range(384)]
    c = _case("c_negative_piece", 384, 384, pairs, 0.5, -1.0)
    rep = replay(c)
    np_, _, pb = plan_cuts(c)
    assert np_ == 3 and pb[0] < pb[1] < pb[2] < pb[3]
    assert all(rep["kept"][i][3] < 0 for i in range(pb[1], pb[2]))
    assert any(rep["kept"][i][3] > 0 for i in range(pb[0], pb[1])) and any(rep["kept"][i][3] > 0 for i in range(pb[2], pb[3]))
    assert len(rep["kept"]) == 384
    return c


def _all_negative():
    pairs = [(i, i + 2, 0.1) for i in range(40)]
    c = _case("c_all_negative", 45, 50, pairs, 0.5, -1.0)
    rep = replay(c)
    assert len(rep["kept"]) == 40 and all(k[3] < 0 for k in rep["kept"]) and rep["ops"] == [(OP_D, 45), (OP_I, 50)] and rep["score"] == 0.0
    return c


def _floor_weight():
    """match_gamma 0.25: a pair of weight exactly floor_w is dropped, one of floor_w + 1 kept; either would join the chain"""
    p1 = np.float32(0.25)
    while quantum(p1) < 2500001:
        p1 = np.nextafter(p1, np.float32(1.0))
    assert quantum(p1) == 2500001
    pairs = [(0, 0, 0.9), (2, 1, 0.25), (5, 4, float(p1)), (7, 7, 0.9)]
    c = _case("c_floor_weight", 9, 9, pairs, 0.0, 0.25)
    rep = replay(c)
    assert [k[:2] for k in rep["dropped"]] == [(2, 1)] and rep["dropped"][0][3] == rep["floor_w"]
    assert rep["kept"][_id_of(rep, 5, 4)][3] == rep["floor_w"] + 1 and _on_chain(rep, 5, 4) and len(rep["chain"]) == 3
    return c


# ---- d. cuts ----
def _staircase(name, n, rng, strands=()):
    """a diagonal of n pairs with weights from a small set; strands = (first id, length): stretches replaced by anti-diagonals (no two
    of their pairs chain, no cut inside them)"""
    ys = list(range(n))
    for s, k in strands:
        ys[s:s + k] = ys[s:s + k][::-1]
    vals = (0.2, 0.4, 0.6, 0.8)
    pairs = [(i, ys[i], vals[int(rng.integers(4))]) for i in range(n)]
    return _case(name, n + 1, n + 3, pairs, 0.0, 0.0)


def _cut_pieces(name, n, want_np, rng):
    c = _staircase(name, n, rng, strands=[(s, 7) for s in range(30, n - 10, 97)])
    np_, _, pb = plan_cuts(c)
    assert np_ == want_np and len(set(pb)) == np_ + 1, "every planned boundary finds a cut"
    return c


def _cut_many(rng):
    """more than 64 planned pieces: two pairs per reference position, more than 8192 pairs on one read"""
    n = 4200
    vals = (0.2, 0.4, 0.6, 0.8)
    pairs = []
    for i in range(n):
        pairs.append((i, i, vals[int(rng.integers(4))]))
        if i % 50 != 49:
            pairs.append((i, i + 1, vals[int(rng.integers(4))]))
    c = _case("d_more_than_64_pieces", n + 1, n + 2, pairs, 0.0, 0.0)
    np_, _, pb = plan_cuts(c)
    assert len(pairs) > MAX_PIECES * PIECE_PAIRS and np_ == MAX_PIECES and len(set(pb)) > 32
    return c


def _cut_strands(rng):
    """anti-diagonal strands that span several planned blocks: planned boundaries without a cut, empty pieces, pb[k] = pb[k - 1]"""
    c = _staircase("d_strands_empty_pieces", 640, rng, strands=[(100, 301), (500, 100)])
    np_, targets, pb = plan_cuts(c)
    empty = [k for k in range(1, np_ + 1) if pb[k] == pb[k - 1]]
    assert np_ == 5 and len(empty) >= 2 and len(set(pb)) >= 3
    return c


def _cut_equal_x():
    """two pairs per reference position, shifted so that a position's two pairs lie on both sides of every block edge"""
    pairs = [(0, 0, 0.5)]
    for i in range(1, 160):
        pairs += [(i, 2 * i, 0.3), (i, 2 * i + 1, 0.6 if i % 3 else 0.3)]
    c = _case("d_equal_x_across_block_edge", 161, 322, pairs, 0.0, 0.0)
    rep = replay(c)
    np_, targets, pb = plan_cuts(c)
    k = rep["kept"]
    assert np_ == 3 and all(k[b * 64 + 63][0] == k[b * 64 + 64][0] for b in targets) and len(set(pb)) == 4
    return c


def _cut_single(lane):
    """256 pairs, two pieces, the planned boundary in block 2 (ids 128 .. 191): two anti-diagonal strands meet after lane `lane` of it, the only
    legal cut of the block"""
    n, cut = 256, 128 + lane
    ys = list(range(n))
    a0, b1 = 110, 215  # strand A: ids a0 .. cut, strand B: ids cut + 1 .. b1
    ys[a0:cut + 1] = ys[a0:cut + 1][::-1]
    ys[cut + 1:b1 + 1] = ys[cut + 1:b1 + 1][::-1]
    pairs = [(i, ys[i], 0.3 + 0.1 * ((i * 7) % 5)) for i in range(n)]
    c = _case("d_only_cut_at_lane_%d" % lane, n + 1, n + 1, pairs, 0.0, 0.0)
    np_, targets, pb = plan_cuts(c)
    legal = legal_cuts(weigh(c)[0])[0]
    assert np_ == 2 and targets == [2] and [i - 128 for i in legal if 128 <= i < 192] == [lane] and pb == [0, cut + 1, n]
    return c


def _cut_equal_y():
    """a run of 51 pairs on ONE read position across the planned block (ids 140 .. 190 of block 128 .. 191): between two of them the prefix
    maximum EQUALS the suffix minimum, which is no cut -- they never chain.  The legal cuts of the block lie at its lanes 0 .. 11 and 62, 63."""
    n = 256
    pairs = []
    for i in range(n):
        if i < 140:
            pairs.append((i, i, 0.3))
        elif i < 191:
            pairs.append((i, 140, 0.5 + 0.01 * (i % 7)))
        else:
            pairs.append((i, i - 50, 0.3))
    c = _case("d_equal_y_is_no_cut", n + 1, n, pairs, 0.0, 0.0)
    rep = replay(c)
    np_, targets, pb = plan_cuts(c)
    legal, pre, suf = legal_cuts(rep["kept"])
    assert np_ == 2 and targets == [2] and all(pre[i] == suf[i + 1] for i in range(140, 190)) and pb == [0, 191, n]
    assert [i - 128 for i in legal if 128 <= i < 192] == list(range(12)) + [62, 63]
    assert sum(1 for i in rep["chain"] if rep["kept"][i][1] == 140) == 1
    return c


# ---- e. groups ----
def _group(x, y0, k, rng, vals=(0.004, 0.008, 0.012)):
    return [(x, y0 + j, vals[int(rng.integers(len(vals)))]) for j in range(k)]


def _group_sizes(rng):
    """reference positions with 64 (the very first group of the list), 1, 2, 63 and 64 (the very last) pairs"""
    pairs = _group(0, 0, 64, rng) + [(1, 70, 0.5)] + _group(2, 60, 2, rng) + _group(3, 40, 63, rng) + [(4, 110, 0.5)] + _group(5, 100, 64, rng)
    c = _case("e_group_sizes", 6, 170, pairs, 0.0, 0.0)
    rep = replay(c)
    sizes = np.bincount(c[3]).tolist()
    assert sizes == [64, 1, 2, 63, 1, 64] and len(rep["kept"]) == len(pairs) and len(rep["chain"]) >= 4
    return c


def _group_65(rng):
    pairs = [(0, 0, 0.5)] + _group(1, 1, 65, rng) + [(2, 80, 0.5)]
    c = _case("e_group65", 4, 90, pairs, 0.0, 0.0)
    assert np.bincount(c[3]).max() == GROUP_LIMIT + 1
    return c


def _group_straddle(rng):
    """groups that lie across position 64 and position 128 of the sorted list (the wavefront's halves of a k_mea_weigh round, and its rounds)"""
    pairs, x, y = [], 0, 0
    while len(pairs) < 60:
        pairs.append((x, y, 0.5))
        x, y = x + 1, y + 1
    pairs += _group(x, y, 10, rng, (0.2, 0.4))  # positions 60 .. 69
    x, y = x + 1, y + 10
    while len(pairs) < 124:
        pairs.append((x, y, 0.5))
        x, y = x + 1, y + 1
    pairs += _group(x, y, 10, rng, (0.2, 0.4))  # positions 124 .. 133
    x, y = x + 1, y + 10
    for _ in range(20):
        pairs.append((x, y, 0.5))
        x, y = x + 1, y + 1
    c = _case("e_groups_across_64_and_128", x + 1, y + 1, pairs, 0.5, 0.0)
    xs = sorted(c[3].tolist())
    assert xs[63] == xs[64] and xs[127] == xs[128] and xs[59] != xs[60] and xs[123] != xs[124]
    return c


def _group_lonely():
    """a kept pair whose group-mates are all dropped (p = 0: quantum 0, not above match_gamma 0)"""
    pairs = [(0, 0, 0.5), (3, 2, 0.0), (3, 3, 0.0), (3, 4, 0.7), (3, 5, 0.0), (3, 6, 0.0), (5, 7, 0.5)]
    c = _case("e_lonely_kept_pair", 7, 9, pairs, 0.0, 0.0)
    rep = replay(c)
    assert [k[:2] for k in rep["dropped"]] == [(3, 2), (3, 3), (3, 5), (3, 6)] and _on_chain(rep, 3, 4) and len(rep["chain"]) == 3
    return c


# ---- f. trace and packing ----
def _trace_cases():
    out = [_case("f_empty", 5, 7, [], 0.0, 0.0), _case("f_single", 6, 5, [(2, 3, 0.7)], 0.0, 0.0),
           _case("f_corner_pairs", 9, 12, [(0, 0, 0.7), (4, 5, 0.6), (8, 11, 0.7)], 0.0, 0.0),
           _case("f_leading_insert_only", 6, 9, [(0, 5, 0.7), (1, 6, 0.7)], 0.0, 0.0),
           _case("f_leading_delete_only", 9, 6, [(5, 0, 0.7), (6, 1, 0.7)], 0.0, 0.0),
           _case("f_diagonal_250", 250, 250, [(i, i, 0.9) for i in range(250)], 0.0, 0.0)]
    assert replay(out[0])["ops"] == [(OP_D, 5), (OP_I, 7)] and replay(out[1])["ops"] == [(OP_D, 2), (OP_I, 3), (OP_M, 1), (OP_D, 3), (OP_I, 1)]
    rep = replay(out[2])
    assert rep["ops"][0] == (OP_M, 1) and rep["ops"][-1] == (OP_M, 1)
    assert replay(out[3])["ops"] == [(OP_I, 5), (OP_M, 2), (OP_D, 4), (OP_I, 2)] and replay(out[4])["ops"] == [(OP_D, 5), (OP_M, 2), (OP_D, 2), (OP_I, 4)]
    assert replay(out[5])["ops"] == [(OP_M, 250)]
    # consecutive pairs of the chain more than 64 list entries apart: 67 light pairs on read positions 0 and 1 between them (none chains after (60, 1))
    pairs = [(0, 0, 0.9)] + [(i, 0, 0.01) for i in range(1, 60)] + [(60, 1, 0.9)] + [(i, 1, 0.01) for i in range(61, 124)]
    pairs += [(i, 0, 0.01) for i in range(124, 128)] + [(128, 2, 0.9)]
    far = _case("f_chain_pairs_far_apart", 130, 4, pairs, 0.0, 0.0)
    rep = replay(far)
    assert [rep["kept"][i][:2] for i in rep["chain"]] == [(0, 0), (60, 1), (128, 2)] and rep["chain"][2] - rep["chain"][1] > 64
    out.append(far)
    for run in ((1 << RUN_BITS) - 1, 1 << RUN_BITS):
        c = _case("f_del_%d" % run, run + 4, 4, [(0, 0, 0.9), (1, 1, 0.9), (run + 2, 2, 0.9), (run + 3, 3, 0.9)], 0.0, 0.0)
        assert replay(c)["ops"] == [(OP_M, 2), (OP_D, run), (OP_M, 2)] and c[1] + 1 > LDS_SPAN
        out.append(c)
    return out


# ---- g. values ----
def _sparse(name, rng, lX, lY, gg, mg, vals, per_pos=6):
    col = np.zeros(lY, dtype=np.int64)
    pairs = []
    for x in range(lX):
        k = min(int(rng.integers(0, per_pos + 1)), lY)
        for y in rng.choice(lY, size=k, replace=False).tolist():
            if col[y] < 64:
                col[y] += 1
                pairs.append((x, int(y), float(vals[int(rng.integers(len(vals)))])))
    return _case(name, lX, lY, pairs, gg, mg)


def _value_cases(rng):
    above = float(np.float32(1.0 + 2.0 ** -20))
    assert above > 1.0 and quantum(above) == 10000009
    out = [_case("g_p_one", 30, 30, [(i, i, 1.0) for i in range(30)] + [(i, i + 1, 0.01) for i in range(29)], 0.5, 0.0),
           _case("g_p_above_one", 30, 31, [(i, i, above) for i in range(30)] + [(i, i + 1, 0.5) for i in range(30)], 0.5, 0.0)]
    tiny = [(0, 0, 0.9), (1, 1, 0.0), (2, 2, 1e-8), (3, 3, 0.9), (4, 2, 0.0), (5, 5, 1e-8)]
    out += [_case("g_quantum_zero_dropped", 7, 7, tiny, 0.5, 0.0), _case("g_quantum_zero_kept", 7, 7, tiny, 0.0, -0.1)]
    assert quantum(1e-8) == 0 and len(replay(out[2])["kept"]) == 2 and len(replay(out[3])["chain"]) == 5
    vals = (0.02, 0.1, 0.25, 0.5, 0.75, 0.9)
    out += [_sparse("g_gap_gamma_0", rng, 120, 100, 0.0, 0.0, vals, 3), _sparse("g_gap_gamma_1", rng, 120, 100, 1.0, 0.0, vals, 3),
            _sparse("g_gap_gamma_1_negative_floor", rng, 90, 110, 1.0, -1.0, vals, 3)]
    # gammas that are no weights between 0 and 1: 250 * 2e7 does not fit the 32 bits the device keeps a weight in.  The host stage and the oracle
    # take them (64-bit weights); staging a batch with them is refused (include/nprealign.h npr_params)
    out.append(_sparse("g_wild_gammas", rng, 60, 60, 250.0, -300.0, vals, 3))
    rep = replay(out[-1])
    assert min(k[3] for k in rep["kept"]) < -(1 << 31)
    return out


# ---- h. the reach of the ring kernel ----
def _ring_query(d):
    """a query d read positions below ytop: 8191 is the ring's last entry, 8192 is out of reach (NPR_ERR_CAPACITY: the batch goes to the host
    stage)"""
    ytop = 8300
    K = ytop - d
    pairs = [(0, K, 0.01), (1, ytop, 0.1), (2, K + 1, 0.9), (3, K + 2, 0.9), (4, K + 3, 0.9)]
    c = _case("h_query_%d" % d, 6, ytop + 5, pairs, 0.0, 0.0)
    rep = replay(c)
    q = _id_of(rep, 2, K + 1)
    assert rep["qdist"][q] == d and rep["back"][q] == _id_of(rep, 0, K) and len(rep["chain"]) == 4
    return c


def _ring_insert(d):
    """an insert d read positions below ytop, at read position 0 (see a_insert): the chain starts with it"""
    pairs = [(0, d, 0.1), (1, 0, 0.9), (2, 1, 0.9), (3, 2, 0.9)]
    c = _case("h_insert_%d" % d, 5, d + 3, pairs, 0.0, 0.0)
    rep = replay(c)
    ins = _id_of(rep, 1, 0)
    assert rep["idist"][ins] == d and rep["chain"][0] == ins and len(rep["chain"]) == 3
    return c


# ---- i. fuzz ----
FUZZ_VALUES = (0.0, 0.05, 0.125, 0.25, 0.5, 0.5000001, 0.75, 1.0)
FUZZ_GAMMAS = tuple((g, m) for g in (0.0, 0.5, 0.9) for m in (-0.1, 0.0, 0.3))


def _fuzz(rng, count=297):
    out = []
    for k in range(count):
        gg, mg = FUZZ_GAMMAS[k % len(FUZZ_GAMMAS)]
        lX, lY = int(rng.integers(1, 301)), int(rng.integers(1, 301))
        out.append(_sparse("i_fuzz_%03d" % k, rng, lX, lY, gg, mg, FUZZ_VALUES, int(rng.integers(0, 7))))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every case, validated, each with the property it is named for asserted (a tuple: shared between the tests, not to be changed)"""
    rng = np.random.default_rng(20260)
    out = []
    out += [_window_query(d) for d in (62, 63, 64, 65)]
    out += [_window_insert(d) for d in (62, 63, 64, 65)]
    out += [_window_jump(J, 1) for J in (1, 63, 64, 65, 500)] + [_window_jump(J, 63) for J in (63, 64, 65, 500)]
    out += [_ties_parallel(200), _ties_block(12), _ties_block(13), _ties_lengths()]
    out += [_zero("c_zero_alone", [(3, 4, 0.5)], 8, 9), _zero("c_zero_first", [(1, 1, 0.5), (3, 3, 0.9), (4, 4, 0.9)], 6, 6),
            _zero("c_zero_last", [(1, 1, 0.9), (2, 2, 0.9), (4, 4, 0.5)], 6, 6), _zero("c_zero_between", [(1, 1, 0.9), (3, 3, 0.5), (5, 5, 0.9)], 7, 7)]
    out += [_negative_piece(), _all_negative(), _floor_weight()]
    out += [_cut_pieces("d_3_pieces", 380, 3, rng), _cut_pieces("d_9_pieces", 1100, 9, rng), _cut_many(rng), _cut_strands(rng), _cut_equal_x()]
    out += [_cut_single(lane) for lane in (0, 31, 32, 63)] + [_cut_equal_y()]
    out += [_group_sizes(rng), _group_65(rng), _group_straddle(rng), _group_lonely()]
    out += _trace_cases()
    out += _value_cases(rng)
    out += [_ring_query(RING - 1), _ring_query(RING), _ring_insert(RING - 1), _ring_insert(RING)]
    out += _fuzz(rng)
    for c in out:
        _validate(c)
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    assert EXPECT_HOST <= set(names) and EXPECT_REFUSED <= set(names) and set(BATCH_TAG) <= set(names) and WIDE_OPS_CASES <= set(names)
    return tuple(out)

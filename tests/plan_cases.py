"""Constructed guides for the device planner (nanopore_amd/csrc/npr_plan.hip): reads whose lengths and guides sit on the planner's own
constants -- the band kernel's tiles of 1024 anti-diagonals and its 1025 staged plan points, the schedule's chunks of 256, the stripe
table's trips of 64 stripes.  No GPU here: the
cases are built with the host planner (realign.plan / frame_schedule / stripes, the npr_plan_* functions of include/nprealign.h);
tests/test_plan_cases_host.py proves that each case has the property it is named for, tests/test_gpu_plan_edges.py stages them.

A case is (name, params kwargs, ref, read, guide ops).  The reference is random ACGT from a fixed seed and the read its copy along the guide: only the lengths
and the guide matter to the planner.  Anti-diagonal d of a read is x + y; D = lX + lY is its last one."""
import functools

import numpy as np

from nanopore_amd import _lib

OP_M, OP_I, OP_D = _lib.OP_M, _lib.OP_I, _lib.OP_D

BAND_TILE = 1024    # npr_plan.hip BAND_TILE: anti-diagonals per tile of k_plan_bands
BAND_STAGE = 1025   # ... and the plan points of a tile it stages in LDS (BAND_STAGE + 1)
SCHED_CHUNK = 256   # npr_plan.hip SCHED_CHUNK: anti-diagonals per chunk of the frame schedule
STRIPE_TRIP = 64    # k_plan_stripes: stripes per trip of its wavefront
STRIPE_COLS = 128   # columns of a stripe (64 lanes, two slots per lane: the stripe class has R = 2)

# The frame classes a one-wavefront task may take under the default context options, smallest first, as (R, NW), and the widest band row
# each admits (npr_sched.h stair_max_width).  The staging's candidate rule (npr_stage.cpp frame_candidates) also asks stair_fits(rows, slots):
# rows * slots < 2^29 - 512.  Every case here has fewer than 2^16 rows and at most 256 slots, 2^24 in all, so that clause never decides and
# the rule is "every class whose width limit admits the widest row" -- which is what candidates() below and the host call agree on.
FRAME_CLASSES = ((1, 1), (2, 1), (4, 1))
FRAME_MAX_WIDTH = {(1, 1): 63, (2, 1): 126, (4, 1): 255}


def spans(ops):
    return sum(n for o, n in ops if o != OP_I), sum(n for o, n in ops if o != OP_D)


def merged(ops):
    """neighbouring runs of one kind joined, runs without a base dropped"""
    out = []
    for o, n in ops:
        if n <= 0:
            continue
        if out and out[-1][0] == o:
            out[-1] = (o, out[-1][1] + n)
        else:
            out.append((o, n))
    return out


def _case(name, kw, ops, rng):
    lX, lY = spans(ops)
    ref = bytes(b"ACGT"[v] for v in rng.integers(0, 4, lX))
    read, x = [], 0   # the read follows the guide: reference bases under M, random ones under I (the runs of test_gpu_plan_edges have an alignment to find)
    for o, n in ops:
        read.append(ref[x:x + n] if o == OP_M else bytes(b"ACGT"[v] for v in rng.integers(0, 4, n)) if o == OP_I else b"")
        x += n if o != OP_I else 0
    read = b"".join(read)
    assert len(read) == lY
    return (name, dict(kw), ref, read, [(int(o), int(n)) for o, n in ops])


def params_of(case):
    from nanopore_amd import realign as R
    return R.make_params(**case[1])


def host_plan(case):
    """the host planner's segments of the case (realign.plan: dicts with D, lo, n, ...)"""
    from nanopore_amd import realign as R
    return R.plan(params_of(case), len(case[2]), len(case[3]), case[4])


def host_schedule(case, shape, segment=0):
    """the host's frame schedule of one segment for the frame (R, NW), or None when that frame cannot follow the band"""
    from nanopore_amd import realign as R
    r, nw = shape
    return R.frame_schedule(params_of(case), len(case[2]), len(case[3]), case[4], 64 * r * nw, r, segment=segment)


def candidates(seg):
    """the frame classes whose width limit admits the segment's widest row (see FRAME_CLASSES)"""
    w = int(seg["n"].max())
    return [s for s in FRAME_CLASSES if w <= FRAME_MAX_WIDTH[s]]


def host_shape(case, segment=0):
    """(candidates, the smallest candidate the host can follow the band with or None)"""
    cand = candidates(host_plan(case)[segment])
    for s in cand:
        if host_schedule(case, s, segment) is not None:
            return cand, s
    return cand, None


def rough(seg):
    """does an edge of the band move by something other than one cell between neighbouring anti-diagonals (k_plan_bands' flag)?"""
    lo = seg["lo"].astype(np.int64)
    hi = lo + 2 * (seg["n"].astype(np.int64) - 1)
    return bool((np.abs(np.diff(lo)) != 1).any() or (np.abs(np.diff(hi)) != 1).any())


def fixed_points_d0(ops):
    """Anti-diagonal of every plan point of a fixed-width band: one piece per guide operation (npr_band.h, NPR_BAND_FIXED; npr_host.cpp
    points_fixed_width), the point after an operation at the lattice point the guide has reached.  m operations -> m + 1 points."""
    d = [0]
    for o, n in ops:
        d.append(d[-1] + (2 * n if o == OP_M else n))
    return np.asarray(d, dtype=np.int64)


def points_per_tile(ops):
    """plan points whose anti-diagonal falls into each tile of BAND_TILE anti-diagonals"""
    return np.bincount(fixed_points_d0(ops) // BAND_TILE)


# ---- A: lengths on the seams -------------------------------------------------------------------------------------------------------------------

A_LENGTHS = (0, 1, 2, 3, 254, 255, 256, 257, 258, 511, 512, 513, 1022, 1023, 1024, 1025, 1026, 2047, 2048, 2049)
# a fixed-width band has one segment whatever split_threshold says (points_fixed_width); 40 wide: the smallest frame class
A_PARAMS = dict(band_mode=_lib.BAND_FIXED, fixed_width=40, split_threshold=0)


def _guide_with_run_at(D, start, run, op):
    """a guide of D anti-diagonals with an indel run of `run` bases that begins at anti-diagonal `start`; M elsewhere, with a one-base
    indel in front / at the end where a parity needs one"""
    ops = []
    head = start
    if head & 1:
        ops.append((OP_I, 1))
        head -= 1
    ops.append((OP_M, head // 2))
    ops.append((op, run))
    tail = D - start - run
    assert tail >= 0
    ops.append((OP_M, tail // 2))
    if tail & 1:
        ops.append((OP_D, 1))
    return [(o, n) for o, n in ops if n > 0]


def family_a():
    rng = np.random.default_rng(1001)
    out = []
    for D in A_LENGTHS:
        ops = [(OP_M, D // 2)] if D % 2 == 0 else merged([(OP_M, D // 4), (OP_I, 1), (OP_M, D // 2 - D // 4)])
        out.append(_case("a_flat_D%d" % D, A_PARAMS, merged(ops), rng))
    q = 0
    for D in A_LENGTHS:
        edges = sorted({e for e in (SCHED_CHUNK * (D // SCHED_CHUNK), SCHED_CHUNK * max(1, D // SCHED_CHUNK - 1), BAND_TILE) if SCHED_CHUNK <= e})
        for e in edges:
            for off in (-2, -1, 0, 1):
                start = e + off
                run = min(1 + q % 3, D - start)
                if run < 1:
                    continue
                op = (OP_I, OP_D)[q % 2]
                q += 1
                out.append(_case("a_run_D%d_at%d%+d_%s%d" % (D, e, off, "MID"[op], run), A_PARAMS, _guide_with_run_at(D, start, run, op), rng))
    return out


# ---- B: rebase at a chunk head -------------------------------------------------------------------------------------------------------------------

# fixed_width / 2 cells either side of the guide path: 61, 126 and 251 cells per row, two to four fewer than the class's frame has slots, so
# that every base of an indel run moves the frame (a rebase towards lower x - y precedes the even anti-diagonals of an I run, one towards
# higher x - y the odd ones of a D run: npr_sched.h)
B_WIDTHS = {(1, 1): 120, (2, 1): 250, (4, 1): 500}


def family_b():
    rng = np.random.default_rng(1002)
    out = []
    for shape, width in B_WIDTHS.items():
        kw = dict(band_mode=_lib.BAND_FIXED, fixed_width=width, split_threshold=0)
        for k, op in ((1, OP_I), (2, OP_D), (3, OP_I), (3, OP_D)):
            # a run of 16 bases from anti-diagonal 256 k - 6 on: it covers the chunk's first two rows
            head = SCHED_CHUNK * k - 6
            ops = [(OP_M, head // 2), (op, 16), (OP_M, 150), ((OP_D, OP_I)[op == OP_I], 16), (OP_M, 40)]
            out.append(_case("b_R%d_chunk%d_%s" % (shape[0], k, "MID"[op]), kw, ops, rng))
    return out


def chunk_head_rebases(case, shape):
    """[(d, rebase)] of the host schedule's non-zero rebases in the first two rows of a chunk after the first"""
    sch = host_schedule(case, shape)
    if sch is None:
        return []
    reb = sch["rebase"]
    return [(d, int(reb[d])) for k in range(1, len(reb) // SCHED_CHUNK + 1) for d in (SCHED_CHUNK * k, SCHED_CHUNK * k + 1) if d < len(reb) and reb[d] != 0]


# ---- C: many pieces per tile ---------------------------------------------------------------------------------------------------------------------

C_PARAMS = dict(band_mode=_lib.BAND_FIXED, fixed_width=40, split_threshold=0)


def family_c():
    rng = np.random.default_rng(1003)
    out = []
    out.append(_case("c_1I1D", C_PARAMS, [(OP_I, 1), (OP_D, 1)] * 1150, rng))                           # 2300 anti-diagonals, a piece each
    out.append(_case("c_M500_1I1D", C_PARAMS, [(OP_M, 250)] + [(OP_I, 1), (OP_D, 1)] * 1150, rng))      # the dense part starts mid-tile
    out.append(_case("c_1M1I1M1D", C_PARAMS, [(OP_M, 1), (OP_I, 1), (OP_M, 1), (OP_D, 1)] * 400, rng))  # 2400 anti-diagonals
    # Operations without a base (npr_batch_create takes them: only a negative length is refused): pieces that own no anti-diagonal, the
    # ones k_plan_bands' search past its staged points exists for.  Runs of them at the read's head, mid-tile, across a tile seam's
    # anti-diagonal (1024 = M 512) and at the read's end; 1500 in a row put more than 1025 points on one anti-diagonal.
    zeros = lambda n: [((OP_I, OP_D)[i % 2], 0) for i in range(n)]
    ops = zeros(1500) + [(OP_M, 150)] + zeros(1100) + [(OP_I, 1), (OP_D, 1)] * 200 + [(OP_M, 162)] + zeros(1300) + [(OP_M, 300)] + zeros(40) + \
        [(OP_I, 3)] + zeros(1030) + [(OP_M, 200), (OP_D, 2)] + zeros(1200)
    out.append(_case("c_zero_runs", C_PARAMS, ops, rng))
    out.append(_case("c_zero_only_tail", C_PARAMS, [(OP_M, 600)] + zeros(2100), rng))
    return out


# ---- D: class fall-through, and rough bands: the search, and why it comes back empty -------------------------------------------------------------
#
# A segment leaves the smallest frame class that admits its width only if the frame cannot follow the band, and k_plan_stripes takes its
# general walk only if k_plan_bands flags the band as rough (an edge that moves by something other than one cell between neighbouring rows).
# Neither can be made from a guide that npr_batch_create accepts:
#   * Every term of band_row_of_piece (npr_band.h) -- the guide path +- fixed_width / 2; 2 ax - d, d - 2 by, 2 bx - d, d - 2 ay of a rectangle;
#     the diagonal run's c -+ odd; the lattice's -d, d - 2 lY, d, 2 lX - d -- moves by exactly one per anti-diagonal, consecutive pieces meet
#     in a lattice point, and a max / min of such terms rounded to the row's parity moves by exactly one as well.  So no band is rough.
#   * A class admits rows of at most slots - 1 cells (stair_max_width; slots - 2 for the two-slot class), so a band that fits keeps one slot
#     of slack, and stair_step (npr_sched.h) looks one row ahead: a frame that may move by one slot before every second row follows any
#     band whose edges move by one cell per row.  So the first candidate never fails, and k_sched_finish's `left` mask, the second round over
#     the same chunks and a second increment of active[] are reached by no batch.
# search_family() is the family the search ran over, widened twice: alternating I and D runs of 20 .. 80 and of 20 .. 200 bases between M runs
# of 1 .. 40, no trimming and trimmed anchors (5, 14), anchored bands with the diagonal expansion that puts the widest row exactly on a class's
# limit, fixed bands of the widths that do the same, one segment and split reads.  tests/test_plan_cases_host.py asserts over all of it that
# no band is rough and that the first candidate class follows every segment: if the planner ever changes so that one of the two can
# happen, that test fails, and the cases it names belong into families D and E here and into the class test of test_gpu_plan_edges.py.
SEARCH_SEEDS = 2000


def _search_guide(rng, longest):
    ops = [(OP_M, int(rng.integers(1, 41)))]
    for i in range(int(rng.integers(4, 17))):
        ops.append(((OP_I, OP_D)[(i + int(rng.integers(0, 2)) * (i % 3 == 0)) % 2], int(rng.integers(20, longest + 1))))
        ops.append((OP_M, int(rng.integers(1, 41))))
    return merged(ops)


def search_family():
    """yields (case, class whose width limit the parameters were fitted to)"""
    fixed_at_limit = {(1, 1): 124, (2, 1): 250, (4, 1): 508}   # fixed_width / 2 cells either side: rows of 63, 126 and 255 cells
    for seed in range(SEARCH_SEEDS):
        rng = np.random.default_rng(7000 + seed)
        ops = _search_guide(rng, (80, 200)[seed % 2])
        shape = FRAME_CLASSES[seed % 3]
        limit = FRAME_MAX_WIDTH[shape]
        if seed % 4 == 3:
            yield _case("s_fixed_seed%d" % seed, dict(band_mode=_lib.BAND_FIXED, fixed_width=fixed_at_limit[shape], split_threshold=0), ops, rng), shape
            continue
        kw = dict(band_mode=_lib.BAND_ANCHOR, constraint_trim=(0, 5, 14)[seed // 4 % 3], split_threshold=(100000, 100000, 40)[seed // 12 % 3])
        probe = lambda e: max(int(g["n"].max()) for g in host_plan(_case("p", dict(kw, diagonal_expansion=e), ops, np.random.default_rng(0))))
        e = limit - probe(0)
        for _ in range(8):   # (the widest row grows by one cell per unit of expansion until the lattice clips it)
            if e < 0 or probe(e) <= limit:
                break
            e -= 1
        if e >= 0 and probe(e) <= limit:
            yield _case("s_anchor_seed%d" % seed, dict(kw, diagonal_expansion=e), ops, rng), shape


# ---- E: stripes ----------------------------------------------------------------------------------------------------------------------------------

E_LENGTHS = (127, 128, 129, 8063, 8064, 8191, 8192, 8193, 16383, 16384)
E_STRIPES = {127: 1, 128: 2, 129: 2, 8063: 63, 8064: 64, 8191: 64, 8192: 65, 8193: 65, 16383: 128, 16384: 129}
# 301 cells per row: wider than the widest one-wavefront frame (255), so the task takes the stripe kernel
E_PARAMS = dict(band_mode=_lib.BAND_FIXED, fixed_width=600, split_threshold=0)
# References of fewer than 255 bases have no row that wide (a row has at most min(lX, lY) + 1 cells) and the four-slot frame would take them
# in a realign batch.  A batch staged for the E-step keeps the four-slot frame class out (npr_stage.cpp frame_candidates: its stripe tasks'
# kernel is the faster one there), so there a row of more than 126 cells goes to the stripes: these cases are staged in that mode.
E_PARAMS_SHORT = dict(band_mode=_lib.BAND_FIXED, fixed_width=600, split_threshold=0, mode=_lib.MODE_EXPECTATIONS)


def _noisy_guide(rng, lX, indel=0.05, max_indel=6, block=(20, 200)):
    """M blocks with indel runs between, lX reference bases in all"""
    ops, x = [], 0
    while x < lX:
        m = min(int(rng.integers(block[0], block[1])), lX - x)
        ops.append((OP_M, m))
        x += m
        if x < lX and rng.random() < 0.9:
            k = int(rng.integers(1, max_indel + 1))
            if rng.random() < 0.5:
                k = min(k, lX - x)
                ops.append((OP_D, k))
                x += k
            else:
                ops.append((OP_I, k))
    return merged(ops)


@functools.lru_cache(maxsize=None)
def family_e():
    rng = np.random.default_rng(1005)
    out = []
    for lX in E_LENGTHS:
        out.append(_case("e_lX%d" % lX, E_PARAMS_SHORT if lX < 255 else E_PARAMS, _noisy_guide(rng, lX), rng))
    # (Rough bands, for k_plan_stripes' general walk: see the note above search_family -- no guide makes one.)
    # A row without a cell (n < 1, k_plan_bands' `bad`) cannot be made from a guide npr_batch_create accepts: a fixed-width band is at least
    # two cells either side of a lattice path that it contains, and an anchored band contains the corner-to-corner path of every one of its
    # rectangles, so every row of either holds a lattice point of the read.  The host test asserts that no case has such a row.
    return tuple(out)


# ---- F: multi-segment reads ----------------------------------------------------------------------------------------------------------------------

def family_f():
    out = []
    for i, (lX, split) in enumerate(((3000, 5), (4500, 40), (6000, 5), (5200, 40))):
        rng = np.random.default_rng(1006 + i)
        kw = dict(band_mode=_lib.BAND_ANCHOR, diagonal_expansion=(10, 4, 0, 12)[i], constraint_trim=(14, 10, 0, 8)[i], split_threshold=split)
        out.append(_case("f_lX%d_split%d" % (lX, split), kw, _noisy_guide(rng, lX, max_indel=90, block=(5, 120)), rng))
    return out


FAMILIES = dict(a=family_a, b=family_b, c=family_c, e=family_e, f=family_f)


@functools.lru_cache(maxsize=None)
def cases(family):
    return tuple(FAMILIES[family]())


def groups(family):
    """the family's cases by their parameters: a batch has one set of parameters"""
    out = {}
    for c in cases(family):
        out.setdefault(tuple(sorted(c[1].items())), []).append(c)
    return [out[k] for k in sorted(out)]

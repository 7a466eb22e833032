"""Shared helpers for the test-suite (test infrastructure; may import oracle/)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as orc  # noqa: E402

MODEL_DIR = os.path.join(ROOT, "nanopore_amd", "mappers")


def load_model_arrays(name="blasr_hmm_0.txt"):
    """Independent (test-side) parser of the two-line HMM file: returns (T[25], E[80], likelihood)."""
    with open(os.path.join(MODEL_DIR, name)) as fh:
        l1 = fh.readline().split()
        l2 = fh.readline().split()
    assert len(l1) == 27 and len(l2) == 80
    return np.array(l1[1:26], dtype=np.float64), np.array(l2, dtype=np.float64), float(l1[26])


def oracle_hmm(name="blasr_hmm_0.txt"):
    T, E, _ = load_model_arrays(name)
    return orc.make_hmm(T, E)


def full_matrix_reference(T, E, X, Y, start=None, end=None):
    """Independent O(lX*lY) linear-space, UNBANDED forward/backward in numpy float64.

    Deliberately written in probability space (not log space) and row-by-row (not by anti-diagonal) so
    that it shares no structure with the oracle.  Valid for short sequences only (no scaling).
    Returns (total, posterior[lX, lY]) for the match state.
    """
    T = np.asarray(T).reshape(5, 5)
    Em = np.full((5, 5), 1.0 / 16.0)
    Em[:4, :4] = np.asarray(E[:16]).reshape(4, 4)
    Ex = np.full((5, 5), 0.25)
    Ey = np.full((5, 5), 0.25)
    for s in range(5):
        blk = np.asarray(E[16 * s:16 * s + 16]).reshape(4, 4)
        Ex[s, :4] = blk.sum(axis=1)
        Ey[s, :4] = blk.sum(axis=0)
    lX, lY = len(X), len(Y)
    if start is None:
        start = np.array([1.0, 0, 0, 0, 0])
    if end is None:
        end = T[:, 0].copy()
    F = np.zeros((lX + 1, lY + 1, 5))
    F[0, 0] = start
    for x in range(lX + 1):
        for y in range(lY + 1):
            if x == 0 and y == 0:
                continue
            if x > 0 and y > 0:
                F[x, y, 0] = Em[X[x - 1], Y[y - 1]] * (F[x - 1, y - 1] @ T[:, 0])
            if x > 0:
                for t in (1, 3):
                    F[x, y, t] = Ex[t, X[x - 1]] * (F[x - 1, y] @ T[:, t])
            if y > 0:
                for t in (2, 4):
                    F[x, y, t] = Ey[t, Y[y - 1]] * (F[x, y - 1] @ T[:, t])
    total = F[lX, lY] @ end
    B = np.zeros((lX + 1, lY + 1, 5))
    B[lX, lY] = end
    for x in range(lX, -1, -1):
        for y in range(lY, -1, -1):
            if x == lX and y == lY:
                continue
            acc = np.zeros(5)
            if x < lX and y < lY:
                acc += T[:, 0] * Em[X[x], Y[y]] * B[x + 1, y + 1, 0]
            if x < lX:
                for t in (1, 3):
                    acc += T[:, t] * Ex[t, X[x]] * B[x + 1, y, t]
            if y < lY:
                for t in (2, 4):
                    acc += T[:, t] * Ey[t, Y[y]] * B[x, y + 1, t]
            B[x, y] = acc
    post = F[1:, 1:, 0] * B[1:, 1:, 0] / total
    return total, post, F, B


def numpy_expectations(T, E, X, Y, start=None, end=None):
    """Baum-Welch expected counts (T[25], E[80]) and the total from full_matrix_reference's forward / backward: every term
    F(from) * t(from, to) * e(to) * B(to) / total, added up cell by cell.  A base N (code 4) is emitted with 1/16 (match) or 1/4
    (gap) and counted in the transitions, in no emission bin.  A gap state's emission is counted by its own base and spread as
    a quarter over the other sequence's four bases (the 80-entry layout of a model file)."""
    tot, _, F, B = full_matrix_reference(T, E, X, Y, start=start, end=end)
    Tm = np.asarray(T).reshape(5, 5)
    Em = np.full((5, 5), 1.0 / 16.0)
    Em[:4, :4] = np.asarray(E[:16]).reshape(4, 4)
    Ex = {s: np.append(np.asarray(E[16 * s:16 * s + 16]).reshape(4, 4).sum(axis=1), 0.25) for s in range(5)}
    Ey = {s: np.append(np.asarray(E[16 * s:16 * s + 16]).reshape(4, 4).sum(axis=0), 0.25) for s in range(5)}
    Texp, Eexp = np.zeros((5, 5)), np.zeros(80)
    for x in range(len(X) + 1):
        for y in range(len(Y) + 1):
            if x > 0 and y > 0:
                w = F[x - 1, y - 1] * Tm[:, 0] * Em[X[x - 1], Y[y - 1]] * B[x, y, 0] / tot
                Texp[:, 0] += w
                if X[x - 1] < 4 and Y[y - 1] < 4:
                    Eexp[X[x - 1] * 4 + Y[y - 1]] += w.sum()
            if x > 0:
                for t in (1, 3):
                    w = F[x - 1, y] * Tm[:, t] * Ex[t][X[x - 1]] * B[x, y, t] / tot
                    Texp[:, t] += w
                    if X[x - 1] < 4:
                        Eexp[t * 16 + X[x - 1] * 4:t * 16 + X[x - 1] * 4 + 4] += 0.25 * w.sum()
            if y > 0:
                for t in (2, 4):
                    w = F[x, y - 1] * Tm[:, t] * Ey[t][Y[y - 1]] * B[x, y, t] / tot
                    Texp[:, t] += w
                    if Y[y - 1] < 4:
                        Eexp[t * 16 + Y[y - 1]:t * 16 + 16:4] += 0.25 * w.sum()
    return Texp.reshape(-1), Eexp, tot


STATE_NAMES = ("match", "shortGapX", "shortGapY", "longGapX", "longGapY")


def count_name(i):
    """The name of entry i of the 105 counts (T[25] then E[80]): T[3][0], E[match][A][T], E[shortGapX][G][*], E[longGapY][*][C]."""
    if i < 25:
        return "T[%d][%d]" % (i // 5, i % 5)
    s, r = divmod(i - 25, 16)
    x, y = "ACGT"[r // 4], "ACGT"[r % 4]
    if s in (1, 3):
        y = "*"   # (a gap in the read: counted by the reference base, spread over the four read bases)
    elif s in (2, 4):
        x = "*"
    return "E[%s][%s][%s]" % (STATE_NAMES[s], x, y)


# Per-bin contract of the E-step counts against the fp64 oracle: |got - want| <= rel * want + floor on every one of the 25 + 80
# entries, and an entry the reference has at exactly 0 (a transition the model lacks, a bin only N bases would reach) is exactly 0.
#
# Why a relative bound per bin holds.  Each count is a sum of positive terms F(from) * t * e * B(to) / P.  The device keeps F, B
# and P in fp32 with an exponent beside them (per cell, per lane or per row: the kernel's choice), so each factor carries a relative
# error of a few 2^-24 per operation of its recursion; those errors are shared by F, B and P (P is the sum of F * B over any
# anti-diagonal) and largely cancel in the quotient.  The one place the precision is lower is the stripe E-step
# (k_dp_tile_cs<.., EM>), whose four gap-state forward values are kept as 24-bit floats with 15 mantissa bits: relative error
# at most 2^-16 = 1.5e-5 on the F factor of a gap-state term, once per term (the planes are written once and read once).  A sum
# of positive terms has a relative error no larger than the largest relative error of its terms, plus the rounding of the sum
# itself: fp32 per lane (n terms: at most (n - 1) * 2^-24, about sqrt(n) * 2^-24 for roundings of either sign, 4e-6 for the few
# thousand terms of a lane), then fp64.  So every bin stays within about 2e-5 of its own size on every path.  Measured on the
# MI355X (test_gpu_em.py's fixtures, every path and model): at most 5.5e-6 against the oracle, 1.3e-5 between two kernels (k_dp_wide
# against k_dp_generic, bands of 1500), on bins of at least 1 count; rel = 1e-4 is 8x above the worst.  Bins below 1 count -- a
# transition the band meets in a few cells, an emission a handful of bases make -- differ by at most 1e-6 counts; the floor,
# 1e-4 counts, is 100x above that and 2e-8 of the totals of these fixtures (5e3 - 2e4 transitions).
COUNTS_REL, COUNTS_FLOOR = 1e-4, 1e-4


def counts_error(got_T, got_E, want_T, want_E):
    """(worst relative error over the entries whose reference count is at least 1, worst absolute error over the others)."""
    got = np.concatenate([np.asarray(got_T, dtype=np.float64).reshape(-1), np.asarray(got_E, dtype=np.float64).reshape(-1)])
    want = np.concatenate([np.asarray(want_T, dtype=np.float64).reshape(-1), np.asarray(want_E, dtype=np.float64).reshape(-1)])
    big = want >= 1.0
    d = np.abs(got - want)
    return (float((d[big] / want[big]).max()) if big.any() else 0.0, float(d[~big].max()) if (~big).any() else 0.0)


def assert_counts_match(got_T, got_E, want_T, want_E, rel=COUNTS_REL, floor=COUNTS_FLOOR, what=""):
    """Every one of the 25 transition and 80 emission counts: finite, |got - want| <= rel * want + floor, and exactly 0 where the
    reference is exactly 0.  On failure the message names each failing entry with got, want and the relative error."""
    got = np.concatenate([np.asarray(got_T, dtype=np.float64).reshape(-1), np.asarray(got_E, dtype=np.float64).reshape(-1)])
    want = np.concatenate([np.asarray(want_T, dtype=np.float64).reshape(-1), np.asarray(want_E, dtype=np.float64).reshape(-1)])
    assert got.shape == want.shape == (105,), (got.shape, want.shape)
    bad = []
    for i in range(105):
        g, w = got[i], want[i]
        ok = np.isfinite(g) and (g == 0.0 if w == 0.0 else abs(g - w) <= rel * abs(w) + floor)
        if not ok:
            name = count_name(i)
            if name not in (b[0] for b in bad):
                bad.append((name, g, w))
    assert not bad, "%s: %d entries off (rel %.1e + floor %.1e): %s" % (
        what, len(bad), rel, floor, "; ".join("%s got %.9g want %.9g (rel %.2e)" % (n, g, w, abs(g - w) / abs(w) if w else float("inf"))
                                              for n, g, w in bad[:12]))


def random_pair(rng, lX, sub=0.1, indel=0.1, max_indel=3):
    """Random reference X and a noisy copy Y with the TRUE global alignment as (op,len) list."""
    X = rng.integers(0, 4, size=lX).astype(np.uint8)
    Y = []
    ops = []
    x = 0
    while x < lX:
        r = rng.random()
        if r < indel / 2:
            k = int(rng.integers(1, max_indel + 1))
            k = min(k, lX - x)
            ops.append((2, k))
            x += k
        elif r < indel:
            k = int(rng.integers(1, max_indel + 1))
            Y.extend(rng.integers(0, 4, size=k).tolist())
            ops.append((1, k))
        else:
            b = int(X[x])
            if rng.random() < sub:
                b = (b + int(rng.integers(1, 4))) % 4
            Y.append(b)
            ops.append((0, 1))
            x += 1
    merged = []
    for op, k in ops:
        if merged and merged[-1][0] == op:
            merged[-1] = (op, merged[-1][1] + k)
        else:
            merged.append((op, k))
    return X, np.array(Y, dtype=np.uint8), merged


def cigar_spans(ops):
    sx = sum(k for op, k in ops if op in (0, 2))
    sy = sum(k for op, k in ops if op in (0, 1))
    return sx, sy


def seg_arith_of(batch):
    """i -> which fp32 arithmetic the device ran each segment of read i in (Batch.segment_arith: 0 per-cell exponents, 1
    row-scaled), for orc.realign_read(..., precision=1, seg_arith=...): the mirror restates whichever the kernel class used."""
    off, ar = batch.segment_arith()
    return lambda i: ar[off[i]:off[i + 1]]

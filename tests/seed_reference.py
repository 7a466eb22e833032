"""References for the seed-mapper tests (test infrastructure): a literal restatement of the definition of a maximal exact match
(include/nprealign.h, "exact-match seeding") and a dictionary oracle for inputs too large for it."""
import numpy as np

from seed_mapper import revcomp

_CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def codes(seq):
    """npr_encode_bases' codes: A C G T -> 0..3 in either letter case, anything else -> 4."""
    return _CODE[np.frombuffer(seq.encode("ascii") if isinstance(seq, str) else seq, dtype=np.uint8)]


def matches_by_definition(refs, read, min_len):
    """The definition, cell by cell: E[a, b] = "reference base a and read base b match" (equal codes, both < 4; a code 4 matches
    nothing).  A match starts at a cell of E whose upper-left neighbour is outside the matrix or not in E (left-maximal), ends at a
    cell whose lower-right neighbour is outside or not in E (right-maximal), and is kept when it is min_len cells long.  One matrix
    per reference sequence, so nothing crosses from one into the next.  Sorted list of (reference index, a, b, L) for ONE
    orientation of the read."""
    out = []
    Y = codes(read)
    for r, ref in enumerate(refs):
        X = codes(ref)
        if not len(X) or not len(Y):
            continue
        E = (X[:, None] == Y[None, :]) & (X[:, None] < 4)
        starts = E.copy()
        starts[1:, 1:] &= ~E[:-1, :-1]
        ends = E.copy()
        ends[:-1, :-1] &= ~E[1:, 1:]
        # (only to keep the lists short: a match is 8 cells or more -- min_len >= k >= 8 -- so a start needs 8 cells of E down its
        # diagonal from itself on and an end 8 cells up to itself; run8[a, b] = E holds at (a, b) .. (a + 7, b + 7))
        assert min_len >= 8
        run8 = np.zeros_like(E)
        if min(E.shape) >= 8:
            n, m = E.shape[0] - 7, E.shape[1] - 7
            run8[:n, :m] = E[:n, :m]
            for t in range(1, 8):
                run8[:n, :m] &= E[t:t + n, t:t + m]
        starts &= run8
        ends[7:, 7:] &= run8[:-7, :-7]
        ends[:7, :] = False
        ends[:, :7] = False
        sa, sb = np.nonzero(starts)
        ea, eb = np.nonzero(ends)
        # along a diagonal starts and ends alternate: in (diagonal, a) order the q-th start belongs to the q-th end
        so, eo = np.lexsort((sa, sa - sb)), np.lexsort((ea, ea - eb))
        sa, sb, ea, eb = sa[so], sb[so], ea[eo], eb[eo]
        assert len(sa) == len(ea) and ((sa - sb) == (ea - eb)).all() and (ea >= sa).all()
        L = ea - sa + 1
        keep = L >= min_len
        out.extend((r, int(a), int(b), int(n)) for a, b, n in zip(sa[keep], sb[keep], L[keep]))
    return sorted(out)


def rows_by_definition(refs, read, min_len, strands=3):
    """What npr_seed_matches returns for one read: rows (reference index, a, b | strand << 31, L) sorted by (strand, reference, a, b)."""
    rows = []
    if strands & 1:
        rows += [(r, a, b, n) for r, a, b, n in matches_by_definition(refs, read, min_len)]
    if strands & 2:
        rows += [(r, a, b | (1 << 31), n) for r, a, b, n in matches_by_definition(refs, revcomp(read), min_len)]
    return rows


def as_rows(hits):
    """int32 rows from the library -> tuples comparable with rows_by_definition's (b | strand << 31 as an unsigned number)."""
    return [(int(r), int(a), int(b) & 0xffffffff, int(n)) for r, a, b, n in hits]


class DictionaryOracle(object):
    """Maximal exact matches through a Python dictionary of the reference's k-mers (tests/seed_mapper.py's way: look up every
    read k-mer, extend to both sides, remember the diagonal stretch already covered), the dictionary built once.  ACGT-only,
    upper-case input, one reference sequence."""

    def __init__(self, ref, k):
        self.ref, self.k = ref, k
        self.index = {}
        for i in range(len(ref) - k + 1):
            self.index.setdefault(ref[i:i + k], []).append(i)

    def matches(self, read, min_len):
        ref, k = self.ref, self.k
        done = {}  # diagonal -> read position up to which it is covered
        out = []
        for j in range(len(read) - k + 1):
            for i in self.index.get(read[j:j + k], ()):
                if done.get(i - j, -1) >= j:
                    continue
                a, b = i, j
                while a > 0 and b > 0 and ref[a - 1] == read[b - 1]:
                    a -= 1
                    b -= 1
                e, f = i + k, j + k
                while e < len(ref) and f < len(read) and ref[e] == read[f]:
                    e += 1
                    f += 1
                done[i - j] = f - k
                if e - a >= min_len:
                    out.append((0, a, b, e - a))
        return sorted(out)

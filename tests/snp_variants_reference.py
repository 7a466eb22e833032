"""A numpy restatement of the SNP-variant rule of include/nprealign.h (npr_snp_variants_table: CALLABLE, BEST, CALLS), written from the
header's text; nothing of the package is imported.  Besides the outputs it returns the three distances a test needs before it may compare
thresholded and floored values exactly with another implementation."""
import numpy as np

MAX_QUAL = 93


def snp_variants_reference(weights, seen, ref_code, error, threshold, evolution=None):
    """weights [rows, 4] >= 0, seen [rows], ref_code [rows] base codes 0..4, error 4 x 4 [candidate, observed], evolution 4 x 4
    [reference, candidate] (None: all ones), probabilities.  -> dict with
      best uint8[rows], qual uint8[rows], call_row int64[n], call_alt uint8[n], call_p float64[n]   (ascending (row, candidate))
      callable        bool[rows]
      threshold_gap   the smallest |p[c] - threshold| over every candidate c != ref of every callable row (inf: none)
      lp_gap          the smallest difference between the two largest lp of a callable row (inf: none; 0 at an exact tie)
      qual_gap        the smallest distance of -10 log10(q) from an integer over the callable rows with q > 0 (inf: none)"""
    w = np.asarray(weights, dtype=np.float64).reshape(-1, 4)
    rows = len(w)
    seen = np.asarray(seen).astype(bool).reshape(rows)
    ref = np.asarray(ref_code).astype(np.int64).reshape(rows)
    log_error = np.log(np.asarray(error, dtype=np.float64).reshape(4, 4))
    with np.errstate(divide="ignore"):
        log_evolution = np.log(np.ones((4, 4)) if evolution is None else np.asarray(evolution, dtype=np.float64).reshape(4, 4))
    total = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    callable_ = seen & (total != 0.0) & (ref <= 3)
    at = np.flatnonzero(callable_)
    best, qual = np.full(rows, 4, dtype=np.uint8), np.zeros(rows, dtype=np.uint8)
    out = dict(best=best, qual=qual, callable=callable_, call_row=np.zeros(0, dtype=np.int64), call_alt=np.zeros(0, dtype=np.uint8),
               call_p=np.zeros(0, dtype=np.float64), threshold_gap=np.inf, lp_gap=np.inf, qual_gap=np.inf)
    if not len(at):
        return out
    r = ref[at]
    f = w[at] / total[at, None]
    lp = np.empty((len(at), 4))
    for c in range(4):
        s = np.zeros(len(at))
        for o in range(4):
            s = s + f[:, o] * log_error[c, o]
        lp[:, c] = log_evolution[r, c] + s
    top = lp.max(axis=1)
    e = np.exp(lp - top[:, None])
    total_e = ((e[:, 0] + e[:, 1]) + e[:, 2]) + e[:, 3]
    p = e / total_e[:, None]
    # BEST: largest lp; among exactly equal ones the reference base if it is one of them, else the lowest code
    on_top = lp == top[:, None]
    b = np.where(on_top[np.arange(len(at)), r], r, on_top.argmax(axis=1))
    others = np.zeros(len(at))
    for c in range(4):
        others = others + np.where(b == c, 0.0, e[:, c])
    q = others / total_e
    with np.errstate(divide="ignore"):
        phred = -10.0 * np.log10(q)
    best[at] = b
    qual[at] = np.where(q == 0.0, MAX_QUAL, np.minimum(MAX_QUAL, np.floor(np.where(q == 0.0, 1.0, phred)))).astype(np.uint8)
    # CALLS
    not_ref = np.arange(4)[None, :] != r[:, None]
    called = not_ref & (p >= threshold)
    which_row, which_c = np.nonzero(called)   # row-major: ascending (row, candidate)
    out.update(call_row=at[which_row].astype(np.int64), call_alt=which_c.astype(np.uint8), call_p=p[which_row, which_c])
    out["threshold_gap"] = float(np.abs(p - threshold)[not_ref].min())
    ordered = np.sort(lp, axis=1)
    with np.errstate(invalid="ignore"):
        gap = ordered[:, 3] - ordered[:, 2]
    out["lp_gap"] = float(np.nanmin(gap))
    finite = phred[q > 0.0]
    if len(finite):
        out["qual_gap"] = float(np.abs(finite - np.rint(finite)).min())
    return out

"""numpy restatement of the per-subject hit lists (include/bgsa_hip.h "hit lists per subject") — a helper, not a test.

The contract is the row contract of hits_reference applied to the transposed valid part of the tile: a candidate is
(score, query id), the id of row r is query_base + r, ids are int32, one list per column below valid_count.
"""
import numpy as np

import hits_reference as H

INT32_MIN, INT32_MAX = H.INT32_MIN, H.INT32_MAX
worst = H.worst


def _columns(tile, valid_count):
    return np.ascontiguousarray(np.asarray(tile)[:, :valid_count].T)


def top_queries(tile, valid_count: int, k_best: int, smallest: bool, query_base: int = 0, into=None):
    """(scores[valid, K] int32, queries[valid, K] int32), best first.  into=(scores, queries): accumulate."""
    cols = _columns(tile, valid_count)
    s, q = H.top_hits(cols, cols.shape[1], k_best, smallest, subject_base=query_base, into=into)
    return s, q.astype(np.int32)


def threshold_queries(tile, valid_count: int, cutoff: int, smallest: bool, cap_per_subject: int, query_base: int = 0, into=None):
    """(counts[valid] int32, scores[valid, cap] int32, queries[valid, cap] int32) in ascending query order; slots behind a
    column's hits hold (0, -1) unless `into` held something else: compare with `threshold_lists_equal`."""
    cols = _columns(tile, valid_count)
    c, s, q = H.threshold_hits(cols, cols.shape[1], cutoff, smallest, cap_per_subject, subject_base=query_base, into=into)
    return c, s, q.astype(np.int32)


threshold_lists_equal = H.threshold_lists_equal


def brute_top_queries(tile, valid_count, k_best, smallest, query_base=0, into=None):
    """The same by plain Python loops over the columns (checks the helper itself on tiny cases)."""
    rows = np.asarray(tile).tolist()
    out_s = np.full((valid_count, k_best), worst(smallest), dtype=np.int32)
    out_q = np.full((valid_count, k_best), -1, dtype=np.int32)
    for c in range(valid_count):
        cands = [(row[c], query_base + r) for r, row in enumerate(rows)]
        if into is not None:
            cands += [(int(s), int(q)) for s, q in zip(into[0][c], into[1][c]) if q >= 0]
        for slot in range(min(k_best, len(cands))):
            best = None
            for s, q in cands:
                if best is None or (s < best[0] if smallest else s > best[0]) or (s == best[0] and q < best[1]):
                    best = (s, q)
            cands.remove(best)
            out_s[c, slot], out_q[c, slot] = best
    return out_s, out_q

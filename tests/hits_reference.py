"""numpy restatement of the hit-selection contract (include/bgsa_hip.h "hit selection") — a helper, not a test.

One total order: a candidate is (score, subject id); better = the larger score (the smaller one with `smallest`), among
equal scores the smaller subject id.  Only the first `valid_count` columns of a tile are candidates; the subject id of
column c is subject_base + c.  Unused slots hold subject -1 and the worst int32 of the direction.
"""
import numpy as np

INT32_MIN, INT32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max


def worst(smallest: bool) -> int:
    return INT32_MAX if smallest else INT32_MIN


def top_hits(tile: np.ndarray, valid_count: int, k_best: int, smallest: bool, subject_base: int = 0, into=None):
    """(scores[nq, K] int32, subjects[nq, K] int64), best first.  into=(scores, subjects): those entries join the
    candidates with their subject ids as stored (accumulate)."""
    tile = np.asarray(tile)
    nq = tile.shape[0]
    cand_s = tile[:, :valid_count].astype(np.int64)
    cand_j = np.broadcast_to(np.arange(valid_count, dtype=np.int64) + subject_base, cand_s.shape)
    if into is not None:
        cand_s = np.concatenate([np.asarray(into[0], dtype=np.int64), cand_s], axis=1)
        cand_j = np.concatenate([np.asarray(into[1], dtype=np.int64), cand_j], axis=1)
    return merge(cand_s, cand_j, k_best, smallest)


def merge(cand_scores: np.ndarray, cand_subjects: np.ndarray, k_best: int, smallest: bool):
    """The k_best best of [nq, n] candidate lists (subject -1 = unused slot, never chosen): np.lexsort on
    (subject, +-score) per row."""
    nq = cand_scores.shape[0]
    out_s = np.full((nq, k_best), worst(smallest), dtype=np.int32)
    out_j = np.full((nq, k_best), -1, dtype=np.int64)
    for r in range(nq):
        live = cand_subjects[r] >= 0
        s, j = cand_scores[r][live], cand_subjects[r][live]
        order = np.lexsort((j, s if smallest else -s))[:k_best]      # last key is the primary one
        out_s[r, : order.size] = s[order]
        out_j[r, : order.size] = j[order]
    return out_s, out_j


def threshold_hits(tile: np.ndarray, valid_count: int, cutoff: int, smallest: bool, cap_per_query: int, subject_base: int = 0,
                   into=None):
    """(counts[nq] int32 — the true numbers, scores[nq, cap] int32, subjects[nq, cap] int64) in ascending subject order;
    on overflow the cap lowest-indexed hits.  Slots behind a row's hits are filled with (0, -1) here: the library
    leaves them as they were, so compare with `threshold_lists_equal`.  into=(counts, scores, subjects): appended behind."""
    tile = np.asarray(tile)
    nq = tile.shape[0]
    if into is None:
        counts = np.zeros(nq, dtype=np.int32)
        scores = np.zeros((nq, cap_per_query), dtype=np.int32)
        subjects = np.full((nq, cap_per_query), -1, dtype=np.int64)
    else:
        counts, scores, subjects = (np.array(x) for x in into)
    for r in range(nq):
        row = tile[r, :valid_count].astype(np.int64)
        cols = np.nonzero(row <= cutoff if smallest else row >= cutoff)[0]
        at = int(counts[r])
        keep = cols[: max(0, cap_per_query - at)]
        scores[r, at: at + keep.size] = row[keep]
        subjects[r, at: at + keep.size] = keep + subject_base
        counts[r] = at + cols.size
    return counts, scores, subjects


def threshold_lists_equal(got, want, cap_per_query: int) -> bool:
    """Counts equal, and the lists equal in the slots the counts cover."""
    gc, gs, gj = (np.asarray(x) for x in got)
    wc, ws, wj = (np.asarray(x) for x in want)
    if not np.array_equal(gc, wc):
        return False
    for r in range(gc.shape[0]):
        n = min(int(wc[r]), cap_per_query)
        if not (np.array_equal(gs[r, :n], ws[r, :n]) and np.array_equal(gj[r, :n], wj[r, :n])):
            return False
    return True


def brute_top_hits(tile, valid_count, k_best, smallest, subject_base=0):
    """The same by a plain Python loop (checks the helper itself on tiny cases)."""
    out_s, out_j = [], []
    for row in np.asarray(tile).tolist():
        cands = [(s, c + subject_base) for c, s in enumerate(row[:valid_count])]
        chosen = []
        for _ in range(k_best):
            best = None
            for s, j in cands:
                if (s, j) in chosen:
                    continue
                if best is None or (s < best[0] if smallest else s > best[0]) or (s == best[0] and j < best[1]):
                    best = (s, j)
            if best is None:
                best = (worst(smallest), -1)
            else:
                chosen.append(best)
            out_s.append(best[0])
            out_j.append(best[1])
    n = len(out_s) // k_best
    return np.array(out_s, dtype=np.int32).reshape(n, k_best), np.array(out_j, dtype=np.int64).reshape(n, k_best)

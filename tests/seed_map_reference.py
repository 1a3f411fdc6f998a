"""numpy / Python restatement of "seeded read mapping" (include/bgsa_hip.h) — a helper, not a test.

The index, the pieces, the candidate rule, the flags, deduplication, selection and blanking, each stated again from the header's
text on plain Python integers; nothing here calls the library.  Windows, ids and strands are those of
tests/reference_map_reference.py.
"""
import numpy as np

import reference_map_reference as M
from align_reference import classes

INT32_MIN = -2 ** 31
SEED_LEN_MAX = 13


# ---- index ----------------------------------------------------------------------------------------------------------------
def buckets_of(ref_codes, q: int) -> dict:
    """value -> the ascending positions p whose k-mer ref[p .. p + q) has that value; a k-mer with a code 4 is left out."""
    ref_codes = np.asarray(ref_codes, dtype=np.int64)
    buckets = {}
    for p in range(ref_codes.size - q + 1):
        piece = ref_codes[p: p + q]
        if (piece < 4).all():
            value = 0
            for c in piece:
                value = value * 4 + int(c)
            buckets.setdefault(value, []).append(p)
    return buckets


def index(ref_codes, q: int):
    """(offsets int64[4^q + 1], positions int64, ascending inside every bucket): bucket c = positions[offsets[c] : offsets[c + 1]]."""
    buckets = buckets_of(ref_codes, q)
    offsets = np.zeros(4 ** q + 1, dtype=np.int64)
    for value, where in buckets.items():
        offsets[value + 1] = len(where)
    offsets = np.cumsum(offsets)
    positions = np.zeros(int(offsets[-1]), dtype=np.int64)
    for value, where in buckets.items():
        positions[offsets[value]: offsets[value + 1]] = sorted(where)
    return offsets, positions


def sorted_buckets(offsets, positions) -> np.ndarray:
    """positions with every bucket sorted: the order inside a bucket is unspecified."""
    out = np.array(positions, dtype=np.int64)
    offsets = np.asarray(offsets, dtype=np.int64)
    for c in np.flatnonzero(np.diff(offsets) > 1):
        out[offsets[c]: offsets[c + 1]].sort()
    return out


# ---- pieces ---------------------------------------------------------------------------------------------------------------
def plan(n: int, max_distance: int, seed_len=None):
    """(B, step, q), or None where step < q."""
    B = min(max_distance, n)
    step = n // (B + 1)
    q = min(12, step) if seed_len is None else seed_len
    return (B, step, q) if 1 <= q <= step else None


def piece_starts(n: int, B: int) -> list:
    step = n // (B + 1)
    return [j * step for j in range(B + 1)]


def strands_of(read_ascii, both_strands: bool = True) -> list:
    """The class rows the pieces are cut from: the read, and its reverse complement."""
    codes = classes(np.asarray(read_ascii, dtype=np.uint8))
    return [codes, M.comp(codes[::-1])] if both_strands else [codes]


def has_n_piece(read_ascii, B: int, q: int, both_strands: bool = True) -> bool:
    n = len(read_ascii)
    return any((row[o: o + q] == 4).any() for row in strands_of(read_ascii, both_strands) for o in piece_starts(n, B))


# ---- candidates -----------------------------------------------------------------------------------------------------------
def lookup_of(offsets, positions):
    return lambda value: positions[offsets[value]: offsets[value + 1]]


def candidates(lookup, L: int, W: int, S: int, read_ascii, B: int, q: int, both_strands: bool = True) -> list:
    """Every (occurrence, window) candidate of one read as a window id, with repetitions, in no particular order.  lookup(value)
    = the positions of that k-mer: lookup_of(offsets, positions), or buckets_of(...).get with a default."""
    n = len(read_ascii)
    n_windows = M.window_count(L, W, S)
    starts = [M.window_start(L, W, S, w) for w in range(n_windows)]
    out = []
    for strand, row in enumerate(strands_of(read_ascii, both_strands)):
        for o in piece_starts(n, B):
            value = 0
            for c in row[o: o + q]:
                value = value * 4 + int(c) % 4
            for p in lookup(value):
                p = int(p)
                for w, at in enumerate(starts):
                    if at <= p and p + q <= at + W and at <= p - o + B and p - o + n - B <= at + W:
                        out.append(strand * n_windows + w)
    return out


def count_or_flag(cands: list, n_piece: bool, max_candidates: int) -> int:
    if n_piece:
        return -1
    return -2 if len(cands) > max_candidates else len(cands)


def deduplicate(cands: list) -> list:
    return sorted(set(cands))


# ---- selection and blanking -----------------------------------------------------------------------------------------------
def select(ids, distances, B: int, k: int):
    """(scores[k], windows[k]) of one read: the k best candidates within B by (distance ascending, id ascending)."""
    order = sorted((int(d), int(g)) for g, d in zip(ids, distances) if 0 <= d <= B)[:k]
    scores = [-d for d, _ in order] + [INT32_MIN] * (k - len(order))
    windows = [g for _, g in order] + [-1] * (k - len(order))
    return np.array(scores, dtype=np.int32), np.array(windows, dtype=np.int32)


def blank(hits, B: int) -> dict:
    """map_reads' result (a ReferenceHits or map_reads_host's dict) with every slot beyond B blanked."""
    get = (lambda name: hits[name]) if isinstance(hits, dict) else (lambda name: getattr(hits, name))
    scores, windows = np.asarray(get("scores")), np.asarray(get("windows"))
    gone = (windows < 0) | (-scores.astype(np.int64) > B)
    out = dict(scores=np.where(gone, INT32_MIN, scores).astype(np.int32), windows=np.where(gone, -1, windows).astype(np.int32),
               strand=np.where(gone, -1, get("strand")).astype(np.int32), keep=np.where(gone, 0, get("keep")).astype(np.int32),
               ref_begin=np.where(gone, -1, get("ref_begin")).astype(np.int64), ref_end=np.where(gone, -1, get("ref_end")).astype(np.int64))
    out["cigars"] = [[None if gone[c, r] else text for r, text in enumerate(row)] for c, row in enumerate(get("cigars"))]
    return out


# ---- brute force ----------------------------------------------------------------------------------------------------------
def window_distances(ref_ascii, W: int, S: int, read_ascii, both_strands: bool = True) -> np.ndarray:
    """The semi-global unit-cost distance of the read inside every window id, by plain DP over the classes (N matches N)."""
    ref_codes = classes(np.asarray(ref_ascii, dtype=np.uint8))
    n_windows = M.window_count(ref_codes.size, W, S)
    rows = M.window_rows(ref_codes, W, S, range(n_windows * (2 if both_strands else 1))).astype(np.int64)
    read = classes(np.asarray(read_ascii, dtype=np.uint8))
    n = read.size
    ramp = np.arange(n + 1, dtype=np.int64)
    d = np.tile(ramp, (rows.shape[0], 1))
    best = d[:, n].copy()
    for i in range(W):
        t = np.empty_like(d)
        t[:, 0] = 0
        np.minimum(d[:, 1:] + 1, d[:, :-1] + (rows[:, i: i + 1] != read[None, :]), out=t[:, 1:])
        d = np.minimum.accumulate(t - ramp, axis=1) + ramp
        np.minimum(best, d[:, n], out=best)
    return best

"""numpy / Python restatement of "a reference as the query set" (include/bgsa_hip.h) — a helper, not a test.

The geometry, the window rows, the coordinate rule, the reversal of a reverse hit's runs and `keep`, each stated again from the
header's text, and map_reads_host: the whole of bgsa_amd.reference.ReferenceMapper.map_reads on the host — windows cut here,
per-window results from trace_reference (FREE_QUERY, 0 / -1 / -1) and place_reference, the list order of query_hits_reference.
"""
import numpy as np

import place_reference as R
import query_hits_reference as Q
import trace_reference as T
from align_reference import classes

LETTERS = np.frombuffer(b"ACGTN", dtype=np.uint8)
CIGAR_CHAR = {1: "I", 2: "D", 7: "=", 8: "X"}


# ---- geometry -------------------------------------------------------------------------------------------------------------
def window_count(L: int, W: int, S: int) -> int:
    assert 1 <= S <= W <= L
    return 1 + (L - W + S - 1) // S


def window_start(L: int, W: int, S: int, w: int) -> int:
    assert 0 <= w < window_count(L, W, S)
    return min(w * S, L - W)


def largest_stride(W: int, n: int, max_distance: int) -> int:
    return W - (n + min(max_distance, n)) + 1


# ---- window rows ----------------------------------------------------------------------------------------------------------
def comp(codes):
    codes = np.asarray(codes, dtype=np.int64)
    return np.where(codes < 4, 3 - codes, 4)


def window_rows(ref_codes, W: int, S: int, ids) -> np.ndarray:
    """[len(ids), W] uint8 codes: the row of every window id; an id outside [0, 2 n_windows) is a row of 4."""
    ref_codes = np.asarray(ref_codes, dtype=np.int64)
    L = ref_codes.size
    n = window_count(L, W, S)
    out = np.full((len(ids), W), 4, dtype=np.uint8)
    for r, g in enumerate(int(x) for x in ids):
        if 0 <= g < n:
            at = window_start(L, W, S, g)
            out[r] = ref_codes[at: at + W]
        elif n <= g < 2 * n:
            at = window_start(L, W, S, g - n)
            out[r] = comp(ref_codes[at: at + W][::-1])
    return out


def rows_buffer(rows: np.ndarray) -> np.ndarray:
    """The flat content buffer: W codes and a newline per row."""
    buf = np.full((rows.shape[0], rows.shape[1] + 1), ord("\n"), dtype=np.uint8)
    buf[:, :-1] = rows
    return buf.reshape(-1)


def reverse_complement(ascii_seq) -> np.ndarray:
    """ASCII in, ASCII out, through the codes: a byte outside the alphabet is class 0 ('A') and comes back as 'T'."""
    return LETTERS[comp(classes(np.asarray(ascii_seq, dtype=np.uint8))[::-1])]


# ---- coordinates, runs, keep ----------------------------------------------------------------------------------------------
def reverse_runs(n_ops: int, row: np.ndarray, cap: int) -> np.ndarray:
    row = np.array(row)
    if 0 < n_ops <= cap:
        row[:n_ops] = row[:n_ops][::-1]
    return row


def keep_of(strand, begin, end) -> np.ndarray:
    """One read's list, best first."""
    keep = np.zeros(len(strand), dtype=np.int32)
    for r in range(len(strand)):
        if begin[r] < 0:
            continue
        hidden = any(keep[q] and strand[q] == strand[r] and begin[q] < end[r] and begin[r] < end[q] for q in range(r))
        keep[r] = 0 if hidden else 1
    return keep


def placements(L: int, W: int, S: int, hit_windows, span, n_ops, cigar, cap: int):
    """bgsa_hip_reference_placements_dev: (strand, ref_begin, ref_end, keep, cigar) for hit_windows[n_reads, k], span[n_reads * k, 4],
    n_ops[n_reads * k], cigar[n_reads * k, cap]; the inputs are not modified."""
    hit_windows = np.asarray(hit_windows)
    n_reads, k = hit_windows.shape
    n = window_count(L, W, S)
    span = np.asarray(span).reshape(n_reads * k, 4)
    n_ops = np.asarray(n_ops).reshape(-1)
    cigar = np.array(cigar).reshape(n_reads * k, cap)
    strand = np.full((n_reads, k), -1, dtype=np.int32)
    begin = np.full((n_reads, k), -1, dtype=np.int64)
    end = np.full((n_reads, k), -1, dtype=np.int64)
    keep = np.zeros((n_reads, k), dtype=np.int32)
    for c in range(n_reads):
        for r in range(k):
            g, p = int(hit_windows[c, r]), c * k + r
            if not 0 <= g < 2 * n:
                continue
            strand[c, r] = g >= n
            qb, qe = int(span[p, 0]), int(span[p, 1])
            if qb < 0:
                continue
            at = window_start(L, W, S, g % n)
            if g < n:
                begin[c, r], end[c, r] = at + qb, at + qe
            else:
                begin[c, r], end[c, r] = at + W - qe, at + W - qb
                cigar[p] = reverse_runs(int(n_ops[p]), cigar[p], cap)
        keep[c] = keep_of(strand[c], begin[c], end[c])
    return strand, begin, end, keep, cigar


def runs_text(runs) -> str:
    return "".join(f"{length}{CIGAR_CHAR[op]}" for length, op in runs)


# ---- the whole pipeline on the host -----------------------------------------------------------------------------------------
def window_scores(windows_ascii: np.ndarray, reads: np.ndarray, chunk: int = 16) -> np.ndarray:
    """tile[nq, ns]: the Myers semi-global score (minus the distance of the read end to end inside the window)."""
    nq, ns = windows_ascii.shape[0], reads.shape[0]
    n = reads.shape[1]
    tile = np.empty((nq, ns), dtype=np.int32)
    for lo in range(0, nq, chunk):
        rows = windows_ascii[lo: lo + chunk]
        h = T.h_matrices(np.repeat(rows, ns, axis=0), np.tile(reads, (rows.shape[0], 1)), T.FREE_QUERY, T.UNIT)
        tile[lo: lo + chunk] = h[:, :, n].max(axis=1).reshape(rows.shape[0], ns)
    return tile


def map_reads_host(reference, W: int, S: int, reads, k_best: int = 1, max_distance=None, both_strands: bool = True):
    """dict(scores, windows, strand, ref_begin, ref_end, keep, cigars) as ReferenceMapper.map_reads returns them."""
    reference = np.frombuffer(bytes(reference), dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else np.asarray(reference, np.uint8)
    reads = np.asarray(reads, dtype=np.uint8)
    L, (ns, n) = reference.size, reads.shape
    n_windows = window_count(L, W, S)
    n_ids = n_windows * (2 if both_strands else 1)
    k_sel = min(64, k_best * (-(-W // S) + 1))
    rows = window_rows(classes(reference), W, S, range(n_ids))
    windows_ascii = LETTERS[rows]
    tile = window_scores(windows_ascii, reads)
    scores, ids = Q.top_queries(tile, ns, k_sel, False)
    if max_distance is None:
        max_distance = int(-np.where(ids >= 0, scores, 0).min())
    span = np.full((ns * k_sel, 4), -1, dtype=np.int32)
    n_ops = np.zeros(ns * k_sel, dtype=np.int32)
    runs_of = {}
    qc, sc = classes(windows_ascii), classes(reads)
    for c in range(ns):
        for r in range(k_sel):
            g, p = int(ids[c, r]), c * k_sel + r
            if g < 0:
                continue
            dist, e, q_begin, runs, _ = R.place(qc[g], sc[c], max_distance)
            assert dist == -scores[c, r]
            span[p] = (-1 if q_begin is None else q_begin, e, 0, n)
            n_ops[p] = len(runs)
            runs_of[p] = runs
    cap = max(1, int(n_ops.max(initial=0)))
    cigar = np.zeros((ns * k_sel, cap), dtype=np.int64)
    for p, runs in runs_of.items():
        cigar[p, : len(runs)] = [length << 4 | op for length, op in runs]
    strand, begin, end, keep, cigar = placements(L, W, S, ids, span, n_ops, cigar, cap)
    cigars = [[runs_text([(int(w) >> 4, int(w) & 15) for w in cigar[c * k_sel + r, : n_ops[c * k_sel + r]]]) if keep[c, r] else None
               for r in range(k_sel)] for c in range(ns)]
    return dict(scores=scores, windows=ids, strand=strand, ref_begin=begin, ref_end=end, keep=keep, cigars=cigars)

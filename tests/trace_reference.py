"""numpy restatement of the contract of bgsa_hip_trace_pairs_dev (include/bgsa_hip.h "score, span and edit script of selected
pairs") — a helper, not a test.

The full linear-gap DP matrix over the library's character classes, H[i][j] = max(H[i-1][j-1] + s(i, j), H[i-1][j] + gap,
H[i][j-1] + gap) with s = match for equal classes and mismatch otherwise, in three modes:

    GLOBAL        H[0][j] = j*gap, H[i][0] = i*gap; score H[m][n] at (m, n); the walk back stops at (0, 0)
    FREE_QUERY    (Myers semi-global: the subject end to end inside the query) H[0][j] = j*gap, H[i][0] = 0; score = the max
                  over i of H[i][n] at the SMALLEST such i; the walk back stops at the first cell with j = 0
    FREE_SUBJECT  (BitPAl semi-global: the query end to end, free subject overhangs) H[0][j] = 0, H[i][0] = i*gap; score =
                  the max over j of H[m][j] at the SMALLEST such j; the walk back stops at the first cell with i = 0

the ONE canonical walk through it (diagonal first, then up 'I', then left 'D'; on a non-free edge the one possible step), and
a validator for any (score, span, runs).  span = (q_begin, q_end, s_begin, s_end), half-open; runs are (length, op) in query
order over the aligned span only, ops and packing as in align_reference.
"""
import numpy as np

from align_reference import OP_D, OP_EQ, OP_I, OP_X, OP_CHAR, classes  # noqa: F401

GLOBAL, FREE_QUERY, FREE_SUBJECT = 0, 1, 2
MODES = (GLOBAL, FREE_QUERY, FREE_SUBJECT)
UNIT = (0, -1, -1)


def h_matrices(queries: np.ndarray, subjects: np.ndarray, mode: int, scores) -> np.ndarray:
    """H[p, i, j] for pair p = (queries[p], subjects[p]) — ASCII rows [P, m] and [P, n] — one numpy row step per DP row:
    the left dependency H[i][j] = max(t[j], H[i][j-1] + gap) is maximum.accumulate(t - ramp) + ramp with ramp = j*gap."""
    match, mismatch, gap = (int(x) for x in scores)
    qc, sc = classes(queries), classes(subjects)
    pairs, m = qc.shape
    n = sc.shape[1]
    ramp = np.arange(n + 1, dtype=np.int32) * gap
    h = np.empty((pairs, m + 1, n + 1), dtype=np.int32)
    h[:, 0, :] = 0 if mode == FREE_SUBJECT else ramp
    for i in range(1, m + 1):
        prev = h[:, i - 1, :]
        t = np.empty((pairs, n + 1), dtype=np.int32)
        t[:, 0] = 0 if mode == FREE_QUERY else i * gap
        np.maximum(prev[:, 1:] + gap, prev[:, :-1] + np.where(qc[:, i - 1: i] == sc, match, mismatch), out=t[:, 1:])
        h[:, i, :] = np.maximum.accumulate(t - ramp, axis=1) + ramp
    return h


def end_cell(h: np.ndarray, mode: int):
    """(score, i, j) of one pair's matrix h[m+1, n+1]: np.argmax returns the first — the smallest — index of the maximum."""
    m, n = h.shape[0] - 1, h.shape[1] - 1
    if mode == GLOBAL:
        return int(h[m, n]), m, n
    if mode == FREE_QUERY:
        i = int(np.argmax(h[:, n]))
        return int(h[i, n]), i, n
    j = int(np.argmax(h[m, :]))
    return int(h[m, j]), m, j


def walk(h: np.ndarray, qc, sc, mode: int, scores):
    """The canonical (score, span, runs) through one pair's matrix."""
    match, mismatch, gap = (int(x) for x in scores)
    score, i, j = end_cell(h, mode)
    q_end, s_end = i, j
    h = h.tolist()
    qc, sc = list(qc), list(sc)
    ops = []
    while not ((i == 0 and j == 0) if mode == GLOBAL else (j == 0 if mode == FREE_QUERY else i == 0)):
        if i == 0:
            ops.append(OP_D)
            j -= 1
        elif j == 0:
            ops.append(OP_I)
            i -= 1
        else:
            same = qc[i - 1] == sc[j - 1]
            if h[i - 1][j - 1] + (match if same else mismatch) == h[i][j]:
                ops.append(OP_EQ if same else OP_X)
                i -= 1
                j -= 1
            elif h[i - 1][j] + gap == h[i][j]:
                ops.append(OP_I)
                i -= 1
            else:
                assert h[i][j - 1] + gap == h[i][j]
                ops.append(OP_D)
                j -= 1
    ops.reverse()
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return score, (i, q_end, j, s_end), [(length, op) for length, op in runs]


def canonical(queries: np.ndarray, subjects: np.ndarray, mode: int, scores):
    """Per pair p = (queries[p], subjects[p]): a list of (score, span, runs)."""
    h = h_matrices(queries, subjects, mode, scores)
    qc, sc = classes(queries), classes(subjects)
    return [walk(h[p], qc[p], sc[p], mode, scores) for p in range(qc.shape[0])]


def validate(query: np.ndarray, subject: np.ndarray, mode: int, scores, score: int, span, runs) -> None:
    """Asserts that `runs` aligns query[q_begin:q_end] with subject[s_begin:s_end], that the span touches the non-free
    edges of `mode`, and that the runs are worth exactly `score` under `scores`."""
    match, mismatch, gap = (int(x) for x in scores)
    qc, sc = classes(query), classes(subject)
    q_begin, q_end, s_begin, s_end = (int(x) for x in span)
    assert 0 <= q_begin <= q_end <= qc.size and 0 <= s_begin <= s_end <= sc.size, span
    if mode != FREE_QUERY:
        assert (q_begin, q_end) == (0, qc.size), f"the query is aligned end to end in this mode, span {span}"
    if mode != FREE_SUBJECT:
        assert (s_begin, s_end) == (0, sc.size), f"the subject is aligned end to end in this mode, span {span}"
    i, j, worth = q_begin, s_begin, 0
    last = None
    for length, op in runs:
        assert length >= 1 and op in OP_CHAR, (length, op)
        assert op != last, "adjacent runs carry the same op"
        last = op
        if op in (OP_EQ, OP_X):
            assert i + length <= q_end and j + length <= s_end, "the script runs past the span"
            same = qc[i: i + length] == sc[j: j + length]
            assert same.all() if op == OP_EQ else not same.any(), ("'=' over different or 'X' over equal classes", i, j)
            i += length
            j += length
            worth += length * (match if op == OP_EQ else mismatch)
        elif op == OP_I:
            i += length
            worth += length * gap
        else:
            j += length
            worth += length * gap
    assert (i, j) == (q_end, s_end), f"the script ends at {(i, j)}, the span at {(q_end, s_end)}"
    assert worth == score, f"the runs are worth {worth}, the score is {score}"

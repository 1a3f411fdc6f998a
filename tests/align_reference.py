"""numpy restatement of the pair-alignment contract (include/bgsa_hip.h "alignment of selected pairs") — a helper, not a test.

The full unit-cost DP matrix over the library's character classes (mapping_table: A C G T N -> 0..4, anything else 0),
the ONE canonical traceback through it, and a validator for any edit script.

Canonical script: the path found walking back from (m, n); at a cell (i, j), i, j > 0: the diagonal if
D[i-1][j-1] + [q_i != s_j] == D[i][j], otherwise up ('I', a query character only) if D[i-1][j] + 1 == D[i][j], otherwise
left ('D', a subject character only); at i == 0 only 'D', at j == 0 only 'I'.  Runs are (length, op) in query order from
the first column, op = the BAM codes below, packed as length << 4 | op.
"""
import re

import numpy as np

OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OP_CHAR = {OP_I: "I", OP_D: "D", OP_EQ: "=", OP_X: "X"}
CHAR_OP = {c: o for o, c in OP_CHAR.items()}


def class_table() -> np.ndarray:
    """256 entries: the library's mapping_table for bytes below 128, class 0 for the rest (map_char of preprocess.hip)."""
    table = np.zeros(256, dtype=np.int64)
    for ch, c in zip(b"ACGTN", range(5)):
        table[ch] = c
    return table


def classes(rows: np.ndarray) -> np.ndarray:
    return class_table()[np.asarray(rows, dtype=np.uint8)]


def dp_matrices(queries: np.ndarray, subjects: np.ndarray) -> np.ndarray:
    """D[p, i, j] for pair p = (queries[p], subjects[p]) — ASCII rows [P, m] and [P, n] — one numpy row step per DP row:
    the left dependency D[i][j] = min(t[j], D[i][j-1] + 1) is minimum.accumulate(t - arange) + arange."""
    qc, sc = classes(queries), classes(subjects)
    pairs, m = qc.shape
    n = sc.shape[1]
    ramp = np.arange(n + 1, dtype=np.int32)
    d = np.empty((pairs, m + 1, n + 1), dtype=np.int32)
    d[:, 0, :] = ramp
    for i in range(1, m + 1):
        prev = d[:, i - 1, :]
        t = np.empty((pairs, n + 1), dtype=np.int32)
        t[:, 0] = i
        np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (qc[:, i - 1: i] != sc), out=t[:, 1:])
        d[:, i, :] = np.minimum.accumulate(t - ramp, axis=1) + ramp
    return d


def traceback(d: np.ndarray, qc: np.ndarray, sc: np.ndarray):
    """The canonical script through one pair's matrix d[m+1, n+1]: (distance, [(length, op), ...])."""
    d = d.tolist()
    qc, sc = list(qc), list(sc)
    i, j = len(qc), len(sc)
    ops = []
    while i > 0 or j > 0:
        if i == 0:
            ops.append(OP_D)
            j -= 1
        elif j == 0:
            ops.append(OP_I)
            i -= 1
        else:
            same = qc[i - 1] == sc[j - 1]
            if d[i - 1][j - 1] + (0 if same else 1) == d[i][j]:
                ops.append(OP_EQ if same else OP_X)
                i -= 1
                j -= 1
            elif d[i - 1][j] + 1 == d[i][j]:
                ops.append(OP_I)
                i -= 1
            else:
                ops.append(OP_D)
                j -= 1
    ops.reverse()
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return d[-1][-1], [(length, op) for length, op in runs]


def canonical(queries: np.ndarray, subjects: np.ndarray):
    """Per pair p = (queries[p], subjects[p]): a list of (distance, runs)."""
    d = dp_matrices(queries, subjects)
    qc, sc = classes(queries), classes(subjects)
    return [traceback(d[p], qc[p], sc[p]) for p in range(qc.shape[0])]


def pack(runs) -> np.ndarray:
    return np.array([(length << 4) | op for length, op in runs], dtype=np.uint32)


def unpack(words) -> list:
    return [(int(w) >> 4, int(w) & 15) for w in np.asarray(words).astype(np.uint32)]


def validate(query: np.ndarray, subject: np.ndarray, distance: int, runs) -> None:
    """Asserts that `runs` is an edit script of `query` into `subject` with exactly `distance` edits."""
    qc, sc = classes(query), classes(subject)
    i = j = edits = 0
    last = None
    for length, op in runs:
        assert length >= 1 and op in OP_CHAR, (length, op)
        assert op != last, "adjacent runs carry the same op"
        last = op
        if op in (OP_EQ, OP_X):
            assert i + length <= qc.size and j + length <= sc.size, "the script runs past a sequence"
            same = qc[i: i + length] == sc[j: j + length]
            assert same.all() if op == OP_EQ else not same.any(), ("'=' over different or 'X' over equal classes", i, j)
            i += length
            j += length
        elif op == OP_I:
            i += length
        else:
            j += length
        if op != OP_EQ:
            edits += length
    assert (i, j) == (qc.size, sc.size), f"the script consumes {(i, j)}, the sequences hold {(qc.size, sc.size)}"
    assert edits == distance, f"X + I + D = {edits}, distance = {distance}"


def to_string(runs) -> str:
    return "".join(f"{length}{OP_CHAR[op]}" for length, op in runs)


def from_string(text: str) -> list:
    return [(int(n), CHAR_OP[c]) for n, c in re.findall(r"(\d+)([=XID])", text)]

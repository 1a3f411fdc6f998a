"""Python-integer restatement of the band-limited pair alignment (include/bgsa_hip.h "band-limited history") — a helper,
not a test.

The rule.  B = max_distance, delta = n - m, dlo = -((B - delta) // 2), dhi = (delta + B) // 2 (myers_band.h: band_schedule).
Rows run in blocks of 32; the block of 0-based rows i0 .. last - 1 (last = min(i0 + 32, m)) runs on the WINDOW of words
[a, b], a = (max(1, i0 + 1 + dlo) - 1) // 32, b = (min(n, last + dhi) - 1) // 32.  Every row of the block is the Myers row on
exactly these words: the lowest window word takes the row-edge carry-ins (hp_in = 1, hn_in = 0, add-carry 0), words left of
the window keep their last deltas, words right of it their initial state (pv = ~0, mv = 0).  D' = m + sum over ALL words of
popc(pv & mask) - popc(mv & mask); D' <= B certifies D' = D and the pair is traced back from (m, n) through the two history
vectors A = Eq | ~D0 and B = Eq | (D0 & Hp) kept for the window words only; otherwise the pair is beyond the bound.

The window's words are one Python integer here, so the inter-word carries are the integer's own.
"""
import align_reference as A

ROWS = 32   # rows per block
WORD = 32


class BandFault(AssertionError):
    """The traceback asked for a word outside its block's window (BGSA_HIP_FAULT_BAND on the device)."""


def block_windows(m: int, n: int, max_distance: int):
    """[(a, b)] per block of 32 rows, or [] when the shape has no band (non-positive lengths, B < 0, |delta| > B)."""
    B, delta = max_distance, n - m
    if m <= 0 or n <= 0 or B < 0 or abs(delta) > B:
        return []
    dlo, dhi = -((B - delta) // 2), (delta + B) // 2
    out = []
    for i0 in range(0, m, ROWS):
        last = min(i0 + ROWS, m)
        out.append(((max(1, i0 + 1 + dlo) - 1) // WORD, (min(n, last + dhi) - 1) // WORD))
    return out


def band_words(m: int, n: int, max_distance: int) -> int:
    return max((b - a + 1 for a, b in block_windows(m, n, max_distance)), default=0)


def align(qc, sc, max_distance: int):
    """(distance | None, runs, band_words) for one pair of class rows (align_reference.classes); None = beyond the bound.
    Raises BandFault if the traceback of a certified pair leaves its windows."""
    qc, sc = [int(c) for c in qc], [int(c) for c in sc]
    m, n = len(qc), len(sc)
    wins = block_windows(m, n, max_distance)
    if not wins:
        return None, [], 0
    word_num = (n + WORD - 1) // WORD
    peq = [0] * 5
    for j, c in enumerate(sc):
        peq[c] |= 1 << j
    pv, mv = (1 << (WORD * word_num)) - 1, 0
    hist = []
    for i in range(m):
        a, b = wins[i // ROWS]
        shift, width = WORD * a, WORD * (b - a + 1)
        mask = (1 << width) - 1
        e, x, mw = (peq[qc[i]] >> shift) & mask, (pv >> shift) & mask, (mv >> shift) & mask
        d0 = ((((x & e) + x) ^ x) | e | mw) & mask
        hp = (~(d0 | x) | mw) & mask
        hn = d0 & x
        hps, hns = ((hp << 1) | 1) & mask, (hn << 1) & mask
        keep = ~(mask << shift)
        pv = (pv & keep) | (((~(d0 | hps) | hns) & mask) << shift)
        mv = (mv & keep) | ((d0 & hps) << shift)
        hist.append(((e | ~d0) & mask, e | (d0 & hp)))
    cols = (1 << n) - 1
    dist = m + bin(pv & cols).count("1") - bin(mv & cols).count("1")
    width = max(b - a + 1 for a, b in wins)
    if dist > max_distance:
        return None, [], width
    i, j, ops = m, n, []
    while i > 0 or j > 0:
        if i == 0:
            ops.append(A.OP_D)
            j -= 1
        elif j == 0:
            ops.append(A.OP_I)
            i -= 1
        else:
            a, b = wins[(i - 1) // ROWS]
            w = (j - 1) // WORD
            if not a <= w <= b:
                raise BandFault(f"cell ({i}, {j}): word {w} outside the window [{a}, {b}]")
            bit = j - 1 - WORD * a
            diag, which = (hist[i - 1][0] >> bit) & 1, (hist[i - 1][1] >> bit) & 1
            if diag:
                ops.append(A.OP_EQ if which else A.OP_X)
                i -= 1
                j -= 1
            elif which:
                ops.append(A.OP_I)
                i -= 1
            else:
                ops.append(A.OP_D)
                j -= 1
    ops.reverse()
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return dist, [(length, op) for length, op in runs], width


def align_rows(queries, subjects, max_distance: int):
    """align() per pair p = (queries[p], subjects[p]) of ASCII rows."""
    qc, sc = A.classes(queries), A.classes(subjects)
    return [align(qc[p], sc[p], max_distance) for p in range(qc.shape[0])]

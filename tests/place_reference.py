"""Python-integer restatement of the band-limited semi-global placement (include/bgsa_hip.h "band-limited semi-global
placement") — a helper, not a test.

The mode is Myers unit-cost semi-global: the subject (n columns) end to end inside the query (m rows), D[0][j] = j and
D[i][0] = 0.

Locate (exact, whatever the bound).  The Myers row on all words with hp_in = 0 at the row edge; run = n at row 0 and moves by
Hp - Hn at column n per row; D* = the smallest run and e = the SMALLEST row that has it.

The bound.  B = min(max_distance, n).  A pair with D* > B is beyond the bound.

The band-limited rows of a pair within the bound run in VIRTUAL rows: o = e - n - B (may be negative), M' = n + B, virtual row
i' = 1 .. M' is query row i = i' + o.  The block of 0-based virtual rows i0 .. last - 1 (last = min(i0 + 32, M')) runs on the
WINDOW of words [a, b], a = (max(1, i0 + 1 - 2B) - 1) // 32, b = (min(n, last) - 1) // 32: the diagonals j - i' in [-2B, 0].
Every row of the block is the Myers row on exactly these words: the lowest window word takes hp_in = 0 when a == 0 (the free
column 0) and 1 otherwise, hn_in and the add-carry 0; words left of the window keep their last deltas, words right of it their
initial state (pv = ~0, mv = 0).  A virtual row whose query row does not exist (i < 1) runs with an all-zero match mask.
D' = (rows run with hp_in = 1) + sum over ALL words of popc(pv & mask) - popc(mv & mask) >= D*; it must equal D*.  The walk back
starts at (e, n) — virtual row M' — through A = Eq | ~D0 and B = Eq | (D0 & Hp) kept for the window words only, diagonal first,
then up 'I', then left 'D', stops at the first cell with j = 0 (its row is q_begin) and on query row 0 emits 'D' for what is left.

The window's words are one Python integer here, so the inter-word carries are the integer's own.
"""
import align_reference as A

ROWS = 32   # virtual rows per block
WORD = 32


class BandFault(AssertionError):
    """The traceback asked for a cell outside its block's window, or D' != D* (BGSA_HIP_FAULT_BAND on the device)."""


def bound_of(n: int, max_distance: int) -> int:
    return min(max_distance, n)


def block_windows(n: int, max_distance: int):
    """[(a, b)] per block of 32 virtual rows; [] for a non-positive length or a negative bound.  Depends on (n, B) only."""
    if n <= 0 or max_distance < 0:
        return []
    B = bound_of(n, max_distance)
    rows = n + B
    out = []
    for i0 in range(0, rows, ROWS):
        last = min(i0 + ROWS, rows)
        out.append(((max(1, i0 + 1 - 2 * B) - 1) // WORD, (min(n, last) - 1) // WORD))
    return out


def band_words(n: int, max_distance: int) -> int:
    return max((b - a + 1 for a, b in block_windows(n, max_distance)), default=0)


def peq_of(sc):
    peq = [0] * 5
    for j, c in enumerate(sc):
        peq[c] |= 1 << j
    return peq


def locate(qc, sc):
    """(D*, e): the best cell of the last column, the smallest such row."""
    n = len(sc)
    peq = peq_of(sc)
    mask = (1 << n) - 1
    top = 1 << (n - 1)
    pv, mv = mask, 0
    run = best = n
    e = 0
    for i, c in enumerate(qc, start=1):
        eq = peq[c]
        d0 = ((((pv & eq) + pv) ^ pv) | eq | mv) & mask
        hp = (~(d0 | pv) | mv) & mask
        hn = d0 & pv
        run += (1 if hp & top else 0) - (1 if hn & top else 0)
        hps, hns = (hp << 1) & mask, (hn << 1) & mask    # hp_in = 0: the free column 0
        pv = (~(d0 | hps) | hns) & mask
        mv = d0 & hps
        if run < best:
            best, e = run, i
    return best, e


def place(qc, sc, max_distance: int):
    """(D*, e, q_begin | None, runs, band_words) for one pair of class rows (align_reference.classes); q_begin None = beyond
    the bound.  Raises BandFault if D' != D* or the traceback of a pair within the bound leaves its windows."""
    qc, sc = [int(c) for c in qc], [int(c) for c in sc]
    m, n = len(qc), len(sc)
    assert m > 0 and n > 0 and max_distance >= 0
    dstar, e = locate(qc, sc)
    B = bound_of(n, max_distance)
    wins = block_windows(n, max_distance)
    width = max(b - a + 1 for a, b in wins)
    if dstar > B:
        return dstar, e, None, [], width
    o, rows = e - n - B, n + B
    word_num = (n + WORD - 1) // WORD
    peq = peq_of(sc)
    pv, mv = (1 << (WORD * word_num)) - 1, 0
    hist = []
    edge_rows = 0
    for iv in range(rows):                     # 0-based virtual row; the query row is iv + 1 + o
        a, b = wins[iv // ROWS]
        shift, wbits = WORD * a, WORD * (b - a + 1)
        mask = (1 << wbits) - 1
        i = iv + 1 + o
        assert i <= m
        eq = (peq[qc[i - 1]] >> shift) & mask if i >= 1 else 0
        if i < 1 and a != 0:
            raise BandFault(f"virtual row {iv + 1}: no query row, yet the window starts at word {a}")
        hp_in = 0 if a == 0 else 1
        edge_rows += hp_in
        x, mw = (pv >> shift) & mask, (mv >> shift) & mask
        d0 = ((((x & eq) + x) ^ x) | eq | mw) & mask
        hp = (~(d0 | x) | mw) & mask
        hn = d0 & x
        hps, hns = ((hp << 1) | hp_in) & mask, (hn << 1) & mask
        keep = ~(mask << shift)
        pv = (pv & keep) | (((~(d0 | hps) | hns) & mask) << shift)
        mv = (mv & keep) | ((d0 & hps) << shift)
        hist.append(((eq | ~d0) & mask, eq | (d0 & hp)))
    cols = (1 << n) - 1
    certified = edge_rows + bin(pv & cols).count("1") - bin(mv & cols).count("1")
    if certified != dstar:
        raise BandFault(f"D' = {certified}, D* = {dstar} at B = {B}")
    iv, j, ops = rows, n, []                   # 1-based virtual row
    while j > 0:
        i = iv + o
        if i == 0:
            ops.append(A.OP_D)
            j -= 1
            continue
        if iv < 1:
            raise BandFault(f"cell ({i}, {j}): above the first virtual row")
        a, b = wins[(iv - 1) // ROWS]
        w = (j - 1) // WORD
        if not a <= w <= b:
            raise BandFault(f"cell ({i}, {j}): word {w} outside the window [{a}, {b}]")
        bit = j - 1 - WORD * a
        diag, which = (hist[iv - 1][0] >> bit) & 1, (hist[iv - 1][1] >> bit) & 1
        if diag:
            ops.append(A.OP_EQ if which else A.OP_X)
            iv -= 1
            j -= 1
        elif which:
            ops.append(A.OP_I)
            iv -= 1
        else:
            ops.append(A.OP_D)
            j -= 1
    q_begin = iv + o
    ops.reverse()
    runs = []
    for op in ops:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return dstar, e, q_begin, [(length, op) for length, op in runs], width


def place_rows(queries, subjects, max_distance: int):
    """place() per pair p = (queries[p], subjects[p]) of ASCII rows."""
    qc, sc = A.classes(queries), A.classes(subjects)
    return [place(qc[p], sc[p], max_distance) for p in range(qc.shape[0])]

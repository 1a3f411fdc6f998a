#!/usr/bin/env python3
"""Early-leave cut rows of the Myers rescue band (myers_band.h: kBandEarlyCuts, DESIGN §4.2, LABNOTES §37).

For every default rescue length (band_rescue_lengths, n = m) the full DP of random uniform ACGT pairs, on the CPU, and
for every low word w of the window the earliest row r behind which the word may leave under the per-lane bound

    limit = min(B, M),  M = D[r][j_r] + (r - j_r),  j_r = 32 (w + 1)

so that at most --rate of the lanes that B certifies fall above M.  M is taken from the true D, which is conservative:
the banded D' is never smaller.  At most two words leave early (myers_band.h: kBandMaxCuts, what the kernel's argument
word holds), the two that save the most word-rows; a length whose cuts save less than --min-gain of the band's
word-rows, or whose uncertified rate with the cuts reaches --pool-rate, gets none.

    python scripts/band_early_cuts.py > profiles/r12_band_early_cuts.txt

prints the report and, at its end, the table rows as myers_band.h holds them.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bgsa_amd", "csrc"))
import rows_ir as R  # noqa: E402


def rescue_lengths():
    """myers_band.h: band_rescue_lengths for n = m."""
    return [n for n in range(65, 161) if (9 * n + 192) % 32 < 8]


def dp_columns(q: np.ndarray, s: np.ndarray, cols):
    """Full edit-distance DP of the pairs (q[k], s[k]), row by row: returns D[m][n] and, for every column j of `cols`,
    D[i][j] for i = 0..m as an array [pairs, m + 1]."""
    n_pairs, m = q.shape
    n = s.shape[1]
    J = np.arange(n + 1, dtype=np.int16)
    prev = np.broadcast_to(J, (n_pairs, n + 1)).copy()
    keep = {j: np.empty((n_pairs, m + 1), dtype=np.int16) for j in cols}
    for j in cols:
        keep[j][:, 0] = j
    t = np.empty_like(prev)
    for i in range(1, m + 1):
        t[:, 0] = i
        np.minimum(prev[:, 1:] + 1, prev[:, :-1] + (q[:, i - 1, None] != s), out=t[:, 1:])
        t -= J                                   # D[i][j] - j = min over k <= j of (t[k] - k)
        np.minimum.accumulate(t, axis=1, out=t)
        t += J
        prev, t = t, prev
        for j in cols:
            keep[j][:, i] = prev[:, j]
    return prev[:, n].copy(), keep


def length_cuts(n: int, pairs: int, chunk: int, rate: float, pool_rate: float, min_gain: float, rng, out):
    h = R.myers_band_rescue_half(n)
    B, nw = 2 * h + 1, (n + 31) // 32
    win = R.myers_band_windows(n, n, h, nw)
    if win is None:
        print(f"{n:4d} bp  h {h}  no band", file=out)
        return []
    total = sum(b - a + 1 for a, b in win)
    # the static rule keeps word w through row 32 (w + 1) + h
    words = [w for w in range(nw - 1) if 32 * (w + 1) + h < n]
    cols = [32 * (w + 1) for w in words]
    over_b = 0
    fails = {w: np.zeros(n + 1, dtype=np.int64) for w in words}      # [r]: lanes with D <= B < ... and D > M(r, w)
    fail_sets = []
    for start in range(0, pairs, chunk):
        k = min(chunk, pairs - start)
        q = rng.integers(0, 4, size=(k, n), dtype=np.uint8)
        s = rng.integers(0, 4, size=(k, n), dtype=np.uint8)
        d, keep = dp_columns(q, s, cols)
        over_b += int((d > B).sum())
        ok = d <= B
        rows = np.arange(n + 1, dtype=np.int32)
        per = {}
        for w, j in zip(words, cols):
            M = keep[j].astype(np.int32) + rows - j
            bad = ok[:, None] & (d[:, None] > M)
            bad[:, :j] = False
            fails[w] += bad.sum(axis=0)
            per[w] = bad
        fail_sets.append(per)
    cand = []
    for w in words:
        static = 32 * (w + 1) + h
        r = static
        while r - 1 >= 32 * (w + 1) and fails[w][r - 1] <= rate * pairs:
            r -= 1
        if r < static:
            cand.append((static - r, r, w))
        print(f"{n:4d} bp  word {w}: static leave after row {static}, early after row {r} "
              f"(adds {fails[w][r] / pairs:.2e}; one row earlier {fails[w][r - 1] / pairs:.2e})", file=out)
    cand = sorted(sorted(cand, reverse=True)[:2], key=lambda c: c[1])
    saved = sum(c[0] for c in cand)
    union = sum(int(np.logical_or.reduce([per[w][:, r] for _, r, w in cand]).sum()) for per in fail_sets) if cand else 0
    after = (over_b + union) / pairs
    take = bool(cand) and saved >= min_gain * total and after < pool_rate
    print(f"{n:4d} bp  h {h}  B {B}  word-rows {total} -> {total - saved} ({100.0 * saved / total:.2f} %)  "
          f"above B {over_b / pairs:.2e}  added by the cuts {union / pairs:.2e}  uncertified {after:.2e}  "
          f"{'TAKEN' if take else 'none'}", file=out)
    out.flush()
    return [(r, w) for _, r, w in cand] if take else []


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--pairs", type=int, default=200000)
    ap.add_argument("--chunk", type=int, default=20000)
    ap.add_argument("--rate", type=float, default=5e-5, help="lanes one cut may add to the rescue")
    ap.add_argument("--pool-rate", type=float, default=2e-3, help="the uncertified rate the pool is sized for")
    ap.add_argument("--min-gain", type=float, default=0.02, help="fewest word-rows saved, of the band's")
    ap.add_argument("--seed", type=int, default=12)
    ap.add_argument("--lengths", type=str, default="", help="comma-separated; default: every default rescue length")
    a = ap.parse_args()
    lengths = [int(x) for x in a.lengths.split(",")] if a.lengths else rescue_lengths()
    table = []
    for n in lengths:
        rng = np.random.default_rng([a.seed, n])
        cuts = length_cuts(n, a.pairs, a.chunk, a.rate, a.pool_rate, a.min_gain, rng, sys.stdout)
        if cuts:
            table.append((n, cuts))
    print(f"\n// kBandEarlyCuts: {a.pairs} pairs per length, seed {a.seed}, rate {a.rate:g}")
    for n, cuts in table:
        cuts = cuts + [(0, 0)] * (2 - len(cuts))
        print(f"    {{{n}, {len([c for c in cuts if c[0]])}, {{{cuts[0][0]}, {cuts[1][0]}}}, {{{cuts[0][1]}, {cuts[1][1]}}}}},")


if __name__ == "__main__":
    main()

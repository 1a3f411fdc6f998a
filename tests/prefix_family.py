"""The query family of the prefix-sharing tests (test_myers_prefix_cpu.py, test_myers_prefix_gpu.py) and the sorted order a
sharing launch computes for it on the device."""
import numpy as np

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

KEY_CHARS = 10      # myers_band.h: kPrefixKeyChars


def _differ(rng, a, at):
    """A copy of `a` that differs from it at position `at` (and is random behind it)."""
    b = a.copy()
    b[at] = ACGT[(int(np.searchsorted(ACGT, a[at])) + 1 + int(rng.integers(3))) % 4]
    b[at + 1:] = ACGT[rng.integers(0, 4, len(a) - at - 1)]
    return b


def family(m, seed=7):
    """About 60 queries of length m: pairs with common prefixes of every length 0..10, one pair sharing exactly 16, one sharing
    more than the first window's rows, two exact duplicates, and X, Y, Z with lcp(X, Y) = 7 > lcp(Y, Z) = 5 — Z resumes at depth 5
    from a slot that X wrote and Y skipped, which a single snapshot (Y's, at depth 7 or none) would get wrong."""
    rng = np.random.default_rng(seed + m)
    fresh = lambda: ACGT[rng.integers(0, 4, m)]
    out = []
    for lcp in range(0, 11):
        a = fresh()
        out += [a, _differ(rng, a, lcp)]
    a = fresh()
    out += [a, _differ(rng, a, 16)]
    a = fresh()
    out += [a, _differ(rng, a, min(40, m - 2))]
    a = fresh()
    out += [a, a.copy()]
    x = fresh()
    x[:8] = np.frombuffer(b"CCCCCAAA", dtype=np.uint8)
    y = _differ(rng, x, 7)
    z = x.copy()
    z[5] = ord("T")                                 # sorts behind X and Y: A < T at position 5
    z[6:] = ACGT[rng.integers(0, 4, m - 6)]
    out += [x, y, z]
    while len(out) < 60:                            # and some that share by chance with the above
        out.append(_differ(rng, out[int(rng.integers(len(out)))], int(rng.integers(0, 9))))
    q = np.stack(out)
    return q[rng.permutation(len(q))]


def sorted_order(q, depths, tile):
    """(order, lcp) as the launch computes them on the device: by the first 10 class codes, then by query number; lcp capped at the
    deepest depth and 0 at every tile start."""
    codes = CODE[q[:, :KEY_CHARS]].astype(np.int64)
    key = np.zeros(len(q), dtype=np.int64)
    for j in range(KEY_CHARS):
        key = key * 8 + (codes[:, j] if j < codes.shape[1] else 0)
    order = np.lexsort((np.arange(len(q)), key))
    lcp = []
    for k, i in enumerate(order):
        if k % tile == 0:
            lcp.append(0)
            continue
        same = codes[i] == codes[order[k - 1]]
        n = int(np.argmin(same)) if not same.all() else KEY_CHARS
        lcp.append(min(n, depths[-1]))
    return order, lcp

"""Band-edge pairs for the certified diagonal band of the Myers global kernels — TEST INFRASTRUCTURE ONLY.

Random reads and lightly mutated copies keep their optimal paths near the main diagonal and their distances far below
B = 2h + 1, so they never touch the outer word of a row's window, the row at which a window gains or loses a word, or the
comparison with B.  The pairs made here do: a low-entropy query q over A C T and subjects that are q shifted by t columns
behind (or by u rows above) a run of a filler character that q does not hold,

    insert-first  s = G^t + q[:n - t]         t insertions, diagonal d = t, then t - delta deletions: 2t - delta edits
    delete-first  s = q[u:] + G^(n - m + u)   u deletions, diagonal d = -u, then the filler:          2u + delta edits

each also with one substitution in the middle of the copied part (the other parity).  The figures are what the construction
intends; the distance of a pair is whatever oracle.dp_edit says.  The band's diagonals are dlo .. dhi as in
myers_band.h: band_schedule, so the full ladders t = max(delta, 0) .. dhi, u = max(-delta, 0) .. -dlo put a path on every
diagonal of the band, and the rungs with |intended - B| <= near straddle the certificate.
"""
from __future__ import annotations

import numpy as np

FILLER = ord("G")


def band_limits(m: int, n: int, h: int):
    """(B, dlo, dhi) of an m-row query against n-column subjects at half-width h (myers_band.h: band_schedule)."""
    B = 2 * h + 1
    delta = n - m
    return B, -((B - delta) // 2), (delta + B) // 2


def three_run_query(m: int) -> np.ndarray:
    """A^a C^a T^(m - 2a), a = m // 3."""
    a = m // 3
    return np.frombuffer(b"A" * a + b"C" * a + b"T" * (m - 2 * a), dtype=np.uint8).copy()


def seeded_runs_query(m: int, seed: int, longest: int | None = None) -> np.ndarray:
    """Runs of random lengths in [longest / 2, longest] over A C T, adjacent runs differ; longest defaults to m // 3."""
    longest = m // 3 if longest is None else longest
    rng = np.random.default_rng(seed)
    out: list[int] = []
    prev = -1
    while len(out) < m:
        c = int(rng.integers(0, 3))
        if c == prev:
            continue
        prev = c
        out += [b"ACT"[c]] * int(rng.integers(max(1, longest // 2), longest + 1))
    return np.array(out[:m], dtype=np.uint8)


def _rung(q: np.ndarray, n: int, kind: str, k: int, sub: int) -> np.ndarray | None:
    m = len(q)
    if kind == "ins":
        keep = n - k
        if keep < 1 or keep > m:
            return None
        s = np.concatenate([np.full(k, FILLER, np.uint8), q[:keep]])
        if sub:
            s[k + keep // 2] = FILLER
    else:
        keep, tail = m - k, n - (m - k)
        if keep < 1 or tail < 0:
            return None
        s = np.concatenate([q[k:], np.full(tail, FILLER, np.uint8)])
        if sub:
            s[keep // 2] = FILLER
    return s


def band_edge_pairs(q: np.ndarray, n: int, h: int, full: bool = True, near: int = 3):
    """Subjects of length n against query q at half-width h: the full ladders (full=True) and the rungs whose intended
    distance lies within `near` of B.  Returns (subjects [k, n] uint8, tags [(kind, shift, sub, intended)]) without
    duplicate rows."""
    q = np.asarray(q, dtype=np.uint8)
    m = len(q)
    assert FILLER not in q
    B, dlo, dhi = band_limits(m, n, h)
    delta = n - m
    rows, tags, seen = [], [], set()
    for kind, first, last, intended in (("ins", max(delta, 0), dhi, lambda t: 2 * t - delta),
                                        ("del", max(-delta, 0), -dlo, lambda u: 2 * u + delta)):
        for k in range(first, max(m, n) + 1):
            d = intended(k)
            if d > B + near:
                break
            close = abs(d - B) <= near
            if not (close or (full and k <= last)):
                continue
            for sub in (0, 1):
                s = _rung(q, n, kind, k, sub)
                if s is None or s.tobytes() in seen:
                    continue
                seen.add(s.tobytes())
                rows.append(s)
                tags.append((kind, k, sub, d + sub))
    return np.stack(rows), tags


def band_edge_two_waves(q: np.ndarray, n: int, h: int, dist, mutate, gen_reads, seed: int, groups: int = 1, lane: int = 0,
                        group: int = 0, near: int = 4):
    """Two waves of `groups` x 64 subjects for one query (groups = 2: the waves of a kernel that carries two subject groups):
      * one in which every lane is within B of q: the near-B rungs with D = B - 1 and D = B and the rungs on the band's
        outermost diagonals dlo and dhi that lie within B, dealt over the groups at lanes 0, 5, 10, ..., among copies of q
        carrying 0 .. 20 random edits (fewer where |n - m| leaves less room below B);
      * one with exactly one lane above B — at `lane` of `group`, the rung with the smallest D > B the ladders hold — and a
        rung with the largest D <= B beside it, among such copies.
    dist / mutate / gen_reads as for band_edge_waves.  Returns (subjects [128 groups, n], distances of the rungs placed in the
    first wave, distance of the one lane above B)."""
    q = np.asarray(q, dtype=np.uint8)
    m = len(q)
    assert groups in (1, 2) and 0 <= lane < 64 and 0 <= group < groups
    B, dlo, dhi = band_limits(m, n, h)
    s, _ = band_edge_pairs(q, n, h, full=False, near=near)
    outer = [r for kind, k in (("ins", dhi), ("del", -dlo)) for sub in (0, 1) if (r := _rung(q, n, kind, k, sub)) is not None]
    have = {r.tobytes() for r in s}
    fresh = [r for r in outer if r.tobytes() not in have]
    if fresh:
        s = np.concatenate([s, np.stack(fresh)])
    D = dist(q[None], s)[0]
    assert (D > B).any() and (D <= B).any(), "the ladders stay on one side of B"
    on_edge = np.array([r.tobytes() in {o.tobytes() for o in outer} for r in s])
    first = np.flatnonzero(((D >= B - 1) | on_edge) & (D <= B))
    assert len(first) <= 13 * groups
    above = s[np.flatnonzero(D == D[D > B].min())[0]]
    below = s[np.flatnonzero(D == D[D <= B].max())[0]]
    size = 64 * groups
    k = min(m, n)
    # 32 copies, cycled over the lanes; an indel of mutate() costs two edits, so the copies stay within B whatever n - m is
    most = min(20, (B - abs(n - m)) // 2)
    pool = gen_reads(seed, 32, n)
    pool[:, :k] = mutate(np.repeat(q[None, :k], 32, axis=0), np.arange(32) % (most + 1), seed)
    out = np.resize(pool, (2 * size, n))
    for i, r in enumerate(first):
        out[64 * (i % groups) + (5 * (i // groups)) % 64] = s[r]
    out[size + 64 * group + (lane + 1) % 64] = below
    out[size + 64 * group + lane] = above
    return np.ascontiguousarray(out), D[first], int(D[D > B].min())


def band_edge_waves(q: np.ndarray, n: int, h: int, dist, mutate, gen_reads, seed: int, inside_waves: int = 0):
    """Whole waves of 64 subjects for one query, so that a GPU run observes the banded result and not the redo:
      * waves in which every lane is within B of q: the full ladders and the near-B rungs with D <= B (one with D = B),
        filled up with copies of q carrying 0 .. 20 random edits;
      * four waves with exactly one lane above B, at lane 0, 31, 32 and 63: a rung with D = B + 1 among 63 lanes with D <= B,
        one of them a rung with D = B.
    dist(q[None], s)[0] is the distance (oracle.dp_edit, negated); mutate / gen_reads as in the oracle package; inside_waves:
    at least so many waves of the first kind.  Returns (subjects [64 w, n], number of waves of the first kind); the four
    waves of the second kind come last, in the order of their lanes."""
    q = np.asarray(q, dtype=np.uint8)
    m = len(q)
    B = 2 * h + 1
    s, _ = band_edge_pairs(q, n, h)
    D = dist(q[None], s)[0]
    inside, at_b, above = s[D <= B], s[D == B], s[D == B + 1]
    assert len(at_b) and len(above), "the ladders hold no pair at B or at B + 1"
    fill = max((-len(inside)) % 64, 64 * inside_waves - len(inside))
    if fill:
        k = min(m, n)
        extra = gen_reads(seed, fill, n)
        extra[:, :k] = mutate(np.repeat(q[None, :k], fill, axis=0), np.arange(fill) % 21, seed)
        assert (dist(q[None], extra)[0] <= B).all()
        inside = np.concatenate([inside, extra])
    waves = [inside]
    for i, lane in enumerate((0, 31, 32, 63)):
        rest = np.concatenate([at_b[i % len(at_b)][None], np.roll(inside, -61 * i, axis=0)[:62]])
        waves.append(np.insert(rest, lane, above[i % len(above)], axis=0))
    return np.ascontiguousarray(np.concatenate(waves)), len(inside) // 64

"""The inputs of the early-leave GPU test (test_myers_band_early_gpu.py) and what the host model says of them.

One query q0 over A C T per length and 192 subjects — three groups of 64, the second wave of a two-group kernel has one live
group — from four families: random reads, copies of q0 with 0 .. 5 edits, the band-edge ladders of oracle/band_edge.py (the
rungs near B and a spread of the others, both kinds), and the rotations q0[k:] + q0[:k].  The queries are q0 with 0 .. 5
substitutions behind its first rows, so sorted neighbours share at least ten rows.  The host model (rows_ir.run_band_early)
gives every lane's D' and limit; the lanes above their limit are spread so that no group holds more than eight for any query —
except in the "nine" bucket, whose third group holds nine for query 0.
"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import oracle as O  # noqa: E402
from oracle import band_edge as E  # noqa: E402

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v
ACT = np.frombuffer(b"ACT", dtype=np.uint8)
LENGTHS = (150, 100, 68)            # five words, and the shortest four- and three-word lengths with cuts
N_DISTINCT = 6                      # queries i and i + 6 are equal: the model runs once per distinct query
PLACES = (0, 31, 32, 63, 17)        # lanes of a group that hold its lanes above their limit (at most five by q0)


def model(q, s, h, cuts):
    """(D', limit) per lane of one query against subjects s."""
    n, nw = len(q), (len(q) + 31) // 32
    score, limit, _ = R.run_band_early(nw, R.build_peq32(s, nw), CODE[q], n, h, cuts)
    return score[0], limit[0]


def queries(q0, count):
    n = len(q0)
    q = np.repeat(q0[None], count, axis=0)
    step = {ord("A"): ord("C"), ord("C"): ord("T"), ord("T"): ord("A")}
    for i in range(count):
        for j in range(i % N_DISTINCT):
            at = 12 + ((7 * (i % N_DISTINCT) + 11 * j) % (n - 14))
            q[i, at] = step[int(q[i, at])]
    return np.ascontiguousarray(q)


def build(n):
    """-> dict: q [24, n], base / nine [192, n], h, cuts, and per bucket the DP's D [6, 192] and the model's over-limit flags."""
    h = R.myers_band_rescue_half(n)
    cuts = R.myers_band_early_cuts(n, h)
    limit_b = 2 * h + 1
    rng = np.random.default_rng(1000 + n)
    q0 = rng.choice(ACT, n)
    ks = list(range(30, 46)) if n == 150 else list(range(h - 15, h + 1))
    rot = np.stack([np.concatenate([q0[k:], q0[:k]]) for k in ks])
    rungs, _ = E.band_edge_pairs(q0, n, h, near=8)
    rand = O.gen_reads(500 + n, 256, n)
    near = O.mutate(np.repeat(q0[None], 48, axis=0), np.arange(48) % 6, 77 + n)
    pool = np.concatenate([rot, rungs, rand, near])
    got, limit = model(q0, pool, h, cuts)
    want = -O.dp_edit(q0[None], pool).astype(np.int64)[0]
    over = np.flatnonzero(got > limit)
    cut_only = [i for i in over if want[i] <= limit_b]              # certified by B, above their own limit
    above_b = [i for i in over if want[i] > limit_b]
    calm = [i for i in np.flatnonzero(got <= limit)]
    rich = len(cut_only) >= 9           # (68 bp has one cut and few pairs that only it turns away)
    assert len(cut_only) >= 5 and len(above_b) >= (8 if rich else 10) and len(calm) >= 192, (n, len(cut_only), len(above_b), len(calm))
    # every family among the calm lanes, in turns
    order = sorted(calm, key=lambda i: (i % 4, i))

    def bucket(counts):
        """counts[g] = (lanes above their limit though D <= B, lanes with D > B) of group g"""
        s = np.empty((192, n), dtype=np.uint8)
        fill, c, a = iter(order), iter(cut_only), iter(above_b)
        for g, (n_cut, n_above) in enumerate(counts):
            hot = [next(c) for _ in range(n_cut)] + [next(a) for _ in range(n_above)]
            lanes = list(PLACES[:len(hot)]) + [3 * j + 1 for j in range(len(hot) - len(PLACES))]
            assert len(set(lanes)) == len(hot)
            for lane in range(64):
                s[64 * g + lane] = pool[hot[lanes.index(lane)]] if lane in lanes else pool[next(fill)]
        return np.ascontiguousarray(s)

    out = {"n": n, "h": h, "cuts": cuts, "q": queries(q0, 24),
           "base": bucket([(3, 2), (2, 3), (3, 1)] if rich else [(2, 2), (1, 3), (2, 1)]),
           "nine": bucket([(2, 2), (2, 2), (5, 4)] if rich else [(1, 2), (1, 2), (3, 6)])}
    for name in ("base", "nine"):
        qs = out["q"][:N_DISTINCT]
        out[name + "_want"] = -O.dp_edit(qs, out[name]).astype(np.int64)
        flags = []
        for q in qs:
            got, limit = model(q, out[name], h, cuts)
            w = out[name + "_want"][len(flags)]
            assert (got >= w).all() and np.array_equal(got[got <= limit], w[got <= limit])
            flags.append(got > limit)
        out[name + "_over"] = np.stack(flags)                   # [6, 192]
    return out

"""numpy / Python restatement of "paired reads" (include/bgsa_hip.h) — a helper, not a test.

The region, the rescue windows, R, the union and selection, the `rescued` flag and the pairing rule, each stated again from the
header's text on plain Python integers, and map_pairs_host: the whole of bgsa_amd.reference.ReferenceMapper.map_pairs on the host.
Nothing here calls the library.  Windows, ids, strands and keep are those of tests/reference_map_reference.py; stage A is its
map_reads_host blanked with seed_map_reference.blank, stage B seed_map_reference's window_distances and select, the placement
place_reference.place and reference_map_reference.placements.
"""
import numpy as np

import place_reference as P
import reference_map_reference as M
import seed_map_reference as S
from align_reference import classes

INT32_MIN = -2 ** 31
FIELDS = ("scores", "windows", "strand", "ref_begin", "ref_end", "keep")
OUTPUTS = ("proper", "slot1", "slot2", "insert", "cost", "n_best", "next_cost")


# ---- stage B: region, rescue windows, R -------------------------------------------------------------------------------------
def region(strand: int, begin: int, end: int, insert_max: int, L: int):
    """[lo, hi) in which the mate of an anchor on `strand` with interval [begin, end) lies."""
    return (begin, min(L, begin + insert_max)) if strand == 0 else (max(0, end - insert_max), end)


def rescue_windows(L: int, W: int, St: int, strand: int, begin: int, end: int, insert_max: int) -> list:
    """The ids, on the mate's strand, of every forward window that meets the anchor's region — by looking at every window."""
    lo, hi = region(strand, begin, end, insert_max, L)
    n = M.window_count(L, W, St)
    return [(1 - strand) * n + w for w in range(n) if M.window_start(L, W, St, w) < hi and M.window_start(L, W, St, w) + W > lo]


def rescue_slots(L: int, W: int, St: int, insert_max: int) -> int:
    return min(M.window_count(L, W, St), -(-(insert_max + W - 1) // St) + 1)


def anchors_of(strand, begin, end, keep, k_anchor: int) -> list:
    """[(strand, begin, end)] of one list: its first k_anchor kept slots, in list order."""
    return [(int(strand[r]), int(begin[r]), int(end[r])) for r in np.flatnonzero(np.asarray(keep))[:k_anchor]]


def rescue_table(L: int, W: int, St: int, strand, begin, end, keep, k_anchor: int, insert_max: int) -> np.ndarray:
    """What bgsa_hip_pair_rescue_windows_dev writes for the anchor lists [n_pairs, k]: int32[n_pairs, k_anchor * R]."""
    R = rescue_slots(L, W, St, insert_max)
    out = np.full((len(keep), k_anchor * R), -1, dtype=np.int32)
    for c in range(len(keep)):
        for a, (s, b, e) in enumerate(anchors_of(strand[c], begin[c], end[c], keep[c], k_anchor)):
            if s in (0, 1) and 0 <= b <= e <= L:
                ids = rescue_windows(L, W, St, s, b, e, insert_max)
                assert len(ids) <= R
                out[c, a * R: a * R + len(ids)] = ids
    return out


def union(own_windows, anchors, L: int, W: int, St: int, insert_max: int) -> list:
    """An end's own window ids and the rescue windows of all its anchors, each id once, ascending."""
    ids = {int(g) for g in own_windows if g >= 0}
    for s, b, e in anchors:
        ids.update(rescue_windows(L, W, St, s, b, e, insert_max))
    return sorted(ids)


def rescued_of(final_windows, own_windows) -> np.ndarray:
    own = {int(g) for g in own_windows if g >= 0}
    return np.array([g >= 0 and int(g) not in own for g in final_windows], dtype=bool)


# ---- stage C: the pairing rule ----------------------------------------------------------------------------------------------
def proper_insert(slot1, slot2, insert_min: int, insert_max: int):
    """slot = (strand, begin, end).  The insert of a proper combination, or None."""
    if slot1[0] == slot2[0]:
        return None
    fwd, rev = (slot1, slot2) if slot1[0] == 0 else (slot2, slot1)
    insert = rev[2] - fwd[1]
    return insert if fwd[1] <= rev[1] and fwd[2] <= rev[2] and insert_min <= insert <= insert_max else None


def live_slots(end) -> list:
    """[(r, strand, begin, end, distance)] of the slots of one list (a dict of this module's FIELDS, one row) that take part."""
    return [(r, int(end["strand"][r]), int(end["ref_begin"][r]), int(end["ref_end"][r]), -int(end["scores"][r]))
            for r in range(len(end["keep"]))
            if end["keep"][r] and end["strand"][r] in (0, 1) and end["ref_begin"][r] >= 0 and -(2 ** 30 - 1) <= end["scores"][r] <= 0]


def choose(end1, end2, insert_min: int, insert_max: int) -> dict:
    """The seven outputs of stage C for one pair."""
    one, two = live_slots(end1), live_slots(end2)
    best, costs = None, []
    for r1, s1, b1, e1, d1 in one:
        for r2, s2, b2, e2, d2 in two:
            insert = proper_insert((s1, b1, e1), (s2, b2, e2), insert_min, insert_max)
            if insert is None:
                continue
            costs.append(d1 + d2)
            if best is None or (d1 + d2, r1, r2) < best[:3]:
                best = (d1 + d2, r1, r2, insert)
    if best is None:
        cost = (one[0][4] if one else 0) + (two[0][4] if two else 0)
        return dict(proper=0, slot1=one[0][0] if one else -1, slot2=two[0][0] if two else -1, insert=0, cost=cost, n_best=0, next_cost=-1)
    above = [c for c in costs if c > best[0]]
    return dict(proper=1, slot1=best[1], slot2=best[2], insert=best[3], cost=best[0], n_best=costs.count(best[0]),
                next_cost=min(above) if above else -1)


def choose_all(end1, end2, insert_min: int, insert_max: int) -> dict:
    """choose() for every row of two results (dicts of arrays [ns, k]); arrays of OUTPUTS."""
    rows = [choose({f: end1[f][c] for f in FIELDS}, {f: end2[f][c] for f in FIELDS}, insert_min, insert_max)
            for c in range(len(end1["keep"]))]
    return {name: np.array([row[name] for row in rows], dtype=np.int64 if name == "insert" else np.int32) for name in OUTPUTS}


# ---- the whole pipeline on the host -----------------------------------------------------------------------------------------
def place_lists(ref, W: int, St: int, reads, scores, ids, bound: int) -> dict:
    """The lists (scores, ids)[ns, k] placed within `bound` and turned into reference coordinates, as map_reads_host does."""
    ref = np.asarray(ref, dtype=np.uint8)
    L, (ns, n), k = ref.size, reads.shape, ids.shape[1]
    n_ids = 2 * M.window_count(L, W, St)
    qc, sc = M.window_rows(classes(ref), W, St, range(n_ids)), classes(reads)
    span = np.full((ns * k, 4), -1, dtype=np.int32)
    n_ops = np.zeros(ns * k, dtype=np.int32)
    runs_of = {}
    for c in range(ns):
        for r in range(k):
            g, p = int(ids[c, r]), c * k + r
            if g < 0:
                continue
            dist, e, q_begin, runs, _ = P.place(qc[g], sc[c], bound)
            assert dist == -scores[c, r]
            span[p] = (-1 if q_begin is None else q_begin, e, 0, n)
            n_ops[p] = len(runs)
            runs_of[p] = runs
    cap = max(1, int(n_ops.max(initial=0)))
    cigar = np.zeros((ns * k, cap), dtype=np.int64)
    for p, runs in runs_of.items():
        cigar[p, : len(runs)] = [length << 4 | op for length, op in runs]
    strand, begin, end, keep, cigar = M.placements(L, W, St, ids, span, n_ops, cigar, cap)
    cigars = [[M.runs_text([(int(w) >> 4, int(w) & 15) for w in cigar[c * k + r, : n_ops[c * k + r]]]) if keep[c, r] else None
               for r in range(k)] for c in range(ns)]
    return dict(scores=scores, windows=ids, strand=strand, ref_begin=begin, ref_end=end, keep=keep, cigars=cigars)


def map_pairs_host(reference, W: int, St: int, reads1, reads2, insert_min: int, insert_max: int, k_best: int = 1, max_distance: int = 0,
                   rescue_distance=None) -> dict:
    """dict(single=(H_1, H_2), end1, end2, rescued1, rescued2 and the arrays of OUTPUTS) as ReferenceMapper.map_pairs returns them;
    single holds the stage A lists."""
    ref = np.frombuffer(bytes(reference), dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else np.asarray(reference, np.uint8)
    reads = (np.asarray(reads1, dtype=np.uint8), np.asarray(reads2, dtype=np.uint8))
    rescue_distance = max_distance if rescue_distance is None else rescue_distance
    L, ns = ref.size, reads[0].shape[0]
    k_sel = min(64, k_best * (-(-W // St) + 1))
    k_pair = k_sel + k_best * rescue_slots(L, W, St, insert_max)
    assert reads[1].shape[0] == ns and 1 <= insert_min <= insert_max and rescue_distance >= max_distance and k_pair <= 64
    single = [S.blank(M.map_reads_host(ref, W, St, rows, k_best=k_best, max_distance=max_distance), min(max_distance, rows.shape[1]))
              for rows in reads]
    final, rescued = [], []
    for e, rows in enumerate(reads):
        own, mate = single[e], single[1 - e]
        bound = min(rescue_distance, rows.shape[1])
        scores = np.empty((ns, k_pair), dtype=np.int32)
        ids = np.empty((ns, k_pair), dtype=np.int32)
        for c in range(ns):
            anchors = anchors_of(mate["strand"][c], mate["ref_begin"][c], mate["ref_end"][c], mate["keep"][c], k_best)
            mine = union(own["windows"][c], anchors, L, W, St, insert_max)
            distances = S.window_distances(ref, W, St, rows[c])
            scores[c], ids[c] = S.select(mine, [distances[g] for g in mine], bound, k_pair)
        final.append(place_lists(ref, W, St, rows, scores, ids, bound))
        rescued.append(np.stack([rescued_of(ids[c], own["windows"][c]) for c in range(ns)]))
    out = dict(single=tuple(single), end1=final[0], end2=final[1], rescued1=rescued[0], rescued2=rescued[1])
    out.update(choose_all(final[0], final[1], insert_min, insert_max))
    return out

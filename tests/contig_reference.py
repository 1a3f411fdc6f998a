"""Host model of "a reference of several contigs" (include/bgsa_hip.h), in plain Python — a helper, not a test.

The layout; the clip as a walk over a hit's columns (clip_runs, clip_hit, clip_lists); the existing pipeline model on the padded
reference followed by that clip (map_reads_model, map_ragged_model, map_pairs_model: the windows, lists, placements and keep of
reference_map_reference, seed_map_reference and pair_reference); the contig form of a SAM line, built on sam_reference; and
contig_distance, a plain semi-global DP of a read against ONE contig that knows nothing of windows, padding or clipping.

The fixture (FIXTURE, contigs, crafted, crafted_unbounded, crafted_pairs) is the smallest shape at which every branch exists.
"""
from types import SimpleNamespace

import numpy as np

import pair_reference as PR
import place_reference as R
import query_hits_reference as Q
import reference_map_reference as M
import sam_reference as S
import seed_map_reference as SM
from align_reference import classes

INT32_MIN = -2 ** 31
REF_ONLY, READ_ONLY, EQUAL, DIFF = 1, 2, 7, 8
ACGT = np.frombuffer(b"ACGT", np.uint8)


# ---- the layout ----------------------------------------------------------------------------------------------------------------
def layout(lens, W: int, P=None) -> tuple:
    """(starts, total): start_0 = 0, start_{i+1} = start_i + len_i + P, total = start_{C-1} + len_{C-1}; P None: W."""
    P = W if P is None else P
    assert len(lens) >= 1 and min(lens) >= 1 and P >= W >= 1
    starts = [0]
    for n in lens[:-1]:
        starts.append(starts[-1] + n + P)
    return starts, starts[-1] + lens[-1]


def padded(sequences, W: int, P=None) -> bytes:
    """The one mapped reference: the contigs at their starts, 'N' between them and up to W where the whole is shorter."""
    starts, total = layout([len(s) for s in sequences], W, P)
    out = bytearray(b"N" * max(total, W))
    for at, seq in zip(starts, sequences):
        out[at: at + len(seq)] = seq
    return bytes(out)


# ---- the clip --------------------------------------------------------------------------------------------------------------------
def contig_of(starts, lens, L: int, begin: int, end: int):
    """The contig that holds the first non-padding base of [begin, end), or None.  An empty interval — a hit of read-only bases —
    belongs to the contig it lies in or at the edge of."""
    if not 0 <= begin <= end <= L:
        return None
    if begin == end:
        return next((c for c, (s, n) in enumerate(zip(starts, lens)) if s <= begin <= s + n), None)
    for c, (s, n) in enumerate(zip(starts, lens)):
        if s + n > begin:
            return c if s < end else None
    return None


def compress(columns) -> list:
    runs = []
    for op in columns:
        if runs and runs[-1][1] == op:
            runs[-1][0] += 1
        else:
            runs.append([1, op])
    return [(n, op) for n, op in runs]


def walk(columns: list, outside: int) -> tuple:
    """The first `outside` reference columns of a script, one op per column, leave the hit: a reference-only column is dropped
    (-1), an X column becomes a read-only base (0), an '=' column becomes a read-only base (+1); read-only columns on the way
    stay.  Returns (the new columns, the change of the distance)."""
    out, at, delta = [], 0, 0
    while outside > 0 and at < len(columns):
        op = columns[at]
        at += 1
        if op == READ_ONLY:
            out.append(READ_ONLY)
            continue
        outside -= 1
        if op == REF_ONLY:
            delta -= 1
        else:
            out.append(READ_ONLY)
            delta += op == EQUAL
    return out + columns[at:], delta


def clip_runs(runs, lead: int, trail: int) -> tuple:
    """(runs, change of the distance) of a script [(length, op)] whose first `lead` and last `trail` reference columns lie outside
    the contig.  Neighbouring columns of one op are one run, so everything converted at an edge, the read-only runs met on the way
    and a read-only run that follows directly are ONE read-only run."""
    columns = [op for n, op in runs for _ in range(n)]
    columns, d_front = walk(columns, lead)
    columns, d_back = walk(columns[::-1], trail)
    return compress(columns[::-1]), d_front + d_back


def clip_hit(starts, lens, L: int, begin: int, end: int, distance: int, runs) -> dict:
    """One placed hit after the clip: contig None = it has no contig base."""
    c = contig_of(starts, lens, L, begin, end)
    if c is None:
        return dict(contig=None)
    lead, trail = max(0, starts[c] - begin), max(0, end - (starts[c] + lens[c]))
    new, delta = clip_runs(runs, lead, trail)
    return dict(contig=c, begin=begin + lead, end=end - trail, distance=distance + delta, runs=new)


def clip_lists(starts, lens, L: int, scores, strand, ref_begin, ref_end, keep, n_ops, cigar, cap: int) -> dict:
    """bgsa_hip_contig_clip_dev on lists [n_reads, k] and rows [n_reads, k, cap] (length << 4 | op): copies of the seven arrays
    after the call, and contig.  Row entries at and behind the new n_ops keep what they held."""
    out = dict(scores=np.array(scores, dtype=np.int32), strand=np.array(strand, dtype=np.int32), ref_begin=np.array(ref_begin, dtype=np.int64),
               ref_end=np.array(ref_end, dtype=np.int64), keep=np.array(keep, dtype=np.int32), n_ops=np.array(n_ops, dtype=np.int32),
               cigar=np.array(cigar, dtype=np.int64))
    n_reads, k = out["scores"].shape
    out["contig"] = np.full((n_reads, k), -1, dtype=np.int32)
    for c in range(n_reads):
        for r in range(k):
            b, e, n = int(out["ref_begin"][c, r]), int(out["ref_end"][c, r]), int(out["n_ops"][c, r])
            if b < 0:
                continue
            which = contig_of(starts, lens, L, b, e)
            if which is None:
                out["ref_begin"][c, r] = out["ref_end"][c, r] = -1
                out["n_ops"][c, r] = 0
                continue
            out["contig"][c, r] = which
            if not 0 <= n <= cap:
                continue
            runs = [(int(w) >> 4, int(w) & 15) for w in out["cigar"][c, r, :n]]
            hit = clip_hit(starts, lens, L, b, e, -int(out["scores"][c, r]), runs)
            out["ref_begin"][c, r], out["ref_end"][c, r], out["scores"][c, r] = hit["begin"], hit["end"], -hit["distance"]
            out["n_ops"][c, r] = len(hit["runs"])
            if len(hit["runs"]) <= cap:
                out["cigar"][c, r, : len(hit["runs"])] = [length << 4 | op for length, op in hit["runs"]]
        out["keep"][c] = M.keep_of(out["strand"][c], out["ref_begin"][c], out["ref_end"][c])
    return out


# ---- the existing pipeline model on the padded reference, then the clip ---------------------------------------------------------------
def place_and_clip(ref: np.ndarray, starts, lens, W: int, St: int, reads, scores, ids, bound: int) -> dict:
    """The lists (scores, ids)[ns, k] placed within `bound` and turned into coordinates of the padded reference (what
    pair_reference.place_lists does), clipped, with the strings of the kept slots: the fields of a ReferenceHits in LINEAR
    coordinates, and contig."""
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
            dist, e, q_begin, runs, _ = R.place(qc[g], sc[c], bound)
            assert dist == -scores[c, r]
            span[p] = (-1 if q_begin is None else q_begin, e, 0, n)
            n_ops[p] = len(runs)
            runs_of[p] = runs
    cap = max(1, int(n_ops.max(initial=0))) + 2
    cigar = np.zeros((ns * k, cap), dtype=np.int64)
    for p, runs in runs_of.items():
        cigar[p, : len(runs)] = [length << 4 | op for length, op in runs]
    strand, begin, end, keep, cigar = M.placements(L, W, St, ids, span, n_ops, cigar, cap)
    out = clip_lists(starts, lens, L, scores, strand, begin, end, keep, n_ops.reshape(ns, k), cigar.reshape(ns, k, cap), cap)
    out["cigars"] = [[M.runs_text([(int(w) >> 4, int(w) & 15) for w in out["cigar"][c, r, : out["n_ops"][c, r]]]) if out["keep"][c, r] else None
                      for r in range(k)] for c in range(ns)]
    out["windows"] = np.array(ids, dtype=np.int32)
    return out


def map_reads_model(sequences, W: int, St: int, P, reads, k_best: int, max_distance=None, blank_bound=None) -> dict:
    """ContigMapper.map_reads (blank_bound None) or map_reads_seeded (blank_bound = min(max_distance, n): every slot beyond it
    blanked, as the seeded entry point leaves them) in LINEAR coordinates: reference_map_reference.map_reads_host's steps on the
    padded reference, then the clip."""
    ref = np.frombuffer(padded(sequences, W, P), dtype=np.uint8)
    starts, _ = layout([len(s) for s in sequences], W, P)
    reads = np.asarray(reads, dtype=np.uint8)
    ns = reads.shape[0]
    n_ids = 2 * M.window_count(ref.size, W, St)
    k_sel = min(64, k_best * (-(-W // St) + 1))
    windows_ascii = M.LETTERS[M.window_rows(classes(ref), W, St, range(n_ids))]
    scores, ids = Q.top_queries(M.window_scores(windows_ascii, reads), ns, k_sel, False)
    if max_distance is None:
        max_distance = int(-np.where(ids >= 0, scores, 0).min())
    if blank_bound is not None:
        gone = (ids < 0) | (-scores.astype(np.int64) > blank_bound)
        scores, ids = np.where(gone, INT32_MIN, scores).astype(np.int32), np.where(gone, -1, ids).astype(np.int32)
    return place_and_clip(ref, starts, [len(s) for s in sequences], W, St, reads, scores, ids, max_distance)


FIELDS = ("scores", "strand", "ref_begin", "ref_end", "keep", "windows", "contig")


def map_ragged_model(sequences, W: int, St: int, P, reads, k_best: int, max_distance: int, seeded: bool) -> dict:
    """The _ragged entry points: read by read what the one-length model gives for that length, in the caller's order."""
    k_sel = min(64, k_best * (-(-W // St) + 1))
    ns = len(reads)
    out = {name: np.zeros((ns, k_sel), dtype=np.int64 if name in ("ref_begin", "ref_end") else np.int32) for name in FIELDS}
    out["cigars"] = [None] * ns
    for n in sorted({len(r) for r in reads}):
        idx = [i for i, r in enumerate(reads) if len(r) == n]
        rows = np.array([list(reads[i]) for i in idx], dtype=np.uint8)
        part = map_reads_model(sequences, W, St, P, rows, k_best, max_distance, min(max_distance, n) if seeded else None)
        for name in FIELDS:
            out[name][idx] = part[name]
        for i, row in zip(idx, part["cigars"]):
            out["cigars"][i] = row
    return out


def local(model: dict, starts) -> dict:
    """A model result as ContigHits reports it: the interval local to the contig."""
    shift = np.where(model["contig"] >= 0, np.asarray(starts, dtype=np.int64)[np.maximum(model["contig"], 0)], 0)
    return dict(model, ref_begin=model["ref_begin"] - shift, ref_end=model["ref_end"] - shift)


def map_pairs_model(sequences, W: int, St: int, P: int, reads1, reads2, insert_min: int, insert_max: int, k_best: int, max_distance: int,
                    rescue_distance=None) -> dict:
    """ContigMapper.map_pairs in LINEAR coordinates: pair_reference.map_pairs_host's stages with every placement clipped — stage A's
    lists before they serve as anchors, stage B's before the pair is chosen."""
    ref = np.frombuffer(padded(sequences, W, P), dtype=np.uint8)
    lens = [len(s) for s in sequences]
    starts, _ = layout(lens, W, P)
    reads = (np.asarray(reads1, dtype=np.uint8), np.asarray(reads2, dtype=np.uint8))
    rescue_distance = max_distance if rescue_distance is None else rescue_distance
    L, ns = ref.size, reads[0].shape[0]
    k_sel = min(64, k_best * (-(-W // St) + 1))
    k_pair = k_sel + k_best * PR.rescue_slots(L, W, St, insert_max)
    assert insert_max <= P and k_pair <= 64
    single = [map_reads_model(sequences, W, St, P, rows, k_best, max_distance, min(max_distance, rows.shape[1])) for rows in reads]
    final, rescued = [], []
    for e, rows in enumerate(reads):
        own, mate = single[e], single[1 - e]
        bound = min(rescue_distance, rows.shape[1])
        scores = np.empty((ns, k_pair), dtype=np.int32)
        ids = np.empty((ns, k_pair), dtype=np.int32)
        for c in range(ns):
            anchors = PR.anchors_of(mate["strand"][c], mate["ref_begin"][c], mate["ref_end"][c], mate["keep"][c], k_best)
            mine = PR.union(own["windows"][c], anchors, L, W, St, insert_max)
            distances = SM.window_distances(ref, W, St, rows[c])
            scores[c], ids[c] = SM.select(mine, [distances[g] for g in mine], bound, k_pair)
        final.append(place_and_clip(ref, starts, lens, W, St, rows, scores, ids, bound))
        rescued.append(np.stack([PR.rescued_of(ids[c], own["windows"][c]) for c in range(ns)]))
    out = dict(single=tuple(single), end1=final[0], end2=final[1], rescued1=rescued[0], rescued2=rescued[1])
    out.update(PR.choose_all(final[0], final[1], insert_min, insert_max))
    return out


# ---- a read against ONE contig ------------------------------------------------------------------------------------------------------
def one_strand_distance(read: bytes, contig: bytes) -> int:
    """Unit-cost distance of the whole read against any stretch of the contig (free ends on the contig; a read base beyond either
    end of the contig is an edit).  Plain DP over bytes, one cell at a time."""
    n = len(read)
    column = list(range(n + 1))      # against the empty stretch: every read base is an edit
    best = column[n]
    for base in contig:
        new = [0] * (n + 1)
        for i in range(1, n + 1):
            new[i] = min(column[i - 1] + (read[i - 1] != base), column[i] + 1, new[i - 1] + 1)
        column = new
        best = min(best, column[n])
    return best


def contig_distance(read: bytes, sequences) -> int:
    """The minimum over the contigs and both strands."""
    return min(one_strand_distance(seq, contig) for contig in sequences for seq in (bytes(read), S.reverse_complement(bytes(read))))


# ---- the contig form of a SAM line ------------------------------------------------------------------------------------------------------
def as_hits(result):
    """A model dict (local coordinates) as the object sam_reference reads: attributes."""
    return SimpleNamespace(**result) if isinstance(result, dict) else result


def placed(hits, c: int, r: int, read: bytes, qual, sequences) -> dict:
    """sam_reference.placed against the hit's own contig: POS and MD are local to it."""
    if r < 0:
        return dict(S.placed(hits, c, r, read, qual, b""), contig=-1)
    which = int(hits.contig[c, r])
    assert 0 <= int(hits.ref_begin[c, r]) <= int(hits.ref_end[c, r]) <= len(sequences[which])
    return dict(S.placed(hits, c, r, read, qual, sequences[which]), contig=which)


def single_records(hits, reads, names, quals, sequences, contig_names, bound: int) -> tuple:
    """(lines, flag, pos, mapq, nm) of ContigMapper.map_reads_sam from the ContigHits of the same arguments."""
    hits = as_hits(hits)
    names = S.default_names(len(reads)) if names is None else names
    lines, flags, poss, mapqs, nms = [], [], [], [], []
    for c, read in enumerate(reads):
        slot, mapq, _, _ = S.list_fields(hits.scores[c], hits.keep[c], bound)
        p = placed(hits, c, slot, bytes(read), None if quals is None else bytes(quals[c]), sequences)
        flag = (16 if p["reverse"] else 0) if p["mapped"] else 4
        lines.append(S.line(names[c], flag, contig_names[p["contig"]] if p["mapped"] else b"*", p["pos"], mapq, p["cigar"], b"*", 0, 0, p["seq"],
                            p["qual"], p["nm"], p["md"]))
        flags.append(flag)
        poss.append(p["pos"])
        mapqs.append(mapq)
        nms.append(-1 if p["nm"] is None else p["nm"])
    return lines, flags, poss, mapqs, nms


def pair_records(paired, reads1, reads2, names, quals1, quals2, sequences, contig_names, starts, bounds) -> tuple:
    """(lines, flag, pos, mapq, nm) of ContigMapper.map_pairs_sam from its map_pairs result (ends local): RNEXT '=' on one contig,
    else the mate's name; an unmapped end takes its mate's contig and '='; TLEN 0 across contigs, else from the linear interval."""
    names = S.default_names(len(reads1)) if names is None else names
    lines, flags, poss, mapqs, nms = [], [], [], [], []
    for c in range(len(reads1)):
        ends = []
        for hits, slot, reads, quals in ((paired.end1, paired.slot1, reads1, quals1), (paired.end2, paired.slot2, reads2, quals2)):
            ends.append(placed(as_hits(hits), c, int(slot[c]), bytes(reads[c]), None if quals is None else bytes(quals[c]), sequences))
        alone = [S.list_fields(hits.scores[c], hits.keep[c], bound) for hits, bound in zip((paired.end1, paired.end2), bounds)]
        mapq = S.pair_fields(int(paired.proper[c]), int(paired.n_best[c]), int(paired.cost[c]), int(paired.next_cost[c]), alone[0][1], alone[1][1])
        tlen = (0, 0)
        if ends[0]["mapped"] and ends[1]["mapped"] and ends[0]["contig"] == ends[1]["contig"]:
            tlen = S.tlen_fields(ends[0]["begin"], ends[0]["end"], ends[1]["begin"], ends[1]["end"])
        for e, (me, mate) in enumerate(((ends[0], ends[1]), (ends[1], ends[0]))):
            flag = 1 | (2 if paired.proper[c] else 0) | (0 if me["mapped"] else 4) | (0 if mate["mapped"] else 8) | \
                (16 if me["reverse"] else 0) | (32 if mate["reverse"] else 0) | (64, 128)[e]
            named = me if me["mapped"] else mate if mate["mapped"] else None
            pos = named["pos"] if named else 0
            rnext = b"*" if not mate["mapped"] else b"=" if not me["mapped"] or me["contig"] == mate["contig"] else contig_names[mate["contig"]]
            lines.append(S.line(names[c], flag, contig_names[named["contig"]] if named else b"*", pos, mapq[e] if me["mapped"] else 0, me["cigar"],
                                rnext, mate["pos"] if mate["mapped"] else 0, tlen[e], me["seq"], me["qual"], me["nm"], me["md"]))
            flags.append(flag)
            poss.append(pos)
            mapqs.append(mapq[e] if me["mapped"] else 0)
            nms.append(-1 if me["nm"] is None else me["nm"])
    return lines, flags, poss, mapqs, nms


def fields_of(line: bytes) -> dict:
    f = line.rstrip(b"\n").split(b"\t")
    out = dict(qname=f[0], flag=int(f[1]), rname=f[2], pos=int(f[3]), mapq=int(f[4]), cigar=f[5].decode(), rnext=f[6], pnext=int(f[7]),
               tlen=int(f[8]), seq=f[9], qual=f[10], nm=None, md=None)
    if len(f) > 11:
        out.update(nm=int(f[11][5:]), md=f[12][5:].decode())
    return out


# ---- the fixture ----------------------------------------------------------------------------------------------------------------------
FIXTURE = dict(W=48, S=8, N=24, MAX_DISTANCE=4, K_BEST=2, LENS=(30, 200, 90, 24, 10), PADDINGS=(48, 70),
               NAMES=(b"tiny", b"chrA", b"chrB", b"read-long", b"stub"))
TINY, CHR_A, CHR_B, READ_LONG, STUB = range(5)     # below the window; ordinary; ordinary; as long as a read; shorter than a read
PAIRS = dict(INSERT_MIN=60, INSERT_MAX=120, PADDING=120, K_BEST=1)


def contigs(seed: int = 20) -> list:
    rng = np.random.default_rng(seed)
    return [ACGT[rng.integers(4, size=n)].tobytes() for n in FIXTURE["LENS"]]


def other(base: int) -> int:
    return b"CGTA"[b"ACGT".index(base)]


def crafted(sequences) -> list:
    """[(class, strand '+' | '-', read)]: every class on both strands, 24 bp each.  A '-' read is what the mapper gets: the reverse
    complement of the sequence the class describes."""
    a, b, tiny, same = sequences[CHR_A], sequences[CHR_B], sequences[TINY], sequences[READ_LONG]
    n, junk = FIXTURE["N"], b"GTCAG"
    one = bytearray(a[80:104])
    one[10] = other(one[10])
    two = bytearray(a[110:122] + a[123:135])          # a base of the contig skipped ...
    two[4] = other(two[4])                            # ... and a substitution
    three = bytearray(b[30:41] + b"A" + b[41:53])     # a base put in, and two substitutions
    three[3], three[20] = other(three[3]), other(three[20])
    forward = [("interior exact", a[50:74]), ("interior 1 edit", bytes(one)), ("interior 2 edits", bytes(two)), ("interior 3 edits", bytes(three)),
               ("inside the contig below the window", tiny[3:27]),
               ("flush at the first base", a[:n]), ("flush at the last base", a[-n:]),
               ("the read-long contig itself", same),
               ("N tail over the end", a[-(n - 3):] + b"NNN"),
               ("all N", b"N" * n)]
    for over in (1, 3, 5):
        forward.append((f"over the start by {over}", junk[:over] + b[: n - over]))
        forward.append((f"over the end by {over}", b[-(n - over):] + junk[:over]))
    out = []
    for name, read in forward:
        assert len(read) == n, name
        out.append((name, "+", bytes(read)))
        out.append((name, "-", S.reverse_complement(bytes(read))))
    return out


def crafted_unbounded(sequences) -> dict:
    """Reads for max_distance=None, one length per call, both strands: {length: [(class, strand, read)]}.
    'around the stub': 7 N, the 10 bp contig, 7 N.  Nothing lies behind the last contig, so the traceback leaves the last 7 bases
    read-only itself and the clip works on the front: 7 '=' on padding become read-only, the distance goes from 7 to 14.
    'around the read-long contig': 3 N, the 24 bp contig, 3 N — 30 bp: ONE run of 30 '=' holds the contig and is cut on both sides,
    the distance goes from 0 to 6."""
    out = {}
    for name, read in (("around the stub", b"N" * 7 + sequences[STUB] + b"N" * 7), ("around the read-long contig", b"NNN" + sequences[READ_LONG] + b"NNN")):
        out[len(read)] = [(name, "+", read), (name, "-", S.reverse_complement(read))]
    return out


def crafted_pairs(sequences) -> list:
    """[(class, read 1, read 2)], 2 x 24 bp, library type FR, for insert range 60..120 and padding 120."""
    a, b, n = sequences[CHR_A], sequences[CHR_B], FIXTURE["N"]
    nowhere = ACGT[np.random.default_rng(77).integers(4, size=n)].tobytes()
    return [("proper inside one contig", a[20:44], S.reverse_complement(a[96:120])),
            ("mates on neighbouring contigs", a[-n:], S.reverse_complement(b[:n])),
            ("end 2 unmapped", a[60:84], nowhere)]


# ---- hand-written hits for the clip alone -------------------------------------------------------------------------------------------
CLIP_LAYOUT = dict(W=8, lens=(20, 10, 5))      # padding 8: contigs at [0, 20), [28, 38), [46, 51); L = 51
SENTINEL = 0x5A5A5A5                           # what a row holds behind its runs
_R, _I, _E, _X = REF_ONLY, READ_ONLY, EQUAL, DIFF
# name -> ((strand, begin, end, distance, runs), what the rule gives: None = unplaced, else (contig, begin, end, distance, runs))
CLIP_CASES = {
    "inside its contig": ((0, 2, 12, 0, [(10, _E)]), (0, 2, 12, 0, [(10, _E)])),
    "the first run splits": ((0, 25, 38, 5, [(5, _X), (8, _E)]), (1, 28, 38, 5, [(3, _I), (2, _X), (8, _E)])),
    "= on padding": ((1, 25, 38, 0, [(13, _E)]), (1, 28, 38, 3, [(3, _I), (10, _E)])),
    "reference-only columns are dropped": ((0, 26, 38, 2, [(2, _R), (10, _E)]), (1, 28, 38, 0, [(10, _E)])),
    "a read-only run on the way": ((0, 26, 38, 4, [(1, _X), (2, _I), (1, _X), (10, _E)]), (1, 28, 38, 4, [(4, _I), (10, _E)])),
    "a read-only run follows directly": ((0, 27, 38, 3, [(1, _X), (2, _I), (10, _E)]), (1, 28, 38, 3, [(3, _I), (10, _E)])),
    "the tail, mirrored": ((1, 10, 23, 3, [(10, _E), (3, _X)]), (0, 10, 20, 3, [(10, _E), (3, _I)])),
    "the tail drops and converts": ((0, 10, 24, 4, [(10, _E), (1, _I), (1, _R), (3, _E)]), (0, 10, 20, 6, [(10, _E), (4, _I)])),
    "one run holds the contig": ((0, 25, 41, 16, [(16, _X)]), (1, 28, 38, 16, [(3, _I), (10, _X), (3, _I)])),
    "two more runs": ((1, 26, 40, 8, [(4, _X), (6, _E), (4, _X)]), (1, 28, 38, 8, [(2, _I), (2, _X), (6, _E), (2, _X), (2, _I)])),
    "padding only": ((0, 21, 27, 0, [(6, _E)]), None),
    "an empty interval in a contig": ((0, 30, 30, 4, [(4, _I)]), (1, 30, 30, 4, [(4, _I)])),
    "an empty interval on padding": ((0, 24, 24, 4, [(4, _I)]), None),
    "a contig below the read": ((0, 44, 51, 3, [(7, _E), (3, _I)]), (2, 46, 51, 5, [(2, _I), (5, _E), (3, _I)])),
    "ends where the next contig begins": ((0, 15, 28, 8, [(5, _E), (8, _X)]), (0, 15, 20, 8, [(5, _E), (8, _I)])),
}
# two hits of one read that meet before the clip and not after it: the second is kept only on the clipped intervals
CLIP_KEEP_CASE = [(0, 15, 23, 3, [(5, _E), (3, _X)]), (0, 20, 30, 8, [(8, _X), (2, _E)])]


def clip_case_lists(k: int, cap: int) -> dict:
    """Every hit of CLIP_CASES, then the two of CLIP_KEEP_CASE side by side, packed k slots to a read (the rest unused slots):
    the seven arrays as bgsa_hip_reference_placements_dev leaves them, rows filled with SENTINEL behind their runs."""
    hits = [hit for hit, _ in CLIP_CASES.values()]
    rows = [hits[i: i + k] for i in range(0, len(hits), k)] if k > 1 else [[hit] for hit in hits]
    rows += [CLIP_KEEP_CASE[:k]] if k > 1 else []
    n = len(rows)
    out = dict(scores=np.full((n, k), INT32_MIN, np.int32), strand=np.full((n, k), -1, np.int32), ref_begin=np.full((n, k), -1, np.int64),
               ref_end=np.full((n, k), -1, np.int64), keep=np.zeros((n, k), np.int32), n_ops=np.zeros((n, k), np.int32),
               cigar=np.full((n, k, cap), SENTINEL, np.int32))
    for c, row in enumerate(rows):
        for r, (strand, begin, end, distance, runs) in enumerate(row):
            out["scores"][c, r], out["strand"][c, r], out["ref_begin"][c, r], out["ref_end"][c, r] = -distance, strand, begin, end
            out["n_ops"][c, r] = len(runs)
            out["cigar"][c, r, : min(len(runs), cap)] = [length << 4 | op for length, op in runs][:cap]
        out["keep"][c] = M.keep_of(out["strand"][c], out["ref_begin"][c], out["ref_end"][c])
    return out

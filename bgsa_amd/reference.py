"""Reads mapped onto ONE reference sequence: the windows are cut on the device, on both strands, and the hits come back in
reference coordinates (include/bgsa_hip.h "a reference as the query set").

The geometry is stated once in the header and restated here (window_plan, max_stride): L mapped bytes, 1 <= S <= W <= L,
n_windows = 1 + ceil((L - W) / S), start(w) = min(w * S, L - W); forward window w has id w, its reverse complement id
n_windows + w.

ONE pipeline maps reads, behind four entry points: check_call refuses, a plan names the bins [(indices, seed length or None)],
ReferenceMapper._map_bins runs every bin as one bucket (_map_bucket: upload, select_windows or select_seeded, place_hits) and
scatters it into the caller's order (decode_cigars), and the seeded entry points send the reads their filter does not cover through
the exhaustive entry point of the same kind (merge_fallback, seed_stats).  The helpers at module level need no device.

Paired reads (include/bgsa_hip.h "paired reads") are that pipeline with a second source of candidates:
map_pairs maps each end through map_reads_seeded (or map_reads), then per end joins the windows its mate's hits point at
(rescue_slots, rescue_region, pair_rescue_windows) to the end's own, runs the seeded steps and place_hits on the union at the
rescue bound, and chooses the best proper pair on the device (pair_select); check_pair_call makes every refusal first.

A reference of SEVERAL contigs (include/bgsa_hip.h "a reference of several contigs") is that one sequence with
padding between the contigs (contig_layout): ContigMapper builds it, lets the pipeline above run unchanged, clips every placed hit
to its contig on the device right after place_hits (the hook _after_place), and reports contig and local coordinates (ContigHits);
its SAM records go through the contig form of the two record passes.

BAM (include/bgsa_hip.h "BAM records") is the SAM stage with another encoding behind the same field assembly:
map_reads_bam / map_pairs_bam run the SAM entry points' mapping with fmt="bam", and sam_records then measures, scans, emits and
frames the records into BGZF blocks of stored deflate — or, with compress=True, deflates them on the device (LZ77 and dynamic
Huffman codes) and packs the blocks —; bam_header, bgzf_blocks and write_bam make a file of them on the host.  With sort=True
(include/bgsa_hip.h "BAM records: coordinate order and index") the records of one call are put in coordinate
order before the passes — keys by a kernel, torch.sort, the per-record tensors gathered — and the arrays of a BAI index are built
after them (SortedBamRecords, BamIndex); bai_bytes and write_bam(index=True) write x.bam.bai beside x.bam.
"""
from __future__ import annotations

import struct
import zlib
from typing import NamedTuple

import numpy as np

import bgsa_amd as B

INT32_MAX = 2 ** 31 - 1


def window_plan(ref_len: int, window_len: int, stride: int) -> tuple[int, np.ndarray]:
    """(n_windows, starts int64[n_windows]) of a reference of ref_len bases cut into windows of window_len every stride bases,
    the last one anchored at the reference's end.  Pure Python: no device, no library."""
    L, W, S = int(ref_len), int(window_len), int(stride)
    if not 1 <= S <= W <= L:
        raise B.BgsaHipError(f"window_plan: rc=-1: needs 1 <= stride <= window_len <= ref_len, got stride {S}, window_len {W}, ref_len {L}")
    n = 1 + -(-(L - W) // S)
    return n, np.minimum(np.arange(n, dtype=np.int64) * S, L - W)


def max_stride(window_len: int, read_len: int, max_distance: int) -> int:
    """The largest stride at which every placement of a read_len bp read within max_distance lies wholly inside at least one
    window: such a placement spans at most read_len + B reference bases, B = min(max_distance, read_len), and every interval of
    that length is inside a window exactly when stride <= window_len - (read_len + B) + 1.  Below 1: no stride does."""
    n = int(read_len)
    return int(window_len) - (n + min(int(max_distance), n)) + 1


SEED_LEN_MAX = 13      # 4^13 + 1 index offsets; include/bgsa_hip.h "seeded read mapping"
INT32_MIN = -2 ** 31
# map_reads_seeded's default max_candidates is max(n_ids // SEED_CAP_FRACTION, SEED_MIN_CANDIDATES).  The fraction is measured
# (profiles/seeded_map.txt, LABNOTES.md §27.3): at 83,682 ids, sort + verify + select of C candidates per read meet the exhaustive
# selection between C = 16,384 and 32,768; n_ids / 8 is the largest power-of-two fraction below that.  The floor: on a small
# reference n_ids / 8 is a handful, fewer than the (B + 1) * ceil(W / S) candidates a read's own locus emits, and every read would
# take the exhaustive path; 256 candidates per read cost a third of the exhaustive selection even at 8,368 ids.
SEED_CAP_FRACTION = 8
SEED_MIN_CANDIDATES = 256


def seed_plan(read_len: int, max_distance: int, seed_len=None) -> tuple[int, int, int]:
    """(B, step, q) of the pigeonhole filter for reads of read_len bp within max_distance: B = min(max_distance, n), the B + 1
    pieces start step = n // (B + 1) apart (piece j at j * step) and are q = seed_len long; seed_len=None: min(12, step).
    step < q — the pieces would overlap, and B edits could then touch all of them — raises, naming the largest bound this
    seed_len allows and the largest seed_len this bound allows.  Pure Python: no device, no library."""
    n = int(read_len)
    if n < 1 or int(max_distance) < 0:
        raise B.BgsaHipError("seed_plan: rc=-1: read_len must be positive and max_distance not negative")
    bound = min(int(max_distance), n)
    step = n // (bound + 1)
    q = min(12, step) if seed_len is None else int(seed_len)
    if seed_len is not None and not 1 <= q <= SEED_LEN_MAX:
        raise B.BgsaHipError(f"seed_plan: rc=-1: seed_len must lie in 1..{SEED_LEN_MAX}")
    if step < q or q < 1:
        longest = min(step, SEED_LEN_MAX)
        by_len = f"seed_len {q} allows max_distance <= {n // q - 1}" if 1 <= q <= n else f"no bound allows seed_len {q}"
        by_bound = f"max_distance {bound} allows seed_len <= {longest}" if longest >= 1 else f"max_distance {bound} allows no seed"
        raise B.BgsaHipError(f"seed_plan: rc=-1: the {bound + 1} pieces of a {n} bp read within distance {bound} start {step} bp apart, "
                             f"too close for seeds of {q} bp: {by_len}; {by_bound}")
    return bound, step, q


def seed_plan_ragged(lens, max_distance: int, seed_len=None) -> list:
    """[(indices, q)] for reads of the lengths `lens` within max_distance: the bins of bin_by_words(lens), in its order, each with the
    seed length its pass uses.  seed_len=None: q = min(12, max(1, step of the bin's shortest read)), that read's step being
    n // (min(max_distance, n) + 1) — the shortest read has the smallest step of its bin, so every longer read's pieces are at least
    q apart too; a read no longer than the bound has step 0, gets q = 1 and is flagged too short (-3) by the candidate call.
    seed_len given: that value for every bin, refused outside 1..SEED_LEN_MAX; the reads whose own step is below it are flagged.
    One q per bin, not per read: a q per read would need one index per distinct step resident at once.  Pure Python: no device,
    no library."""
    if int(max_distance) < 0:
        raise B.BgsaHipError("seed_plan_ragged: rc=-1: max_distance is negative")
    if seed_len is not None and not 1 <= int(seed_len) <= SEED_LEN_MAX:
        raise B.BgsaHipError(f"seed_plan_ragged: rc=-1: seed_len must lie in 1..{SEED_LEN_MAX}")
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    out = []
    for idx in B.bin_by_words(lens):
        n = int(lens[idx].min())
        out.append((idx, int(seed_len) if seed_len is not None else min(12, max(1, n // (min(int(max_distance), n) + 1)))))
    return out


def blank_beyond(hits: "ReferenceHits", bound: int) -> "ReferenceHits":
    """map_reads' result with every slot whose distance exceeds `bound` (and every unused slot) blanked: scores INT32_MIN, windows,
    strand, ref_begin and ref_end -1, keep 0, cigar None.  This is what map_reads_seeded returns, bit for bit.  (A result without
    strings — cigars None, the SAM path's — stays without.)"""
    gone = (hits.windows < 0) | (-hits.scores.astype(np.int64) > int(bound))
    cigars = None if hits.cigars is None else [[None if gone[c, r] else text for r, text in enumerate(row)] for c, row in enumerate(hits.cigars)]
    return ReferenceHits(np.where(gone, INT32_MIN, hits.scores).astype(np.int32), np.where(gone, -1, hits.strand).astype(np.int32),
                         np.where(gone, -1, hits.ref_begin).astype(np.int64), np.where(gone, -1, hits.ref_end).astype(np.int64),
                         np.where(gone, 0, hits.keep).astype(np.int32), cigars, np.where(gone, -1, hits.windows).astype(np.int32))


def rescue_slots(ref_len: int, window_len: int, stride: int, insert_max: int) -> int:
    """R of include/bgsa_hip.h "paired reads": the most rescue windows one anchor can name, min(n_windows, ceil((insert_max + W - 1)
    / S) + 1) — a region is at most insert_max long, so the starts of the windows that meet it lie in a range of insert_max + W - 1
    bases: that many strides' worth of regular windows, and the anchored last one.  Pure Python: no device, no library."""
    n_windows = window_plan(ref_len, window_len, stride)[0]
    if int(insert_max) < 1:
        raise B.BgsaHipError("rescue_slots: rc=-1: insert_max is not positive")
    return min(n_windows, -(-(int(insert_max) + int(window_len) - 1) // int(stride)) + 1)


def rescue_region(strand: int, begin: int, end: int, insert_max: int, ref_len: int) -> tuple[int, int]:
    """[lo, hi) on the forward reference in which the mate of an anchor on `strand` with interval [begin, end) lies (library type FR:
    the mate is on strand 1 - strand, the forward-strand mate upstream): [begin, min(L, begin + insert_max)) behind a forward
    anchor, [max(0, end - insert_max), end) in front of a reverse one.  Pure Python: no device, no library."""
    if int(strand) == 0:
        return int(begin), min(int(ref_len), int(begin) + int(insert_max))
    return max(0, int(end) - int(insert_max)), int(end)


def check_pair_call(both_strands: bool, shape1, shape2, insert_min, insert_max, k_best, max_distance, rescue_distance, seeded: bool,
                    seed_len, max_candidates, cigar_cap, window_len: int, stride: int, ref_len: int, n_ids: int) -> dict:
    """Every refusal of map_pairs, in one order: a mapper of one strand, unequal row counts, the insert range, a missing
    max_distance, rescue_distance below max_distance, the stride rule at rescue_distance for end 1 then end 2, k_pair beyond 64 —
    the message names the largest k_best and the largest insert_max that fit —, then what the per-end entry point refuses
    (check_call, end 1 then end 2: the 1,024 bp limit, k_best, a negative bound, the seed plan, cigar_cap, max_candidates).
    shape_e = (ns, n_e).  Returns what the stages need: k_best, k_sel, R, k_pair, rescue_distance, and per end the rescue bound
    and the cigar cap.  Nothing is launched or allocated here, so a refused call leaves the mapper as it was."""
    who = "map_pairs"
    W, S = int(window_len), int(stride)
    if not both_strands:
        raise B.BgsaHipError(f"{who}: rc=-1: the mates of a pair lie on opposite strands: the mapper needs both_strands=True")
    if shape1[0] != shape2[0]:
        raise B.BgsaHipError(f"{who}: rc=-1: row c of both arrays is pair c, got {shape1[0]} and {shape2[0]} rows")
    if not 1 <= int(insert_min) <= int(insert_max) <= INT32_MAX:
        raise B.BgsaHipError(f"{who}: rc=-1: needs 1 <= insert_min <= insert_max, got {insert_min} and {insert_max}")
    if max_distance is None:
        raise B.BgsaHipError(f"{who}: rc=-1: max_distance is required: the single-end lists and the rescue bound are derived from it")
    rescue_distance = int(max_distance) if rescue_distance is None else int(rescue_distance)
    if rescue_distance < int(max_distance):
        raise B.BgsaHipError(f"{who}: rc=-1: rescue_distance {rescue_distance} is below max_distance {int(max_distance)}")
    lens = (int(shape1[1]), int(shape2[1]))
    for e, n in enumerate(lens, start=1):
        largest = max_stride(W, n, rescue_distance)
        if S > largest:
            allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
            raise B.BgsaHipError(f"{who}: rc=-1: at stride {S} a placement of end {e} ({n} bp) within rescue_distance {min(rescue_distance, n)} "
                                 f"can lie in no window of {W} bp: {allowed}")
    n_windows = window_plan(ref_len, W, S)[0]
    per_locus = -(-W // S) + 1

    def k_pair_of(k: int, slots: int) -> int:
        return min(B.V_NUM, k * per_locus) + k * slots
    k_best, R = int(k_best), rescue_slots(ref_len, W, S, insert_max)
    k_sel, k_pair = min(B.V_NUM, max(k_best, 0) * per_locus), k_pair_of(max(k_best, 0), R)
    if k_pair > B.V_NUM:
        fits = max((k for k in range(1, min(k_best, B.V_NUM)) if k_pair_of(k, R) <= B.V_NUM), default=0)
        room = (B.V_NUM - k_sel) // k_best      # rescue slots per anchor that fit beside the single-end list
        widest = int(insert_max) if n_windows <= room else (room - 1) * S - W + 1
        by_k = f"at insert_max {int(insert_max)} the largest k_best is {fits}" if fits else f"no k_best fits insert_max {int(insert_max)}"
        by_insert = f"at k_best {k_best} the largest insert_max is {widest}" if room >= 1 and widest >= 1 else f"no insert_max fits k_best {k_best}"
        raise B.BgsaHipError(f"{who}: rc=-1: k_pair = k_sel + k_best * R = {k_sel} + {k_best} * {R} = {k_pair} slots per end exceed "
                             f"{B.V_NUM}: {by_k}; {by_insert}")
    bounds, caps = [], []
    for n in lens:
        plan = (lambda limit, n=n: seed_plan(n, limit, seed_len)) if seeded else None
        cap = check_call(who, n, False, k_best, max_distance, seeded, cigar_cap, max_candidates, W, S, ref_len, n_ids, True, plan)[2]
        bounds.append(min(rescue_distance, n))
        caps.append(cap)
    return dict(k_best=k_best, k_sel=k_sel, rescue_slots=R, k_pair=k_pair, rescue_distance=rescue_distance, bounds=tuple(bounds),
                caps=tuple(caps))


class ReferenceHits(NamedTuple):
    """What ReferenceMapper.map_reads returns, numpy, one row per read and one column per selected hit, best first."""
    scores: np.ndarray      # [ns, k_sel] int32: minus the distance of the read inside its r-th best window; INT32_MIN = unused slot
    strand: np.ndarray      # [ns, k_sel] int32: 0 forward, 1 reverse, -1 unused slot
    ref_begin: np.ndarray   # [ns, k_sel] int64: half-open interval on the forward reference, -1 where the hit is not placed
    ref_end: np.ndarray     # [ns, k_sel] int64
    keep: np.ndarray        # [ns, k_sel] int32: 1 = the best view of its locus, 0 = unplaced, or a locus already reported
    cigars: list            # cigars[c][r]: the edit script along the forward reference, or None where keep is 0
    windows: np.ndarray     # [ns, k_sel] int32: the window ids behind the hits (reverse ones from n_windows on), -1 = unused


class Placement(NamedTuple):
    strand: int
    ref_begin: int
    ref_end: int
    distance: int
    cigar: str


class PairedHits(NamedTuple):
    """What ReferenceMapper.map_pairs returns, numpy, one row per pair (include/bgsa_hip.h "paired reads")."""
    end1: ReferenceHits     # end 1's final list, k_pair wide: its single-end hits and the rescued ones, best first
    end2: ReferenceHits
    rescued1: np.ndarray    # [ns, k_pair] bool: the slot's window is not among the end's single-end windows
    rescued2: np.ndarray
    proper: np.ndarray      # [ns] int32: 1 = a proper combination was chosen
    slot1: np.ndarray       # [ns] int32: the chosen slot of end1 (not proper: its first kept slot), -1 = none
    slot2: np.ndarray
    insert: np.ndarray      # [ns] int64: R.end - F.begin of the chosen combination, 0 when not proper
    cost: np.ndarray        # [ns] int32: d1 + d2 of the chosen slots
    n_best: np.ndarray      # [ns] int32: the proper combinations at the chosen cost
    next_cost: np.ndarray   # [ns] int32: the smallest proper cost above the chosen one, -1 = none


# ---- the host side of the four map_reads entry points: no device, no library ---------------------------------------------------
def check_call(who: str, longest: int, ragged: bool, k_best, max_distance, seeded: bool, cigar_cap, max_candidates,
               window_len: int, stride: int, ref_len: int, n_ids: int, limit_1024: bool, plan=None) -> tuple:
    """Every refusal of the map_reads entry point `who`, in one order: the 1,024 bp limit (limit_1024: every entry point but
    map_reads), k_best, max_distance (seeded: required), the seed plan (plan(max_distance), a call that raises or returns what the
    caller needs: seed_plan or seed_plan_ragged), the stride rule for the longest read, and for a seeded call the int32 index, then
    cigar_cap and max_candidates.  ragged picks the wording for a list of mixed lengths.  Returns (k_best, bound, cap,
    max_candidates, plan's result): bound = min(max_distance, longest), 0 for max_distance=None; cap = window_len + longest unless
    cigar_cap says otherwise; max_candidates None unless seeded, its default max(n_ids // 8, 256).  Nothing is launched or
    allocated here, so a refused call leaves the mapper as it was."""
    longest = int(longest)
    if limit_1024 and longest > 1024:
        why = "have no per-lane form (one length per call: map_reads)" if ragged else "have no verify kernel (map_reads takes them)"
        raise B.BgsaHipError(f"{who}: rc=-2: reads beyond 1,024 bp {why}")
    k_best = int(k_best)
    if not 1 <= k_best <= B.V_NUM:
        raise B.BgsaHipError(f"{who}: rc=-1: k_best must lie in 1..{B.V_NUM}")
    if seeded and max_distance is None:
        raise B.BgsaHipError(f"{who}: rc=-1: max_distance is required: the seed filter is derived from it "
                             f"({who.replace('_seeded', '')} takes max_distance=None)")
    if max_distance is not None and int(max_distance) < 0:
        raise B.BgsaHipError(f"{who}: rc=-1: max_distance is negative")
    planned = None if plan is None else plan(int(max_distance))
    bound = 0 if max_distance is None else min(int(max_distance), longest)
    largest = max_stride(window_len, longest, bound)
    if stride > largest:
        allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
        read = f"the longest read ({longest} bp)" if ragged else f"a {longest} bp read"
        raise B.BgsaHipError(f"{who}: rc=-1: at stride {stride} a placement of {read} within distance {bound} can lie in no window of "
                             f"{window_len} bp: {allowed}")
    if seeded and ref_len > INT32_MAX:
        raise B.BgsaHipError(f"{who}: rc=-1: the index holds int32 positions: a reference beyond 2^31 - 1 bases goes in parts")
    cap = window_len + longest if cigar_cap is None else int(cigar_cap)
    if cap < 1:
        raise B.BgsaHipError(f"{who}: rc=-1: cigar_cap is not positive")
    if seeded:
        max_candidates = max(n_ids // SEED_CAP_FRACTION, SEED_MIN_CANDIDATES) if max_candidates is None else int(max_candidates)
        if max_candidates < 0:
            raise B.BgsaHipError(f"{who}: rc=-1: max_candidates is negative")
    return k_best, bound, cap, (max_candidates if seeded else None), planned


def hit_arrays(hits: ReferenceHits) -> tuple:
    """The six arrays of a result, cigars left out: scores, strand, ref_begin, ref_end, keep, windows."""
    return hits[:5] + (hits.windows,)


def blank_hits(ns: int, k: int, cigars) -> ReferenceHits:
    """A result of ns reads whose every slot is unused: scores INT32_MIN, windows, strand and the interval -1, keep 0."""
    blank = np.full((ns, k), -1, dtype=np.int32)
    return ReferenceHits(np.full((ns, k), INT32_MIN, dtype=np.int32), blank, np.full((ns, k), -1, dtype=np.int64),
                         np.full((ns, k), -1, dtype=np.int64), np.zeros((ns, k), dtype=np.int32), cigars, blank.copy())


def decode_cigars(who: str, keep, n_ops, runs, cap: int, idx, cigars: list) -> None:
    """The edit scripts of one bin into the caller's order: keep and n_ops [n, k_sel], runs [n, k_sel, cap] uint32 (length << 4 | op)
    are the host copies of what place_hits returns for the bin, idx[c] is where the bin's read c stands in the caller's order.
    cigars[idx[c]][r] becomes the string of every kept slot; the others are left as they are (None).  A kept hit with more runs
    than its row holds raises, naming that read in the caller's order."""
    at = np.asarray(idx).tolist()
    kept = np.nonzero(keep)
    for c, r, n in zip(kept[0].tolist(), kept[1].tolist(), n_ops[kept].tolist()):
        if n > cap:
            raise B.BgsaHipError(f"{who}: hit {r} of read {at[c]} has {n} runs, its row holds {cap} (raise cigar_cap)")
        cigars[at[c]][r] = "".join(f"{w >> 4}{B.CIGAR_OPS[w & 15]}" for w in runs[c, r, :n].tolist())


def merge_fallback(out: ReferenceHits, rest, full: ReferenceHits) -> None:
    """Row i of `full` — the exhaustive result, blanked, of the reads the seed filter does not cover — into row rest[i] of `out`:
    the six arrays and the cigar rows.  Nothing else of `out` changes."""
    for mine, theirs in zip(hit_arrays(out), hit_arrays(full)):
        mine[rest] = theirs
    for at, row in zip(np.asarray(rest).tolist(), full.cigars):
        out.cigars[at] = row


def seed_stats(flags, totals, seed_len, max_candidates: int, bins=None) -> dict:
    """last_seed_stats from the reads' flags (a candidate count, or -1 an 'N' in a piece, -2 above max_candidates, -3 too short for
    the seed) and the totals (emitted, unique, within the bound).  bins (map_reads_seeded_ragged: one dict per bin) adds the keys
    reads_fallback_short and bins; without it the dict is map_reads_seeded's."""
    flags = np.asarray(flags)
    stats = dict(reads_seeded=int((flags >= 0).sum()), reads_fallback_n=int((flags == -1).sum()),
                 reads_fallback_cap=int((flags == -2).sum()))
    if bins is not None:
        stats["reads_fallback_short"] = int((flags == -3).sum())
    stats.update(candidates_emitted=int(totals[0]), candidates_unique=int(totals[1]), candidates_within_bound=int(totals[2]),
                 seed_len=seed_len, max_candidates=max_candidates)
    if bins is not None:
        stats["bins"] = bins
    return stats


# ---- SAM records: include/bgsa_hip.h "SAM records" — the host side, no device, no library ---------------------------------------
class SamRecords(NamedTuple):
    """What ReferenceMapper.map_reads_sam and map_pairs_sam return: the records' text as the device wrote it, and four columns."""
    text: np.ndarray        # uint8: the records, one line each, without a header
    offsets: np.ndarray     # int64[n + 1]: record i is text[offsets[i] : offsets[i + 1]]
    flag: np.ndarray        # int32[n]
    pos: np.ndarray         # int64[n]: POS, 1-based; 0 for an unmapped record without a mapped mate
    mapq: np.ndarray        # int32[n]
    nm: np.ndarray          # int32[n]: the distance, -1 for an unmapped record


def list_mapq(d1: int, n1: int, d2, bound: int) -> int:
    """The MAPQ of a hit list whose primary slot has distance d1 and n1 kept slots at that distance, d2 the smallest kept distance
    above d1 (None or -1: none), bound the distance the list is complete within (-1: none).  The header's heuristic, in integers."""
    if n1 >= 2:
        return 3 if n1 == 2 else 2 if n1 == 3 else 1 if n1 <= 9 else 0
    gap = d2 - d1 if d2 is not None and d2 >= 0 else bound + 1 - d1 if bound >= 0 else 6
    return max(0, min(60, 10 * gap))


def pair_mapq(torch, proper, n_best, cost, next_cost, alone1, alone2) -> tuple:
    """The two ends' MAPQ from pair_select's outputs and the ends' list MAPQs (alone_e), elementwise on tensors: a proper pair gets
    the table value of n_best >= 2, else min(60, 10 * (next_cost - cost)), 60 without a next cost; an end of a pair that is not
    proper keeps its own."""
    table = 3 - (n_best >= 3).to(torch.int32) - (n_best >= 4).to(torch.int32) - (n_best >= 10).to(torch.int32)
    gap = (10 * (next_cost - cost)).clamp(min=0, max=60).masked_fill(next_cost < 0, 60)
    both = torch.where(n_best >= 2, table, gap.to(torch.int32))
    return torch.where(proper != 0, both, alone1), torch.where(proper != 0, both, alone2)


def _field_bytes(who: str, what: str, text) -> np.ndarray:
    """A name as uint8, refused where it is empty or holds a byte outside '!'..'~'."""
    if isinstance(text, str):
        text = text.encode("ascii", "replace")
    name = np.array(bytearray(text), dtype=np.uint8)
    if name.size == 0:
        raise B.BgsaHipError(f"{who}: rc=-1: {what} is empty")
    if ((name < 33) | (name > 126)).any():
        raise B.BgsaHipError(f"{who}: rc=-1: {what} holds a tab, a space, a newline or another byte outside '!'..'~'")
    return name


def check_sam_call(who: str, lens, names, quals, reference_name) -> tuple:
    """Every refusal the SAM entry point `who` adds to the mapping call's own, before anything is launched: reference_name and every
    name non-empty and of bytes '!'..'~' (no tab, space or newline), as many names as reads, as many QUAL strings as reads, each as
    long as its read and of bytes '!'..'~'.  lens[c] is read c's length; names a sequence of str or bytes, None: r0, r1, ...; quals
    a [ns, n] uint8 array or a sequence of byte strings, None: no QUAL.  Returns (reference_name uint8, the names as one flat uint8
    array, its int64[ns + 1] offsets, the QUAL rows uint8[ns, max(lens)] or None).  Array operations only: no loop over the reads."""
    lens = np.asarray(lens, dtype=np.int64).reshape(-1)
    ns = int(lens.size)
    rname = _field_bytes(who, "reference_name", reference_name)
    if names is None:
        names = np.char.add("r", np.arange(ns).astype(str))
    try:
        texts = np.asarray(names)
        if texts.dtype.kind == "U":
            texts = np.char.encode(texts, "ascii")
    except (UnicodeError, ValueError) as exc:
        raise B.BgsaHipError(f"{who}: rc=-1: names must be ASCII strings or byte strings ({exc})") from None
    if texts.dtype.kind != "S" or texts.ndim != 1:
        raise B.BgsaHipError(f"{who}: rc=-1: names must be a sequence of ASCII strings or byte strings")
    if texts.shape[0] != ns:
        raise B.BgsaHipError(f"{who}: rc=-1: {texts.shape[0]} names for {ns} reads")
    name_lens = np.char.str_len(texts).astype(np.int64)
    if (name_lens == 0).any():
        raise B.BgsaHipError(f"{who}: rc=-1: the name of read {int(np.flatnonzero(name_lens == 0)[0])} is empty")
    letters = np.ascontiguousarray(texts).view(np.uint8).reshape(ns, -1)
    flat = letters[np.arange(letters.shape[1]) < name_lens[:, None]]
    bad = (flat < 33) | (flat > 126)
    if bad.any():
        at = int(np.repeat(np.arange(ns), name_lens)[bad][0])
        raise B.BgsaHipError(f"{who}: rc=-1: the name of read {at} holds a tab, a space, a newline or another byte outside '!'..'~'")
    offsets = np.zeros(ns + 1, dtype=np.int64)
    np.cumsum(name_lens, out=offsets[1:])
    rows = None
    if quals is not None:
        if isinstance(quals, np.ndarray) and quals.ndim == 2:
            rows = np.ascontiguousarray(quals, dtype=np.uint8)
            qual_lens = np.full(rows.shape[0], rows.shape[1], dtype=np.int64)
        else:
            if len(quals) != ns:
                raise B.BgsaHipError(f"{who}: rc=-1: {len(quals)} QUAL strings for {ns} reads")
            try:
                rows, qual_lens = B.pad_ragged(quals)
            except B.BgsaHipError as exc:
                raise B.BgsaHipError(f"{who}: rc=-1: quals: {exc}") from None
        if rows.shape[0] != ns:
            raise B.BgsaHipError(f"{who}: rc=-1: {rows.shape[0]} QUAL strings for {ns} reads")
        wrong = np.flatnonzero(np.asarray(qual_lens, dtype=np.int64) != lens)
        if wrong.size:
            c = int(wrong[0])
            raise B.BgsaHipError(f"{who}: rc=-1: the QUAL of read {c} has {int(qual_lens[c])} bytes, the read {int(lens[c])}")
        own = np.arange(rows.shape[1]) < lens[:, None]
        bad = own & ((rows < 33) | (rows > 126))
        if bad.any():
            raise B.BgsaHipError(f"{who}: rc=-1: the QUAL of read {int(np.flatnonzero(bad.any(axis=1))[0])} holds a byte outside '!'..'~'")
    return rname, flat, offsets, rows


def write_sam(path, header: bytes, records: SamRecords) -> None:
    """The header (ReferenceMapper.sam_header) and the records' text into the file `path`."""
    with open(path, "wb") as out:
        out.write(header)
        out.write(memoryview(np.ascontiguousarray(records.text)))


# ---- BAM records: include/bgsa_hip.h "BAM records" — the host side, no device, no library ---------------------------------------
class BamRecords(NamedTuple):
    """What ReferenceMapper.map_reads_bam and map_pairs_bam return: the records in BAM's layout inside BGZF blocks — of stored
    deflate, or deflated where the call said compress=True —, as the device wrote them, and SamRecords' four columns."""
    blocks: np.ndarray      # uint8: the framed BGZF blocks of this call's records, without the BAM header and without the EOF block
    offsets: np.ndarray     # int64[n + 1]: record i, its block_size included, is payload[offsets[i] : offsets[i + 1]] of the inflated blocks
    flag: np.ndarray        # int32[n]
    pos: np.ndarray         # int64[n]: POS, 1-based; 0 for an unmapped record without a mapped mate
    mapq: np.ndarray        # int32[n]
    nm: np.ndarray          # int32[n]: the distance, -1 for an unmapped record


BGZF_BLOCK_PAYLOAD = 0xff00       # 65,280: what every BGZF writer puts into a block; the format's own limit is 65,505
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")      # SAMv1 §4.1.2: the empty block that ends a file


def bgzf_blocks(data, block_payload: int = BGZF_BLOCK_PAYLOAD) -> bytes:
    """`data` in BGZF blocks of STORED deflate, block_payload bytes each (the last may be shorter; no data: no block), the framing
    bgsa_hip_bgzf_frame_dev writes on the device — here for the BAM header.  Without the EOF block."""
    if not 1 <= int(block_payload) <= BGZF_BLOCK_PAYLOAD:
        raise B.BgsaHipError(f"bgzf_blocks: rc=-1: block_payload {block_payload} outside 1..{BGZF_BLOCK_PAYLOAD}")
    data, out = bytes(data), []
    for at in range(0, len(data), int(block_payload)):
        piece = data[at: at + int(block_payload)]
        out.append(b"\x1f\x8b\x08\x04\x00\x00\x00\x00\x00\xff\x06\x00BC\x02\x00" + struct.pack("<HBHH", len(piece) + 30, 1, len(piece),
                                                                                               len(piece) ^ 0xffff))
        out.append(piece)
        out.append(struct.pack("<II", zlib.crc32(piece), len(piece)))
    return b"".join(out)


def bam_header_bytes(who: str, text: bytes, references) -> bytes:
    """The uncompressed BAM header: the magic, l_text and the SAM header text, n_ref, and l_name, the name + NUL and l_ref of every
    (name, length) of `references`.  A length beyond 2^31 - 1 is refused."""
    out = [b"BAM\x01", struct.pack("<i", len(text)), text, struct.pack("<i", len(references))]
    for name, n in references:
        if int(n) > 2 ** 31 - 1:
            raise B.BgsaHipError(f"{who}: rc=-1: {name.decode()} has {int(n)} bases, a BAM header holds 2^31 - 1 at the most")
        out += [struct.pack("<i", len(name) + 1), name, b"\x00", struct.pack("<i", int(n))]
    return b"".join(out)


def check_bam_call(who: str, lens, names, quals, reference_name, block_payload=BGZF_BLOCK_PAYLOAD, compress=False, sort=False,
                   ref_lens=()) -> tuple:
    """check_sam_call's refusals and returns, then BAM's own, before anything is launched or allocated: a name longer than 254
    bytes (l_read_name is one byte and counts the NUL), a block_payload outside 1..65,280, a compress or a sort that is not a
    bool, and with sort=True a reference or contig (ref_lens) longer than 2^29 bases: a BAI index reaches no further."""
    checked = check_sam_call(who, lens, names, quals, reference_name)
    name_lens = np.diff(checked[2])
    if (name_lens > 254).any():
        c = int(np.flatnonzero(name_lens > 254)[0])
        raise B.BgsaHipError(f"{who}: rc=-1: the name of read {c} has {int(name_lens[c])} bytes, a BAM record holds 254 at the most")
    if isinstance(block_payload, bool) or not isinstance(block_payload, (int, np.integer)) or not 1 <= int(block_payload) <= BGZF_BLOCK_PAYLOAD:
        raise B.BgsaHipError(f"{who}: rc=-1: block_payload {block_payload!r} outside 1..{BGZF_BLOCK_PAYLOAD}")
    if not isinstance(compress, (bool, np.bool_)):
        raise B.BgsaHipError(f"{who}: rc=-1: compress {compress!r} is not a bool")
    if not isinstance(sort, (bool, np.bool_)):
        raise B.BgsaHipError(f"{who}: rc=-1: sort {sort!r} is not a bool")
    if sort:
        for c, n in enumerate(np.asarray(ref_lens, dtype=np.int64).reshape(-1).tolist()):
            if n > BAI_REACH:
                raise B.BgsaHipError(f"{who}: rc=-1: sort=True: reference {c} has {n} bases, a BAI index reaches 2^29 = {BAI_REACH}")
    return checked


def check_coordinate_header(who: str, header: bytes) -> None:
    """The refusal of an uncompressed BAM header whose @HD line does not say SO:coordinate: an indexed file is a sorted one."""
    text = bytes(header)[8: 8 + max(struct.unpack_from("<i", bytes(header), 4)[0], 0)] if len(header) >= 8 else b""
    if b"SO:coordinate" not in text.split(b"\n")[0]:
        raise B.BgsaHipError(f"{who} the header's @HD line does not say SO:coordinate (bam_header(sort_order=\"coordinate\"))")


def write_bam(path, header: bytes, records, index: bool = False) -> None:
    """A BAM file: the header (ReferenceMapper.bam_header, uncompressed) framed by bgzf_blocks, the blocks of `records` — one
    BamRecords or a sequence of them, in order: batches of reads stream into one file —, then BGZF_EOF.  index=True: `records` is
    ONE SortedBamRecords (a sorted file holds one call's records) and the header says SO:coordinate; the BAI index goes to
    path + ".bai" (bai_bytes, its offsets moved behind the framed header)."""
    framed = bgzf_blocks(header)
    if index:
        if not isinstance(records, SortedBamRecords):
            raise B.BgsaHipError("write_bam: rc=-1: index=True takes ONE SortedBamRecords (map_reads_bam / map_pairs_bam with sort=True)")
        check_coordinate_header("write_bam: rc=-1: index=True, and", header)
    batches = [records] if isinstance(records, (BamRecords, SortedBamRecords)) else list(records)
    with open(path, "wb") as out:
        out.write(framed)
        for batch in batches:
            out.write(memoryview(np.ascontiguousarray(batch.blocks)))
        out.write(BGZF_EOF)
    if index:
        with open(str(path) + ".bai", "wb") as out:
            out.write(bai_bytes(records.index, records.flag, records.ref_id, len(framed)))


# ---- BAM records: coordinate order and index: include/bgsa_hip.h — the host side, no device, no library --------------------------
BAI_REACH = 1 << 29               # what a BAI's bins and 16 Kbp windows cover
BAI_WINDOW_SHIFT = 14
BAI_META_BIN = 37450
SORT_ORDERS = ("unsorted", "coordinate")


# ---- duplicate marking: include/bgsa_hip.h "Duplicate marking" — the host side, no device, no library ---------------------------
DUPLICATE_FLAG = 0x400
DUPLICATE_MIN_QUALITY = 15        # Picard's SUM_OF_BASE_QUALITIES counts the bases of quality 15 and above
DUPLICATE_STATS = ("pair_units", "fragment_units", "records_skipped", "duplicate_pair_units", "duplicate_fragment_units", "records_flagged")


def check_mark_duplicates(who: str, mark_duplicates) -> bool:
    """The refusal of a mark_duplicates that is not a bool, in sort's wording; before anything is launched."""
    if not isinstance(mark_duplicates, (bool, np.bool_)):
        raise B.BgsaHipError(f"{who}: rc=-1: mark_duplicates {mark_duplicates!r} is not a bool")
    return bool(mark_duplicates)


class BamIndex(NamedTuple):
    """The arrays of a BAI index as the device built them for ONE call's sorted records; offsets are virtual offsets relative to
    the first byte of the call's blocks."""
    ref_lens: np.ndarray      # int64[n_ref]
    chunk_ref: np.ndarray     # int32[n_chunks]: the chunks in (ref, bin, beg) order
    chunk_bin: np.ndarray     # int32[n_chunks]
    chunk_beg: np.ndarray     # int64[n_chunks]
    chunk_end: np.ndarray     # int64[n_chunks]
    window_base: np.ndarray   # int64[n_ref + 1]: reference c owns linear[window_base[c] : window_base[c + 1]]
    linear: np.ndarray        # int64: the suffix minimum of the windows' smallest offsets; INT64_MAX behind the last record
    n_intv: np.ndarray        # int64[n_ref]: the windows of reference c a .bai writes


class SortedBamRecords(NamedTuple):
    """What map_reads_bam and map_pairs_bam return with sort=True: BamRecords' six fields in OUTPUT (coordinate) order, then the
    refID column, the permutation and the index."""
    blocks: np.ndarray
    offsets: np.ndarray
    flag: np.ndarray
    pos: np.ndarray
    mapq: np.ndarray
    nm: np.ndarray
    ref_id: np.ndarray        # int32[n]: -1 for a record without coordinates
    order: np.ndarray         # int64[n]: output record i is input record order[i]
    index: BamIndex


def sort_order_line(who: str, sort_order) -> bytes:
    """The @HD line for sort_order "unsorted" or "coordinate"; anything else is refused."""
    if not isinstance(sort_order, str) or sort_order not in SORT_ORDERS:
        raise B.BgsaHipError(f"{who}: rc=-1: sort_order {sort_order!r} is neither 'unsorted' nor 'coordinate'")
    return b"@HD\tVN:1.6\tSO:" + sort_order.encode() + b"\n"


def bai_bytes(index: BamIndex, flag, ref_id, base: int = 0) -> bytes:
    """The .bai file (SAMv1 §5.2) of `index` and the sorted records' flag and ref_id columns, every offset moved by base << 16
    (base: the bytes in front of the call's blocks in the file, the framed header).  Per reference its bins ascending — bin,
    n_chunk, the chunks —, the metadata pseudo-bin 37450 last — (smallest begin, largest end), (mapped, unmapped) —, n_intv and the
    linear offsets; n_no_coor at the end.  A reference without records: n_bin 0 and n_intv 0.  Host only."""
    flag, ref_id = np.asarray(flag).reshape(-1), np.asarray(ref_id).reshape(-1)
    shift = int(base) << 16
    n_ref = int(np.asarray(index.ref_lens).size)
    chunk_ref = np.asarray(index.chunk_ref)
    first = np.searchsorted(chunk_ref, np.arange(n_ref + 1))       # the chunks are in (ref, bin, beg) order
    out = [b"BAI\x01", struct.pack("<i", n_ref)]
    for c in range(n_ref):
        lo, hi = int(first[c]), int(first[c + 1])
        if hi == lo:
            out.append(struct.pack("<ii", 0, 0))
            continue
        bins = np.asarray(index.chunk_bin[lo:hi])
        cuts = np.concatenate(([0], np.flatnonzero(np.diff(bins)) + 1, [hi - lo]))
        out.append(struct.pack("<i", cuts.size))                  # the bins and the pseudo-bin
        pairs = np.stack((index.chunk_beg[lo:hi], index.chunk_end[lo:hi]), axis=1).astype(np.uint64) + np.uint64(shift)
        for a, b in zip(cuts[:-1].tolist(), cuts[1:].tolist()):
            out += [struct.pack("<Ii", int(bins[a]), b - a), pairs[a:b].astype("<u8").tobytes()]
        own = ref_id == c
        unmapped = int((own & ((flag & 4) != 0)).sum())
        out.append(struct.pack("<Ii4Q", BAI_META_BIN, 2, int(index.chunk_beg[lo:hi].min()) + shift, int(index.chunk_end[lo:hi].max()) + shift,
                               int(own.sum()) - unmapped, unmapped))
        n_intv = int(index.n_intv[c])
        at = int(index.window_base[c])
        out += [struct.pack("<i", n_intv), (np.asarray(index.linear[at: at + n_intv]).astype(np.uint64) + np.uint64(shift)).astype("<u8").tobytes()]
    out.append(struct.pack("<Q", int((ref_id < 0).sum())))
    return b"".join(out)


# ---- BAM records: merge: include/bgsa_hip.h "BAM records: merge" ------------------------------------------------------------------
MERGE_COLUMNS = ("lengths", "key", "ref_id", "pos", "end", "bin", "flag", "POS", "mapq", "nm")      # per record, in input order
MERGE_DUPLICATE_COLUMNS = ("end_key", "score", "key_a", "key_b")                                    # per record, per unit x 3


def check_bam_merge(who: str, block_payload=BGZF_BLOCK_PAYLOAD, compress=False, mark_duplicates=False, segment_blocks=4096, reserve_bytes=None,
                    ref_lens=()) -> None:
    """What a merge refuses before anything is launched or allocated, pure host: a compress or mark_duplicates that is not a bool,
    a block_payload outside 1..65,280, a segment_blocks that is not an int >= 1, a reserve_bytes that is not None or an int >= 0,
    a reference or contig (ref_lens) beyond 2^29 bases."""
    def is_int(x):
        return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))
    if not isinstance(compress, (bool, np.bool_)):
        raise B.BgsaHipError(f"{who}: rc=-1: compress {compress!r} is not a bool")
    check_mark_duplicates(who, mark_duplicates)
    if not is_int(block_payload) or not 1 <= int(block_payload) <= BGZF_BLOCK_PAYLOAD:
        raise B.BgsaHipError(f"{who}: rc=-1: block_payload {block_payload!r} outside 1..{BGZF_BLOCK_PAYLOAD}")
    if not is_int(segment_blocks) or int(segment_blocks) < 1:
        raise B.BgsaHipError(f"{who}: rc=-1: segment_blocks {segment_blocks!r} is not an int >= 1")
    if reserve_bytes is not None and (not is_int(reserve_bytes) or int(reserve_bytes) < 0):
        raise B.BgsaHipError(f"{who}: rc=-1: reserve_bytes {reserve_bytes!r} is neither None nor an int >= 0")
    for c, n in enumerate(np.asarray(ref_lens, dtype=np.int64).reshape(-1).tolist()):
        if n > BAI_REACH:
            raise B.BgsaHipError(f"{who}: rc=-1: reference {c} has {n} bases, a BAI index reaches 2^29 = {BAI_REACH}")


def check_bam_merge_add(who: str, merge, mapper, ends: int, block_payload=BGZF_BLOCK_PAYLOAD, compress=False, sort=False,
                        mark_duplicates=False) -> None:
    """What a call with merge= refuses before anything is launched, pure host: a merge that is no BamMerge, or another mapper's, or
    finished; a batch of the other kind (a merge has one `ends`: 1 single-end, 2 paired); a sort, compress, block_payload or
    mark_duplicates beside the merge — they belong to the merge and stay at their defaults in the call."""
    if not isinstance(merge, BamMerge):
        raise B.BgsaHipError(f"{who}: rc=-1: merge {merge!r} is not a BamMerge (mapper.bam_merge())")
    given = [name for name, value, default in (("sort", sort, False), ("compress", compress, False), ("block_payload", block_payload, BGZF_BLOCK_PAYLOAD),
                                               ("mark_duplicates", mark_duplicates, False)) if value is not default and value != default]
    if given:
        raise B.BgsaHipError(f"{who}: rc=-1: {', '.join(given)} beside merge=: they belong to the merge (mapper.bam_merge(...))")
    if merge.mapper is not mapper:
        raise B.BgsaHipError(f"{who}: rc=-1: the merge belongs to another mapper")
    if merge.finished:
        raise B.BgsaHipError(f"{who}: rc=-1: the merge is finished")
    if merge.ends not in (None, ends):
        kinds = {1: "single-end", 2: "paired"}
        raise B.BgsaHipError(f"{who}: rc=-1: a {kinds[ends]} batch into a merge of {kinds[merge.ends]} ones: a merge has one `ends`")


class BamMerge:
    """The BAM records of any number of map_reads_bam / map_pairs_bam calls (merge=this), kept on the device as every call emitted
    them — in input order, batch after batch —, and finished into ONE coordinate-sorted, indexed result: finish() returns the
    SortedBamRecords of one sort=True call on the concatenated reads, write() streams the same bytes to a .bam and its .bai
    (include/bgsa_hip.h "BAM records: merge").  Made by mapper.bam_merge(); nothing is allocated before the
    first batch."""

    def __init__(self, mapper, block_payload: int = BGZF_BLOCK_PAYLOAD, compress: bool = False, mark_duplicates: bool = False,
                 segment_blocks: int = 4096, reserve_bytes=None):
        check_bam_merge("bam_merge", block_payload, compress, mark_duplicates, segment_blocks, reserve_bytes, mapper.index_ref_lens())
        self.mapper, self.block_payload, self.compress = mapper, int(block_payload), bool(compress)
        self.mark_duplicates, self.segment_blocks = bool(mark_duplicates), int(segment_blocks)
        self.reserve_bytes = None if reserve_bytes is None else int(reserve_bytes)
        self.ends, self.finished = None, False
        self.n, self.payload_bytes, self.payload = 0, 0, None      # records, their bytes, the device buffer that holds them
        self.columns = {name: [] for name in MERGE_COLUMNS + MERGE_DUPLICATE_COLUMNS}
        self.key_counts = [0, 0, 0]                                # pair units, fragment units, skipped records: the key kernel's

    def _append(self, ends: int, payload, payload_bytes: int, columns: dict, key_counts=None) -> int:
        """One accepted batch: its emitted payload (a device tensor, payload_bytes of it) behind the others', its per-record device
        tensors (MERGE_COLUMNS, and MERGE_DUPLICATE_COLUMNS with the key kernel's three counters where the merge marks
        duplicates) kept as they are.  Called after the batch's last check; the number of records added."""
        torch = self.mapper.aligner.torch
        need = self.payload_bytes + payload_bytes
        if self.payload is None or need > self.payload.numel():
            room = max(need, 1, self.reserve_bytes or 0) if self.payload is None else max(need, 2 * self.payload.numel())
            grown = torch.empty(room, dtype=torch.uint8, device=self.mapper.aligner.device)
            if self.payload_bytes:
                grown[: self.payload_bytes] = self.payload[: self.payload_bytes]
            self.payload = grown
        self.payload[self.payload_bytes: need] = payload[:payload_bytes]
        n = int(columns["lengths"].shape[0])
        for name, value in columns.items():
            self.columns[name].append(value)
        if key_counts is not None:
            self.key_counts = [a + b for a, b in zip(self.key_counts, key_counts)]
        self.ends, self.n, self.payload_bytes = ends, self.n + n, need
        return n

    def _column(self, name: str, dtype):
        """A column of all batches, batch after batch."""
        torch, dev = self.mapper.aligner.torch, self.mapper.aligner.device
        parts = self.columns[name]
        return torch.cat(parts).contiguous() if parts else torch.empty(0, dtype=dtype, device=dev)

    def _empty_index(self) -> BamIndex:
        """The index of no record: no chunk, no window filled (the index calls take no empty array)."""
        ref_lens = self.mapper.index_ref_lens()
        window_base = np.zeros(ref_lens.size + 1, dtype=np.int64)
        windows = int(B.lib().bgsa_hip_bam_index_windows(ref_lens.ctypes.data, ref_lens.size, window_base.ctypes.data))
        none = [np.zeros(0, dtype=dtype) for dtype in (np.int32, np.int32, np.int64, np.int64)]
        return BamIndex(ref_lens, *none, window_base, np.full(windows, np.iinfo(np.int64).max, dtype=np.int64), np.zeros(ref_lens.size, dtype=np.int64))

    def _finish(self, who: str, on_blocks) -> tuple:
        """The steps of finish and write: one stable sort of all keys, duplicate marking over all records, the scan of the sorted
        lengths, then per segment of segment_blocks blocks gather -> frame or deflate and pack -> one copy, handed to
        on_blocks(numpy bytes); the index at the end.  Everything of SortedBamRecords but the blocks."""
        m, L = self.mapper, B.lib()
        a = m.aligner
        torch, dev, n, total, P = a.torch, a.device, self.n, self.payload_bytes, self.block_payload
        self.finished = True
        order = m.sort_permutation(self._column("key", torch.int64)).contiguous()
        flag = self._column("flag", torch.int32).clone()
        if self.mark_duplicates:
            counts = torch.zeros(6, dtype=torch.int32, device=dev)
            score = self._column("score", torch.int32)
            if n and self.ends == 2:
                by, keys = m.duplicate_order(score, self._column("key_a", torch.int64), self._column("key_b", torch.int64))
                m.duplicate_marks(keys, by, n, 2, flag, counts[3:])
            if n:
                by, keys = m.duplicate_order(score.repeat_interleave(self.ends), self._column("end_key", torch.int64))
                m.duplicate_marks(keys, by, n, 1, flag, counts[3:])
            m.last_duplicate_stats = dict(zip(DUPLICATE_STATS, self.key_counts + counts[3:].tolist()))
        src_offsets, dst_offsets = (torch.zeros(n + 1, dtype=torch.int64, device=dev) for _ in range(2))
        lengths = self._column("lengths", torch.int64)
        src_offsets[1:] = torch.cumsum(lengths, 0)
        dst_offsets[1:] = torch.cumsum(lengths[order], 0)
        span = self.segment_blocks * P
        lo = torch.arange(0, total, span, dtype=torch.int64, device=dev)
        first = torch.searchsorted(dst_offsets[1:].contiguous(), lo, right=True)                  # the first record that ends behind lo
        behind = torch.searchsorted(dst_offsets[:-1].contiguous(), (lo + span).clamp(max=total))      # the records that start before hi
        plan = torch.stack((lo, first, behind - first), dim=1).cpu().tolist()                    # one copy: every segment's records
        segment = torch.empty(max(min(span, total), 1), dtype=torch.uint8, device=dev)
        refused = torch.zeros(1, dtype=torch.int32, device=dev)
        block_offsets, base = [], 0
        for at, head, count in plan:
            size = min(span, total - at)
            B.check(L.bgsa_hip_bam_gather_dev(self.payload.data_ptr(), total, src_offsets.data_ptr(), n, order.data_ptr(), dst_offsets.data_ptr(),
                                              n, head, count, at, at + size, flag.data_ptr(), segment.data_ptr(), refused.data_ptr(),
                                              a._stream()), "bam_gather_dev")
            if self.compress:
                blocks, framed, offsets = m.bgzf_deflated(who, segment, size, P, with_offsets=True)
                block_offsets.append(offsets[:-1] + base)
            else:
                framed = int(L.bgsa_hip_bgzf_framed_bytes(size, P))
                blocks = torch.empty(framed, dtype=torch.uint8, device=dev)
                B.check(L.bgsa_hip_bgzf_frame_dev(segment.data_ptr(), size, P, blocks.data_ptr(), framed, a._stream()), "bgzf_frame_dev")
            host = blocks[:framed].cpu().numpy()
            if int(refused.item()):
                raise B.BgsaHipError(f"{who}: the gather pass refused {int(refused.item())} records: an order, offsets or lengths that do "
                                     f"not describe the merged payload")
            on_blocks(host)
            base += framed
        if self.compress:
            block_offsets = torch.cat(block_offsets + [torch.full((1,), base, dtype=torch.int64, device=dev)]).contiguous()
        coordinates = [self._column(name, torch.int32) for name in ("ref_id", "pos", "end", "bin")]
        coordinates = [x[order].contiguous() for x in coordinates]
        index = m.bam_index(who, *coordinates, dst_offsets, total, P, block_offsets if self.compress else None) if n else self._empty_index()
        column = lambda name, dtype: self._column(name, dtype)[order].cpu().numpy()      # noqa: E731
        return (dst_offsets.cpu().numpy(), flag[order].cpu().numpy(), m.local_pos(column("POS", torch.int64)), column("mapq", torch.int32),
                column("nm", torch.int32), coordinates[0].cpu().numpy(), order.cpu().numpy(), index)

    def finish(self) -> SortedBamRecords:
        """All records in coordinate order with their index: what ONE map_reads_bam / map_pairs_bam call with sort=True (and this
        merge's compress, block_payload and mark_duplicates) returns for the concatenated reads; `order` holds global input
        indices, batch after batch.  With mark_duplicates the mapper's last_duplicate_stats is filled.  No batch can follow."""
        pieces = []
        rest = self._finish("bam_merge.finish", pieces.append)
        return SortedBamRecords(np.concatenate(pieces) if pieces else np.zeros(0, dtype=np.uint8), *rest)

    def write(self, path, header: bytes) -> None:
        """The file write_bam(path, header, self.finish(), index=True) writes, every segment's blocks streamed as they arrive: the
        framed header, the blocks, BGZF_EOF, then path + ".bai".  A header without SO:coordinate is refused first."""
        check_coordinate_header("bam_merge.write: rc=-1:", header)
        framed = bgzf_blocks(header)
        with open(path, "wb") as out:
            out.write(framed)
            _, flag, _, _, _, ref_id, _, index = self._finish("bam_merge.write", lambda blocks: out.write(memoryview(blocks)))
            out.write(BGZF_EOF)
        with open(str(path) + ".bai", "wb") as out:
            out.write(bai_bytes(index, flag, ref_id, len(framed)))


# ---- Pileup: include/bgsa_hip.h "Pileup" ---------------------------------------------------------------------------------------------
PILEUP_COLUMNS = ("A", "C", "G", "T", "other", "deleted", "inserted", "reverse")      # the count matrix's eight columns, fixed
PILEUP_STATS = ("records_used", "records_filtered", "records_malformed", "bases_counted", "bases_low_quality")
PILEUP_EXCLUDE_FLAGS = 0x704      # unmapped, secondary, QC fail, duplicate


def _is_int(x) -> bool:
    return isinstance(x, (int, np.integer)) and not isinstance(x, (bool, np.bool_))


def check_pileup(who: str, min_mapq=0, min_base_quality=13, exclude_flags=PILEUP_EXCLUDE_FLAGS) -> tuple:
    """What mapper.pileup refuses before anything is allocated, pure host: a min_mapq that is no int in 0..255, a min_base_quality
    outside 0..93, exclude_flags outside 0..65535.  Returns the three as ints."""
    for name, value, top in (("min_mapq", min_mapq, 255), ("min_base_quality", min_base_quality, 93), ("exclude_flags", exclude_flags, 65535)):
        if not _is_int(value) or not 0 <= int(value) <= top:
            raise B.BgsaHipError(f"{who}: rc=-1: {name} {value!r} is not an int in 0..{top}")
    return int(min_mapq), int(min_base_quality), int(exclude_flags)


def check_pileup_sites(who: str, min_cover=8, min_alt=3, min_percent=20) -> tuple:
    """What Pileup.sites refuses before anything is launched: a min_cover or min_alt that is no int >= 1 (and below 2^31), a
    min_percent that is no int in 0..100.  Returns the three as ints."""
    for name, value, low, top in (("min_cover", min_cover, 1, 2 ** 31 - 1), ("min_alt", min_alt, 1, 2 ** 31 - 1), ("min_percent", min_percent, 0, 100)):
        if not _is_int(value) or not low <= int(value) <= top:
            raise B.BgsaHipError(f"{who}: rc=-1: {name} {value!r} is not an int in {low}..{top}")
    return int(min_cover), int(min_alt), int(min_percent)


def check_pileup_add(who: str, pileup, mapper, merge=None) -> None:
    """What a call with pileup= refuses before anything is launched, pure host: a pileup that is no Pileup, or another mapper's;
    a merge= beside it that marks duplicates — that merge learns its duplicate flags only at finish(), the pileup could not
    honour them."""
    if not isinstance(pileup, Pileup):
        raise B.BgsaHipError(f"{who}: rc=-1: pileup {pileup!r} is not a Pileup (mapper.pileup())")
    if pileup.mapper is not mapper:
        raise B.BgsaHipError(f"{who}: rc=-1: the pileup belongs to another mapper")
    if merge is not None and getattr(merge, "mark_duplicates", False):
        raise B.BgsaHipError(f"{who}: rc=-1: pileup= beside a merge with mark_duplicates=True: the merge flags its duplicates at finish(), "
                             f"after this call's records were counted")


class PileupSites(NamedTuple):
    """The candidate sites of a Pileup, in ascending (linear) position: numpy arrays of one length.  ref is the reference's code
    0..3, alt the qualifying column of the highest count (0..3 a base, 5 a deletion, 6 an insertion behind pos), alts_mask bit a
    for every qualifying column a.  On a ContigMapper pos is local to contig; elsewhere contig is None."""
    pos: np.ndarray         # int64
    ref: np.ndarray         # uint8
    alt: np.ndarray         # uint8
    alt_count: np.ndarray   # int32
    cover: np.ndarray       # int32: columns 0..5 summed
    alts_mask: np.ndarray   # uint8
    contig: object = None   # int32 on a ContigMapper


class Pileup:
    """Per-position base counts of the records of any number of map_reads_* / map_pairs_* calls (pileup=this), on the device:
    counts [ref_len, 8] int32 in LINEAR coordinates, the columns PILEUP_COLUMNS, and the five counters of PILEUP_STATS
    (include/bgsa_hip.h "Pileup").  A record contributes when it is mapped, carries none of exclude_flags —
    the default leaves out secondary, QC-fail and duplicate records — and has mapq >= min_mapq; a base with QUAL below
    min_base_quality is not counted (no QUAL: every base is).  Made by mapper.pileup().
    LIMITS: the mates of an overlapping pair are both counted; duplicates are only those marked within the call
    (mark_duplicates=True), never across calls; no base-alignment quality, no genotype likelihoods, no VCF; insertions are counted
    per run, not per inserted sequence."""

    def __init__(self, mapper, min_mapq: int = 0, min_base_quality: int = 13, exclude_flags: int = PILEUP_EXCLUDE_FLAGS):
        self.min_mapq, self.min_base_quality, self.exclude_flags = check_pileup("pileup", min_mapq, min_base_quality, exclude_flags)
        a = mapper.aligner
        self.mapper = mapper
        self.counts = a.torch.zeros((mapper.ref_len, len(PILEUP_COLUMNS)), dtype=a.torch.int32, device=a.device)
        self._stats = a.torch.zeros(len(PILEUP_STATS), dtype=a.torch.int64, device=a.device)

    def _add(self, batch, n: int) -> None:
        """The counts kernel on a bgsa_hip_sam_batch_t of n records.  Called after the call's last check."""
        B.check(B.lib().bgsa_hip_pileup_dev(batch, n, self.min_mapq, self.min_base_quality, self.exclude_flags, self.counts.data_ptr(),
                                            self._stats.data_ptr(), self.mapper.aligner._stream()), "pileup_dev")

    def stats(self) -> dict:
        """The five counters, in one small copy."""
        return dict(zip(PILEUP_STATS, self._stats.tolist()))

    def depth(self):
        """Columns 0..5 summed: the device tensor int32[ref_len] of the records that cover every position."""
        torch = self.mapper.aligner.torch
        return self.counts[:, :6].sum(dim=1, dtype=torch.int32)

    def counts_host(self, begin: int = 0, end=None) -> np.ndarray:
        """Rows [begin, end) of counts (linear positions) on the host."""
        return self.counts[int(begin): self.mapper.ref_len if end is None else int(end)].cpu().numpy()

    def reset(self) -> None:
        self.counts.zero_()
        self._stats.zero_()

    def sites(self, min_cover: int = 8, min_alt: int = 3, min_percent: int = 20) -> PileupSites:
        """The candidate sites, reduced on the device: a position whose reference base is A, C, G or T, whose cover (columns 0..5)
        is >= min_cover and where a column other than the reference's — a base, the deletions, the insertions — holds >= min_alt
        and >= min_percent % of the cover (integers).  The count pass, a scan of the workgroups' counts, ONE scalar read back, the
        emit pass, one copy per array; the count matrix stays on the device."""
        min_cover, min_alt, min_percent = check_pileup_sites("pileup.sites", min_cover, min_alt, min_percent)
        m, L = self.mapper, B.lib()
        a = m.aligner
        torch, dev = a.torch, a.device
        n_blocks = int(L.bgsa_hip_pileup_site_blocks(m.ref_len))
        block_sites = torch.empty(n_blocks, dtype=torch.int32, device=dev)
        test = (self.counts.data_ptr(), m.d_reference.data_ptr(), m.ref_len, min_cover, min_alt, min_percent)
        B.check(L.bgsa_hip_pileup_sites_count_dev(*test, block_sites.data_ptr(), n_blocks, a._stream()), "pileup_sites_count_dev")
        ends = torch.cumsum(block_sites, 0, dtype=torch.int64)
        total = int(ends[-1].item())                    # the one scalar read back: it sizes the outputs
        block_offsets = (ends - block_sites).contiguous()
        pos = torch.empty(max(total, 1), dtype=torch.int64, device=dev)
        ref, alt, mask = (torch.empty(max(total, 1), dtype=torch.uint8, device=dev) for _ in range(3))
        alt_count, cover = (torch.empty(max(total, 1), dtype=torch.int32, device=dev) for _ in range(2))
        overflow = torch.zeros(1, dtype=torch.int32, device=dev)
        B.check(L.bgsa_hip_pileup_sites_emit_dev(*test, block_offsets.data_ptr(), n_blocks, total, pos.data_ptr(), ref.data_ptr(), alt.data_ptr(),
                                                 mask.data_ptr(), alt_count.data_ptr(), cover.data_ptr(), overflow.data_ptr(), a._stream()),
                "pileup_sites_emit_dev")
        if int(overflow.item()):
            raise B.BgsaHipError(f"pileup.sites: the emit pass found {int(overflow.item())} sites beyond the {total} the count pass found")
        local, contig = m.local_sites(pos[:total].cpu().numpy())
        return PileupSites(local, ref[:total].cpu().numpy(), alt[:total].cpu().numpy(), alt_count[:total].cpu().numpy(),
                           cover[:total].cpu().numpy(), mask[:total].cpu().numpy(), contig)


class SeedBucket(NamedTuple):
    """What the steps of select_seeded share for one resident bucket (ReferenceMapper.seed_bucket)."""
    d_rows: object          # the bucket's ASCII rows on the device, read_len + 1 bytes each
    read_len: int           # the rows' width
    bound: int
    shape: tuple            # the leading arguments of the candidate calls: the geometry, the index, the seed length
    count: object           # the three C calls: the equal-length ones, or the *_lens_dev ones
    emit: object
    verify: object
    lens_of: object         # lens_of(lo, hi): the extra argument of count and emit for the reads [lo, hi): () or (pointer,)
    lens_all: tuple         # the extra argument of verify: () or (the bucket's lengths,)


class ReferenceMapper:
    """One reference, resident on the device as mapped codes, and a Myers semi-global aligner over its windows.

    reference: bytes, str or a 1-D uint8 array of ASCII bases (a '\\n' in it raises: it is one sequence, not a file).  It is
    uploaded and mapped once; the windows of window_len every stride bases exist only as query rows built on the device, a
    segment of segment_windows ids at a time.  both_strands=False leaves the reverse-complemented windows out.

    Limits: one read length per map_reads call (map_reads_ragged takes reads of mixed lengths up to 1,024 bp), Myers unit-cost
    distance, one GPU.  The r-th distinct locus of a read is reported if its best window is among the read's k_sel best
    windows; for k_best = 1 that always holds."""

    def __init__(self, reference, window_len: int, stride: int, device: str = "cuda:0", both_strands: bool = True,
                 segment_windows: int = 65536):
        if isinstance(reference, str):
            reference = reference.encode("ascii")
        if isinstance(reference, (bytes, bytearray, memoryview)):
            ref = np.frombuffer(reference, dtype=np.uint8)
        else:
            ref = np.ascontiguousarray(reference, dtype=np.uint8)
        if ref.ndim != 1:
            raise B.BgsaHipError("ReferenceMapper: rc=-1: the reference is one sequence (1-D)")
        if (ref == ord("\n")).any():
            raise B.BgsaHipError("ReferenceMapper: rc=-1: the reference holds a newline: pass the bases of ONE sequence, not a file's lines")
        self.ref_len, self.window_len, self.stride = int(ref.size), int(window_len), int(stride)
        self.n_windows, self.starts = window_plan(self.ref_len, self.window_len, self.stride)
        if 2 * self.n_windows > INT32_MAX:
            raise B.BgsaHipError(f"ReferenceMapper: rc=-1: {self.n_windows} windows on two strands do not fit int32 window ids")
        self.both_strands = bool(both_strands)
        self.n_ids = self.n_windows * (2 if self.both_strands else 1)
        self.segment_windows = int(segment_windows)
        if self.segment_windows < 1:
            raise B.BgsaHipError("ReferenceMapper: rc=-1: segment_windows is not positive")
        self.aligner = a = B.DeviceAligner(B.ALGO_MYERS, device, semi_global=True)
        torch = a.torch
        self.d_reference = torch.zeros(self.ref_len + 8, dtype=torch.uint8, device=a.device)
        self.d_reference[: self.ref_len].copy_(torch.from_numpy(ref))
        B.check(B.lib().bgsa_hip_map_queries_dev(self.d_reference.data_ptr(), self.ref_len, a._stream()), "map_queries")
        self.d_rows = None      # the query rows of one segment / of one block's hit windows, grown on demand
        self.seed_indexes = {}  # seed_len -> (offsets, positions) device tensors (map_reads_seeded builds them on first use)
        self.d_verify_work = None   # the carries of a verify beyond 16 words, grown on demand
        self.last_seed_stats = None
        self.last_pair_stats = None
        self.last_duplicate_stats = None    # of the last SAM / BAM call with mark_duplicates=True

    def _rows_buffer(self, n_rows: int):
        need = n_rows * (self.window_len + 1) + 8
        if self.d_rows is None or self.d_rows.numel() < need:
            self.d_rows = self.aligner.torch.zeros(need, dtype=self.aligner.torch.uint8, device=self.aligner.device)
        return self.d_rows

    def _build_rows(self, d_ids, first_id: int, n_rows: int):
        """n_rows window rows as the aligner's query set: the ids first_id + r (d_ids None), or d_ids[r]."""
        a = self.aligner
        rows = self._rows_buffer(n_rows)
        B.check(B.lib().bgsa_hip_reference_windows_dev(self.d_reference.data_ptr(), self.ref_len, self.window_len, self.stride,
                                                       None if d_ids is None else d_ids.data_ptr(), int(first_id), n_rows,
                                                       rows.data_ptr(), a._stream()), "reference_windows_dev")
        a.set_query_rows_device(rows, n_rows, self.window_len)

    def k_selected(self, k_best: int) -> int:
        """Windows selected per read for k_best loci: a locus shows in up to ceil(W / S) overlapping windows, and one more
        holds a clipped copy at an edge."""
        return min(B.V_NUM, int(k_best) * (-(-self.window_len // self.stride) + 1))

    def select_windows(self, k_sel: int, block_rows: int = 1000):
        """The device half of map_reads' selection, for the reads the aligner holds (aligner.set_subjects(reads, qlen=window_len)):
        the ids in segments, every segment's rows built straight into the aligner's content buffer and joined to the lists by
        top_queries.  Returns device tensors (scores[ns, k_sel] int32, window ids[ns, k_sel] int32)."""
        a = self.aligner
        segment = min(self.segment_windows, self.n_ids)
        into = None
        for lo in range(0, self.n_ids, segment):
            self._build_rows(None, lo, min(segment, self.n_ids - lo))
            into = a.top_queries(k_sel, block_rows=block_rows, query_base=lo, into=into)
        return into

    def place_hits(self, ids, max_distance, cap: int, block_rows: int = 1000, ragged: bool = False):
        """The device half of map_reads' placement: block_rows reads at a time, the hit windows ids[ns, k_sel] gathered by id,
        placed within max_distance and turned into reference coordinates.  Returns device tensors (strand, ref_begin, ref_end,
        keep, n_ops — all [ns, k_sel] —, cigar[ns, k_sel, cap]).
        ragged (the aligner holds a bucket of set_reads_ragged, which place_pairs_banded refuses): the hits are traced with
        trace_pairs, every read at its own length, and a hit beyond max_distance (None: no bound) is then marked as
        place_pairs_banded leaves it — q_begin -1, n_ops 0 — so that it is reported unplaced."""
        a, L = self.aligner, B.lib()
        torch, dev, W = a.torch, a.device, self.window_len
        ns, k_sel = ids.shape
        span = torch.full((ns, k_sel, 4), -1, dtype=torch.int32, device=dev)
        distance = torch.full((ns, k_sel), -1, dtype=torch.int32, device=dev)
        n_ops = torch.zeros((ns, k_sel), dtype=torch.int32, device=dev)
        cigar = torch.zeros((ns, k_sel, cap), dtype=torch.int32, device=dev)
        strand = torch.empty((ns, k_sel), dtype=torch.int32, device=dev)
        ref_begin = torch.empty((ns, k_sel), dtype=torch.int64, device=dev)
        ref_end = torch.empty((ns, k_sel), dtype=torch.int64, device=dev)
        keep = torch.empty((ns, k_sel), dtype=torch.int32, device=dev)
        block = max(1, min(int(block_rows), ns))
        for lo in range(0, ns, block):
            hi = min(lo + block, ns)
            hit = ids[lo:hi]
            n_rows = (hi - lo) * k_sel
            self._build_rows(hit, 0, n_rows)
            pair_queries = torch.arange(n_rows, dtype=torch.int32, device=dev)
            columns = torch.arange(lo, hi, dtype=torch.int64, device=dev).repeat_interleave(k_sel)
            pair_subjects = torch.where(hit.reshape(-1) >= 0, columns, torch.full_like(columns, -1))
            into = (distance[lo:hi].view(-1), span[lo:hi].view(-1, 4), n_ops[lo:hi].view(-1), cigar[lo:hi].view(-1, cap))
            if ragged:
                distance[lo:hi] = 0    # trace_pairs reports scores: minus the distance, 0 where nobody owns the pair
                a.trace_pairs(pair_queries, pair_subjects, cigar_cap=cap, into=into)
                if max_distance is not None:
                    beyond = -distance[lo:hi] > int(max_distance)
                    span[lo:hi, :, 0].masked_fill_(beyond, -1)
                    n_ops[lo:hi].masked_fill_(beyond, 0)
            else:
                a.place_pairs_banded(pair_queries, pair_subjects, max_distance, cigar_cap=cap, into=into)
            B.check(L.bgsa_hip_reference_placements_dev(self.ref_len, W, self.stride, hit.data_ptr(), hi - lo, k_sel,
                                                        span[lo:hi].data_ptr(), n_ops[lo:hi].data_ptr(), cigar[lo:hi].data_ptr(), cap,
                                                        strand[lo:hi].data_ptr(), ref_begin[lo:hi].data_ptr(), ref_end[lo:hi].data_ptr(),
                                                        keep[lo:hi].data_ptr(), a._stream()), "reference_placements_dev")
        return strand, ref_begin, ref_end, keep, n_ops, cigar

    def _after_place(self, scores, ids, strand, ref_begin, ref_end, keep, n_ops, cigar) -> None:
        """Called with the device tensors of every place_hits result (_map_bucket, stage B of map_pairs) before anything reads them.
        One sequence: nothing to do.  ContigMapper clips the hits to their contigs here, in place."""

    def _sam_passes(self, fmt: str = "sam") -> tuple:
        """The two record passes as (measure, emit), each called with the batch and the rest of the C call's arguments."""
        return getattr(B.lib(), f"bgsa_hip_{fmt}_measure_dev"), getattr(B.lib(), f"bgsa_hip_{fmt}_emit_dev")

    # ---- the one pipeline behind map_reads, map_reads_ragged, map_reads_seeded and map_reads_seeded_ragged ----------------------
    def _coordinates_pass(self):
        """The key pass of sam_records(sort=True): bgsa_hip_bam_coordinates_dev, the contig mapper's with its table."""
        return B.lib().bgsa_hip_bam_coordinates_dev

    def index_ref_lens(self) -> np.ndarray:
        """The lengths of the references in refID's order: what a BAI index of this mapper's records covers."""
        return np.array([self.ref_len], dtype=np.int64)

    def _check(self, who: str, longest: int, ragged: bool, k_best, max_distance, cigar_cap, seeded: bool = False, max_candidates=None,
               plan=None) -> tuple:
        """check_call with this mapper's geometry; map_reads alone takes reads beyond 1,024 bp."""
        return check_call(who, longest, ragged, k_best, max_distance, seeded, cigar_cap, max_candidates, self.window_len, self.stride,
                          self.ref_len, self.n_ids, who != "map_reads", plan)

    @staticmethod
    def _one_length(who: str, reads) -> np.ndarray:
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        if reads.ndim != 2 or reads.shape[0] < 1 or reads.shape[1] < 1:
            raise B.BgsaHipError(f"{who}: rc=-1: reads must be [ns, n] with ns, n >= 1 (one read length per call)")
        return reads

    def _map_bucket(self, rows: np.ndarray, lens, k_sel: int, limit, cap: int, block_rows: int, seed=None, on_device: bool = False) -> tuple:
        """One bucket through the pipeline: rows [n, width] ASCII and lens (the reads' own lengths, or None where all are width
        long) are uploaded (DeviceAligner._set_bucket), the k_sel best windows of every read selected — seed None: select_windows
        over every window; seed (q, max_candidates): select_seeded within min(limit, width) —, placed within limit (place_hits, per
        read where lens is given) and the stream checked for faults.  limit None (exhaustive only): no bound where lens is given,
        else the worst selected distance, one scalar read back.  Returns host arrays: (the six of hit_arrays, n_ops, runs as uint32,
        the reads' seed flags, (emitted, unique, within the bound)); the last two None without a seed.  on_device (the SAM entry points):
        the six, n_ops and the runs stay device tensors, the runs int32 [n, k_sel, cap]; only the flags and the totals are copied."""
        a = self.aligner
        torch = a.torch
        d_rows, d_lens = a._set_bucket(rows, lens, qlen=self.window_len, reads_ragged=lens is not None)
        flags = totals = None
        if seed is None:
            d_rows = None      # only the seed filter reads the ASCII rows again
            scores, ids = self.select_windows(k_sel, block_rows)
            if limit is None and lens is None:
                limit = -int(torch.where(ids >= 0, scores, torch.zeros_like(scores)).min().item())
        else:
            scores, ids, counts, stats = self.select_seeded(d_rows, rows.shape[0], rows.shape[1], min(limit, rows.shape[1]), seed[0], k_sel,
                                                            seed[1], block_rows, d_lens=d_lens)
        strand, ref_begin, ref_end, keep, n_ops, cigar = self.place_hits(ids, limit, cap, block_rows, ragged=lens is not None)
        self._after_place(scores, ids, strand, ref_begin, ref_end, keep, n_ops, cigar)
        a.check_faults()
        if seed is not None:
            flags, totals = counts.cpu().numpy(), tuple(int(x.item()) for x in stats)
        if on_device:
            return (scores, strand, ref_begin, ref_end, keep, ids), n_ops, cigar, flags, totals
        arrays = tuple(x.cpu().numpy() for x in (scores, strand, ref_begin, ref_end, keep, ids))
        return arrays, n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32), flags, totals

    def _map_bins(self, who: str, rows: np.ndarray, lens: np.ndarray, plan, k_sel: int, limit, cap: int, block_rows: int,
                  max_candidates=None, sink=None) -> tuple:
        """The bins of `plan` — [(indices into rows, seed length or None for the exhaustive path)] —, each as one bucket of its own
        width through _map_bucket, scattered into the caller's order.  A bin of one length goes without lengths and launches the
        equal-length kernels; a seeded one too short for its seed and the bound is flagged -3 here, without a call.  Returns
        (hits, flags[ns], [emitted, unique, within], bins: one dict per bin for last_seed_stats).
        sink (the SAM entry points): every bucket's DEVICE tensors go to sink.add(idx, the six, n_ops, runs) instead — nothing but
        the flags is copied, no string is made, and hits is None."""
        ns = rows.shape[0]
        out = None if sink is not None else blank_hits(ns, k_sel, [[None] * k_sel for _ in range(ns)])
        flags, totals, bins = np.zeros(ns, dtype=np.int32), [0, 0, 0], []
        for idx, q in plan:
            mine = lens[idx]
            width, mixed = int(mine.max()), bool((mine != mine[0]).any())
            bins.append(dict(words=(width + 31) // 32, reads=int(idx.size), q=q, emitted=0, unique=0))
            if q is not None and not mixed and width // (min(limit, width) + 1) < q:      # the C call would refuse the bucket
                flags[idx] = -3
                continue
            bucket = rows[:, :width] if idx.size == ns else rows[idx, :width]      # one bin of all reads: no copy
            arrays, n_ops, runs, seen, stats = self._map_bucket(bucket, mine if mixed else None, k_sel, limit, cap, block_rows,
                                                                None if q is None else (q, max_candidates), on_device=sink is not None)
            if sink is not None:
                sink.add(idx, arrays, n_ops, runs)
            else:
                for field, theirs in zip(hit_arrays(out), arrays):
                    field[idx] = theirs
                decode_cigars(who, arrays[4], n_ops, runs, cap, idx, out.cigars)
            if q is not None:
                flags[idx] = seen
                bins[-1].update(emitted=stats[0], unique=stats[1])
                totals = [t + s for t, s in zip(totals, stats)]
        return out, flags, totals, bins

    def _map_uncovered(self, out: ReferenceHits, flags, exhaustive, bound: int) -> None:
        """The reads the seed filter does not cover (a negative flag): one sub-batch through `exhaustive` (rest -> ReferenceHits),
        blanked beyond bound, into the caller's order."""
        rest = np.flatnonzero(flags < 0)
        if rest.size:
            merge_fallback(out, rest, blank_beyond(exhaustive(rest), bound))

    def map_reads(self, reads: np.ndarray, k_best: int = 1, max_distance=None, block_rows: int = 1000, cigar_cap=None) -> ReferenceHits:
        """reads: [ns, n] uint8 ASCII, one length.  Selects every read's k_sel = k_selected(k_best) best windows over both
        strands (top_queries, segment by segment: the number of segments never changes a result), places the read inside
        each within max_distance (place_pairs_banded on the hit windows, gathered on the device block_rows reads at a time) and
        reports reference coordinates, with the copies of one locus marked (keep).  max_distance=None: the worst selected
        distance, one scalar read back, so that every hit is placed.
        A stride above max_stride(window_len, n, max_distance) — with max_distance=None: above window_len - n + 1, where not even
        an exact placement is sure of a window — is refused before anything is launched: some placement within the bound would
        lie in no window, and the best window's distance would not be the reference's optimum.
        cigar_cap=None: window_len + n runs per hit, which cannot overflow (4 bytes each: pass a smaller cap for many reads)."""
        reads = self._one_length("map_reads", reads)
        ns, n = reads.shape
        k_best, _, cap, _, _ = self._check("map_reads", n, False, k_best, max_distance, cigar_cap)
        limit = None if max_distance is None else int(max_distance)
        plan = [(np.arange(ns), None)]      # one bin of the whole batch
        return self._map_bins("map_reads", reads, np.full(ns, n, dtype=np.int32), plan, self.k_selected(k_best), limit, cap, block_rows)[0]

    # ---- seeded mapping: include/bgsa_hip.h "seeded read mapping" -----------------------------------------------------------
    def seed_index(self, seed_len: int):
        """The k-mer index of the forward reference for seeds of seed_len bp, built on the device on first use and kept:
        (offsets int32[4^q + 1], positions int32[max(L - q + 1, 1)]) device tensors; bucket c is positions[offsets[c] : offsets[c + 1]]."""
        q = int(seed_len)
        if q not in self.seed_indexes:
            a, L = self.aligner, B.lib()
            torch = a.torch
            n_offsets = int(L.bgsa_hip_seed_index_offsets(q))
            if n_offsets < 0 or self.ref_len > INT32_MAX:
                raise B.BgsaHipError(f"seed_index: rc=-1: seed_len must lie in 1..{SEED_LEN_MAX} and the reference within 2^31 - 1 bases")
            offsets = torch.empty(n_offsets, dtype=torch.int32, device=a.device)
            positions = torch.empty(max(self.ref_len - q + 1, 1), dtype=torch.int32, device=a.device)
            work = torch.empty(max(int(L.bgsa_hip_seed_index_workspace_bytes(self.ref_len, q)), 8), dtype=torch.uint8, device=a.device)
            B.check(L.bgsa_hip_seed_index_build_dev(self.d_reference.data_ptr(), self.ref_len, q, offsets.data_ptr(), positions.data_ptr(),
                                                    work.data_ptr(), work.numel(), a._stream()), "seed_index_build_dev")
            torch.cuda.current_stream(a.device).synchronize()      # the workspace goes away with this frame
            self.seed_indexes[q] = (offsets, positions)
        return self.seed_indexes[q]

    # The steps of select_seeded, for the reads [lo, hi) of one resident bucket: seed_bucket once, then seed_candidates ->
    # seed_dedupe -> seed_verify -> seed_select per block.  scripts/measure_seeded_*.py time these same methods.
    def seed_bucket(self, d_rows, read_len: int, bound: int, seed_len: int, d_lens=None) -> SeedBucket:
        """What the four steps share: the index of seed_len (built on first use) and the C calls — d_lens None: the equal-length
        ones; d_lens (the bucket's int32 lengths, one per column): the *_lens_dev ones, every read at its own length.  The
        aligner holds the bucket; d_rows are its ASCII rows on the device, read_len + 1 bytes each."""
        L = B.lib()
        offsets, positions = self.seed_index(seed_len)
        shape = (self.ref_len, self.window_len, self.stride, offsets.data_ptr(), positions.data_ptr(), int(seed_len))
        if d_lens is None:
            return SeedBucket(d_rows, int(read_len), int(bound), shape, L.bgsa_hip_seed_count_candidates_dev, L.bgsa_hip_seed_emit_candidates_dev,
                              L.bgsa_hip_reference_verify_pairs_dev, lambda lo, hi: (), ())
        return SeedBucket(d_rows, int(read_len), int(bound), shape, L.bgsa_hip_seed_count_candidates_lens_dev,
                          L.bgsa_hip_seed_emit_candidates_lens_dev, L.bgsa_hip_reference_verify_pairs_lens_dev,
                          lambda lo, hi: (d_lens[lo:hi].data_ptr(),), (d_lens.data_ptr(),))

    def seed_candidates(self, job: SeedBucket, lo: int, hi: int, max_candidates: int, counts):
        """Step 1: count (counts[lo:hi] filled: the candidates of every read, or its flag -1 / -2 / -3), an exclusive scan with its
        one scalar read back — it sizes the lists —, emit.  Returns (cand_read int32[total]: the read's index in the block,
        cand_window int32[total]), copies of one pair among them."""
        a = self.aligner
        torch, dev = a.torch, a.device
        reads = (job.d_rows.data_ptr() + lo * (job.read_len + 1), *job.lens_of(lo, hi), job.read_len, hi - lo, job.bound, int(self.both_strands))
        B.check(job.count(*job.shape, *reads, int(max_candidates), counts[lo:hi].data_ptr(), a._stream()), "seed_count_candidates_dev")
        ends = counts[lo:hi].clamp(min=0).to(torch.int64).cumsum(0)
        total = int(ends[-1].item())                    # the one scalar read back per block: it sizes the candidate arrays
        prefix = (ends - counts[lo:hi].clamp(min=0)).contiguous()
        cand_read = torch.empty(total, dtype=torch.int32, device=dev)
        cand_window = torch.empty(total, dtype=torch.int32, device=dev)
        if total:
            B.check(job.emit(*job.shape, *reads, counts[lo:hi].data_ptr(), prefix.data_ptr(), 0, cand_read.data_ptr(), cand_window.data_ptr(),
                             a._stream()), "seed_emit_candidates_dev")
        return cand_read, cand_window

    def seed_dedupe(self, cand_read, cand_window):
        """Step 2: the candidates sorted by (read, window id), every pair once (torch.unique).  Returns (pair_read int64[n],
        pair_window int32[n])."""
        n_ids2 = 2 * self.n_windows
        keys = self.aligner.torch.unique(cand_read.to(self.aligner.torch.int64) * n_ids2 + cand_window)
        pair_read = keys // n_ids2
        return pair_read, (keys - pair_read * n_ids2).to(self.aligner.torch.int32)

    def seed_verify(self, job: SeedBucket, lo: int, pair_read, pair_window):
        """Step 3: the exact distance of every pair's read (pair_read + lo in the bucket) inside its window, int32[n]."""
        a, L = self.aligner, B.lib()
        torch, dev = a.torch, a.device
        n_pairs = pair_read.numel()
        distance = torch.full((n_pairs,), -1, dtype=torch.int32, device=dev)
        pair_subject = pair_read + lo
        if n_pairs:
            need = int(L.bgsa_hip_reference_verify_workspace_bytes(self.window_len, job.read_len, n_pairs))
            if need and (self.d_verify_work is None or self.d_verify_work.numel() < need):
                self.d_verify_work = torch.empty(need, dtype=torch.uint8, device=dev)
            work = self.d_verify_work if need else None
            B.check(job.verify(self.d_reference.data_ptr(), self.ref_len, self.window_len, self.stride, a.d_peq.data_ptr(), *job.lens_all,
                               job.read_len, a.ns, a.wn, pair_window.data_ptr(), pair_subject.data_ptr(), n_pairs, 0, distance.data_ptr(),
                               None if work is None else work.data_ptr(), 0 if work is None else work.numel(), a._stream()),
                    "reference_verify_pairs_dev")
        return distance

    def seed_select(self, job: SeedBucket, lo: int, hi: int, pair_read, pair_window, distance, k_sel: int, scores, ids) -> None:
        """Step 4: every read's k_sel best candidates within the bound into scores[lo:hi] and ids[lo:hi], the reads' segments of
        the pair list found by searchsorted."""
        a = self.aligner
        torch = a.torch
        n_pairs = pair_read.numel()
        segments = torch.searchsorted(pair_read, torch.arange(hi - lo + 1, dtype=torch.int64, device=a.device)).contiguous()
        B.check(B.lib().bgsa_hip_seed_select_dev(pair_window.data_ptr() if n_pairs else None, distance.data_ptr() if n_pairs else None,
                                                 segments.data_ptr(), hi - lo, job.bound, k_sel, scores[lo:hi].data_ptr(), ids[lo:hi].data_ptr(),
                                                 a._stream()), "seed_select_dev")

    def select_seeded(self, d_rows, n_reads: int, read_len: int, bound: int, seed_len: int, k_sel: int, max_candidates: int,
                      block_rows: int = 1000, d_lens=None):
        """The device half of map_reads_seeded's selection, for the reads the aligner holds AND whose ASCII rows d_rows (stride
        read_len + 1) are on the device: block_rows reads at a time count -> emit -> sort and deduplicate (torch) -> verify ->
        select.  Returns (scores[n_reads, k_sel] int32, window ids[n_reads, k_sel] int32, counts[n_reads] int32: the candidates
        of every read or its flag -1 / -2, stats: three device scalars emitted / unique / within the bound).  A flagged read
        gets a list of unused slots.
        d_lens (the bucket's int32 lengths, one per column; map_reads_seeded_ragged): read_len is the rows' width, every read is
        counted, emitted and verified at its own length by the *_lens_dev calls, and a read too short for seed_len is flagged -3.
        d_lens=None launches exactly the equal-length calls."""
        torch, dev = self.aligner.torch, self.aligner.device
        job = self.seed_bucket(d_rows, read_len, bound, seed_len, d_lens)
        scores = torch.empty((n_reads, k_sel), dtype=torch.int32, device=dev)
        ids = torch.empty((n_reads, k_sel), dtype=torch.int32, device=dev)
        counts = torch.empty(n_reads, dtype=torch.int32, device=dev)
        emitted = torch.zeros((), dtype=torch.int64, device=dev)
        unique, within = torch.zeros_like(emitted), torch.zeros_like(emitted)
        block = max(1, min(int(block_rows), n_reads))
        for lo in range(0, n_reads, block):
            hi = min(lo + block, n_reads)
            cand_read, cand_window = self.seed_candidates(job, lo, hi, max_candidates, counts)
            pair_read, pair_window = self.seed_dedupe(cand_read, cand_window)
            distance = self.seed_verify(job, lo, pair_read, pair_window)
            self.seed_select(job, lo, hi, pair_read, pair_window, distance, k_sel, scores, ids)
            emitted += cand_read.numel()
            unique += pair_read.numel()
            within += ((distance >= 0) & (distance <= bound)).sum()
        return scores, ids, counts, (emitted, unique, within)

    def map_reads_seeded(self, reads: np.ndarray, k_best: int = 1, max_distance=None, seed_len=None, max_candidates=None,
                         block_rows: int = 1000, cigar_cap=None) -> ReferenceHits:
        """map_reads without the pass over every window: an exact pigeonhole k-mer filter names, per read, the windows that can hold
        it within max_distance, and only those are verified (include/bgsa_hip.h "seeded read mapping").  max_distance is required: the
        filter is derived from it.  With B = min(max_distance, n) the result equals blank_beyond(map_reads(reads, k_best,
        max_distance), B) field by field and bit for bit: every window within B is a candidate, the slots beyond B are a suffix
        of map_reads' lists and unplaced there too.
        seed_len=None: min(12, n // (B + 1)); seeds that would overlap (seed_plan) are refused before anything is launched, as are
        map_reads' own refusals (the stride rule, k_best, cigar_cap) and reads beyond 1,024 bp.  One read length per call.
        A read with an 'N' in one of its pieces, or with more than max_candidates candidates (default max(n_ids // 8, 256): the measured break-even), is not answered
        from candidates: those reads, and only those, go through map_reads as a sub-batch.  max_candidates never changes a result,
        only the time.  last_seed_stats says what happened."""
        who = "map_reads_seeded"
        reads = self._one_length(who, reads)
        ns, n = reads.shape
        k_best, bound, cap, max_candidates, (_, _, q) = self._check(who, n, False, k_best, max_distance, cigar_cap, True, max_candidates,
                                                                    lambda limit: seed_plan(n, limit, seed_len))
        plan = [(np.arange(ns), q)]      # one bin, placed within the bound the filter was derived from
        out, flags, totals, _ = self._map_bins(who, reads, np.full(ns, n, dtype=np.int32), plan, self.k_selected(k_best), bound, cap,
                                               block_rows, max_candidates)
        self.last_seed_stats = seed_stats(flags, totals, q, max_candidates)
        self._map_uncovered(out, flags, lambda rest: self.map_reads(reads[rest], k_best, int(max_distance), block_rows, cigar_cap), bound)
        return out

    def map_reads_seeded_ragged(self, reads, k_best: int = 1, max_distance=None, seed_len=None, max_candidates=None,
                                block_rows: int = 1000, cigar_cap=None) -> ReferenceHits:
        """map_reads_seeded for reads of MIXED lengths (byte strings or 1-D uint8 arrays, 1..1,024 bp, as map_reads_ragged takes them):
        exact, and equal to blank_beyond(map_reads_ragged(reads, k_best, max_distance), max_distance) field by field and bit for bit,
        in the caller's order.  The reads are binned by words (seed_plan_ragged: one seed length per bin); every bin is one bucket
        whose padded ASCII rows stay on the device, and runs count -> emit -> sort and deduplicate -> verify -> select with every
        read at its own length (the *_lens_dev calls; a bin of one length launches what map_reads_seeded launches), then the
        placement map_reads_ragged makes for that bin.  A read with an 'N' in a piece (-1), with more than max_candidates
        candidates (-2) or too short for its bin's seed and the bound (-3) goes through map_reads_ragged, all of them as one
        sub-batch.  max_candidates, seed_len and block_rows never change a result.  max_distance is required; the other refusals
        are map_reads_ragged's own, all made before anything is launched or allocated.  last_seed_stats says what happened."""
        who = "map_reads_seeded_ragged"
        rows, lens = B.pad_ragged(reads)
        k_best, _, cap, max_candidates, plan = self._check(who, rows.shape[1], True, k_best, max_distance, cigar_cap, True, max_candidates,
                                                           lambda limit: seed_plan_ragged(lens, limit, seed_len))
        limit = int(max_distance)
        out, flags, totals, bins = self._map_bins(who, rows, lens, plan, self.k_selected(k_best), limit, cap, block_rows, max_candidates)
        self.last_seed_stats = seed_stats(flags, totals, None if seed_len is None else int(seed_len), max_candidates, bins)
        self._map_uncovered(out, flags, lambda rest: self.map_reads_ragged([rows[i, : lens[i]] for i in rest], k_best, limit, block_rows,
                                                                           cigar_cap), limit)
        return out

    def map_reads_ragged(self, reads, k_best: int = 1, max_distance=None, block_rows: int = 1000, cigar_cap=None) -> ReferenceHits:
        """map_reads for reads of MIXED lengths: a list of byte strings or 1-D uint8 arrays, 1..1,024 bp each.  The reads are binned by
        the 32-bit words they occupy (bin_by_words), so that a short read is not scored at the longest one's width; every bin is ONE
        bucket of the aligner (set_reads_ragged(bin, qlen=window_len): every read scored and traced at its own length) and makes
        one pass over the reference — select_windows, then the hit windows gathered by id block_rows reads at a time, traced
        (trace_pairs) and turned into reference coordinates.  A hit whose distance exceeds max_distance is reported unplaced
        (ref_begin -1, keep 0, cigar None), as map_reads does; max_distance=None places every hit.  The result is in the caller's
        order and equals, read by read, map_reads called once per exact length.
        The stride check is map_reads' rule applied with the LONGEST read (shorter reads span less); it is made before anything
        is launched.  cigar_cap=None: window_len + the longest read."""
        rows, lens = B.pad_ragged(reads)
        k_best, _, cap, _, _ = self._check("map_reads_ragged", rows.shape[1], True, k_best, max_distance, cigar_cap)
        limit = None if max_distance is None else int(max_distance)
        plan = [(idx, None) for idx in B.bin_by_words(lens)]
        return self._map_bins("map_reads_ragged", rows, lens, plan, self.k_selected(k_best), limit, cap, block_rows)[0]

    # ---- paired reads: include/bgsa_hip.h "paired reads" --------------------------------------------------------------------
    # The steps of map_pairs' stage B for the pairs [lo, hi) of one end's resident bucket: pair_rescue_windows -> pair_union ->
    # seed_dedupe -> seed_verify -> seed_select, then place_hits over the whole end; stage C is pair_select.
    # scripts/measure_pair_map.py times these same methods.
    def verify_bucket(self, d_rows, read_len: int, bound: int) -> SeedBucket:
        """What seed_verify and seed_select need of a resident bucket of one read length, without an index: the bucket's rows, its
        width, the bound the selection keeps and the equal-length verify call."""
        return SeedBucket(d_rows, int(read_len), int(bound), None, None, None, B.lib().bgsa_hip_reference_verify_pairs_dev, lambda lo, hi: (), ())

    def pair_rescue_windows(self, anchors, lo: int, hi: int, k_anchor: int, insert_max: int):
        """Step 1: the rescue windows of the pairs [lo, hi).  anchors = the mate's (strand, ref_begin, ref_end, keep) as device tensors
        [ns, k].  Returns int32[hi - lo, k_anchor * R]: ids ascending within an anchor's group of R, -1 elsewhere."""
        a = self.aligner
        strand, ref_begin, ref_end, keep = anchors
        slots = rescue_slots(self.ref_len, self.window_len, self.stride, insert_max)
        rescue = a.torch.empty((hi - lo, int(k_anchor) * slots), dtype=a.torch.int32, device=a.device)
        B.check(B.lib().bgsa_hip_pair_rescue_windows_dev(self.ref_len, self.window_len, self.stride, strand[lo:hi].data_ptr(),
                                                         ref_begin[lo:hi].data_ptr(), ref_end[lo:hi].data_ptr(), keep[lo:hi].data_ptr(), hi - lo,
                                                         strand.shape[1], int(k_anchor), int(insert_max), rescue.data_ptr(), a._stream()),
                "pair_rescue_windows_dev")
        return rescue

    def pair_union(self, own_ids, rescue):
        """Step 2: an end's own window ids [n, k_sel] and its rescue windows [n, k_anchor * R] as one candidate list (cand_read
        int32: the pair's index in the block, cand_window int32), the unused entries (-1) left out; seed_dedupe sorts it and
        keeps every id once."""
        torch = self.aligner.torch
        both = torch.cat((own_ids, rescue), dim=1)
        rows = torch.arange(both.shape[0], dtype=torch.int32, device=both.device).unsqueeze(1).expand_as(both)
        used = both >= 0
        return rows[used], both[used]

    def rescue_end(self, reads: np.ndarray, own: ReferenceHits, mate: ReferenceHits, k_best: int, k_pair: int, insert_max: int, bound: int,
                   cap: int, block_rows: int = 1000):
        """Stage B for one end: the bucket uploaded, block_rows pairs at a time the rescue windows of the mate's anchors joined to
        the end's own ids, verified and selected within `bound`, then placed.  Returns device tensors — (scores, strand, ref_begin,
        ref_end, keep, ids, rescued: all [ns, k_pair]), n_ops, cigar — and four device scalars: the anchors, the rescue windows
        emitted, the unique pairs verified, the slots rescued."""
        a = self.aligner
        torch, dev = a.torch, a.device
        ns, n = reads.shape
        d_rows, _ = a._set_bucket(reads, None, qlen=self.window_len)
        job = self.verify_bucket(d_rows, n, bound)
        own_ids = torch.from_numpy(np.ascontiguousarray(own.windows)).to(dev)
        anchors = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (mate.strand, mate.ref_begin, mate.ref_end, mate.keep))
        scores = torch.empty((ns, k_pair), dtype=torch.int32, device=dev)
        ids = torch.empty((ns, k_pair), dtype=torch.int32, device=dev)
        rescued = torch.empty((ns, k_pair), dtype=torch.bool, device=dev)
        emitted = torch.zeros((), dtype=torch.int64, device=dev)
        verified = torch.zeros_like(emitted)
        block = max(1, min(int(block_rows), ns))
        for lo in range(0, ns, block):
            hi = min(lo + block, ns)
            rescue = self.pair_rescue_windows(anchors, lo, hi, k_best, insert_max)
            cand_read, cand_window = self.pair_union(own_ids[lo:hi], rescue)
            pair_read, pair_window = self.seed_dedupe(cand_read, cand_window)
            distance = self.seed_verify(job, lo, pair_read, pair_window)
            self.seed_select(job, lo, hi, pair_read, pair_window, distance, k_pair, scores, ids)
            rescued[lo:hi] = (ids[lo:hi] >= 0) & ~(ids[lo:hi, :, None] == own_ids[lo:hi, None, :]).any(dim=2)
            emitted += (rescue >= 0).sum()
            verified += pair_read.numel()
        strand, ref_begin, ref_end, keep, n_ops, cigar = self.place_hits(ids, bound, cap, block_rows)
        self._after_place(scores, ids, strand, ref_begin, ref_end, keep, n_ops, cigar)
        n_anchors = (anchors[3] != 0).sum(dim=1).clamp(max=k_best).sum()
        return (scores, strand, ref_begin, ref_end, keep, ids, rescued), n_ops, cigar, (n_anchors, emitted, verified, rescued.sum())

    def _rescue_checked(self, e: int, reads, single, call: dict, insert_max: int, block_rows: int):
        """rescue_end for end e of map_pairs' call (check_pair_call's dict), and the stream checked for faults."""
        out = self.rescue_end(reads[e], single[e], single[1 - e], call["k_best"], call["k_pair"], int(insert_max), call["bounds"][e],
                              call["caps"][e], block_rows)
        self.aligner.check_faults()
        return out

    def pair_select(self, one, two, insert_min: int, insert_max: int, block_rows: int = 1000):
        """Stage C: the best proper combination of every pair.  one, two = (scores, strand, ref_begin, ref_end, keep) of the two
        ends' final lists, device tensors [ns, k].  Returns device tensors (proper, slot1, slot2, insert int64, cost, n_best,
        next_cost), int32 unless said, one entry per pair."""
        a = self.aligner
        torch, dev = a.torch, a.device
        ns = one[0].shape[0]
        out = [torch.empty(ns, dtype=torch.int64 if i == 3 else torch.int32, device=dev) for i in range(7)]
        block = max(1, min(int(block_rows), ns))
        for lo in range(0, ns, block):
            hi = min(lo + block, ns)
            B.check(B.lib().bgsa_hip_pair_select_dev(*(x[lo:hi].data_ptr() for x in one), one[0].shape[1],
                                                     *(x[lo:hi].data_ptr() for x in two), two[0].shape[1], hi - lo, int(insert_min),
                                                     int(insert_max), *(x[lo:hi].data_ptr() for x in out), a._stream()), "pair_select_dev")
        return tuple(out)

    def map_pairs(self, reads1: np.ndarray, reads2: np.ndarray, insert_min: int, insert_max: int, k_best: int = 1, max_distance=None,
                  rescue_distance=None, seeded: bool = True, seed_len=None, max_candidates=None, block_rows: int = 1000,
                  cigar_cap=None) -> PairedHits:
        """Paired-end mapping, library type FR (include/bgsa_hip.h "paired reads"): reads1[ns, n1] and reads2[ns, n2] uint8 ASCII,
        row c of both is pair c; the lengths may differ, each in 1..1,024.
        Stage A maps each end alone: map_reads_seeded(reads_e, k_best, max_distance, ...), or with seeded=False map_reads blanked
        beyond min(max_distance, n_e) — the same lists.  Stage B gives every end a second source of candidates: the windows that
        meet the regions its mate's first k_best kept hits point at (rescue_region; at most R = rescue_slots(...) per anchor), joined
        to the end's own windows, verified exactly, the k_pair = k_sel + k_best * R best within min(rescue_distance, n_e) selected
        and placed within that bound.  So the copy of a repeat beside a unique mate, and a mate with more than max_distance edits,
        are found without raising the bound — and with it shortening the seed — for every read.  Stage C chooses, per pair, the
        proper combination of the two final lists of least cost d1 + d2, ties by (slot1, slot2).
        rescue_distance=None: max_distance.  Refused before anything is launched or allocated (check_pair_call states the order): a
        mapper of one strand, unequal row counts, a bad insert range, a missing max_distance, rescue_distance < max_distance, a
        stride above max_stride(window_len, n_e, rescue_distance), k_pair > 64 (nothing is truncated silently), and what
        map_reads_seeded / map_reads refuse.  block_rows, seed_len and max_candidates never change a result.
        last_pair_stats says what happened; with seeded=True its key seed holds the two ends' last_seed_stats."""
        who = "map_pairs"
        reads = (self._one_length(who, reads1), self._one_length(who, reads2))
        call = check_pair_call(self.both_strands, reads[0].shape, reads[1].shape, insert_min, insert_max, k_best, max_distance,
                               rescue_distance, seeded, seed_len, max_candidates, cigar_cap, self.window_len, self.stride, self.ref_len,
                               self.n_ids)
        a = self.aligner
        k_best, k_pair, limit = call["k_best"], call["k_pair"], int(max_distance)
        single, seed = [], []
        for rows in reads:      # stage A: the existing entry points, their fallbacks and stats included
            if seeded:
                single.append(self.map_reads_seeded(rows, k_best, limit, seed_len, max_candidates, block_rows, cigar_cap))
                seed.append(self.last_seed_stats)
            else:
                single.append(blank_beyond(self.map_reads(rows, k_best, limit, block_rows, cigar_cap), min(limit, rows.shape[1])))
        ends, lists, counts = [], [], []
        for e, rows in enumerate(reads):      # stage B: end e's bucket resident, its mate's lists as anchors
            final, n_ops, cigar, seen = self._rescue_checked(e, reads, single, call, insert_max, block_rows)
            arrays = tuple(x.cpu().numpy() for x in final)
            cigars = [[None] * k_pair for _ in range(rows.shape[0])]
            decode_cigars(who, arrays[4], n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32), call["caps"][e], np.arange(rows.shape[0]),
                          cigars)
            ends.append((ReferenceHits(*arrays[:5], cigars, arrays[5]), arrays[6]))
            lists.append(final)
            counts.append(seen)
        chosen = self.pair_select(lists[0][:5], lists[1][:5], insert_min, insert_max, block_rows)      # stage C
        # ... and once more without the rescued slots: the pairs that are proper only through one of them
        plain = self.pair_select(*((*x[:4], x[4] * (~x[6]).to(x[4].dtype)) for x in lists), insert_min, insert_max, block_rows)
        a.check_faults()
        proper, slot1, slot2, insert, cost, n_best, next_cost = (x.cpu().numpy() for x in chosen)
        totals = [int(sum(seen[i] for seen in counts).item()) for i in range(4)]
        self.last_pair_stats = dict(pairs=int(proper.size), anchors=totals[0], rescue_windows=totals[1], pairs_verified=totals[2],
                                    slots_rescued=totals[3], proper=int(proper.sum()),
                                    proper_through_rescue=int(((chosen[0] == 1) & (plain[0] == 0)).sum().item()), k_pair=k_pair,
                                    rescue_slots=call["rescue_slots"], rescue_distance=call["rescue_distance"],
                                    seed=tuple(seed) if seeded else None)
        return PairedHits(ends[0][0], ends[1][0], ends[0][1], ends[1][1], proper, slot1, slot2, insert, cost, n_best, next_cost)

    @staticmethod
    def pairs_of(paired: PairedHits) -> list:
        """Per pair (end 1's chosen Placement or None, end 2's, proper): the chosen slots of map_pairs' result — the proper
        combination, or without one each end's first kept hit — for callers who want no more than that."""
        def chosen(hits: ReferenceHits, c: int, r: int):
            if r < 0:
                return None
            return Placement(int(hits.strand[c, r]), int(hits.ref_begin[c, r]), int(hits.ref_end[c, r]), -int(hits.scores[c, r]), hits.cigars[c][r])
        return [(chosen(paired.end1, c, int(paired.slot1[c])), chosen(paired.end2, c, int(paired.slot2[c])), bool(paired.proper[c]))
                for c in range(paired.proper.shape[0])]

    @staticmethod
    def placements_of(hits: ReferenceHits, k_best: int = 1) -> list:
        """Per read the first k_best kept hits of map_reads' result, best first, as Placement(strand, ref_begin, ref_end,
        distance, cigar) — for callers who want no more than that."""
        out = []
        for c in range(hits.keep.shape[0]):
            rows = np.flatnonzero(hits.keep[c])[: int(k_best)]
            out.append([Placement(int(hits.strand[c, r]), int(hits.ref_begin[c, r]), int(hits.ref_end[c, r]), -int(hits.scores[c, r]),
                                  hits.cigars[c][r]) for r in rows])
        return out

    # ---- SAM records: include/bgsa_hip.h "SAM records" ----------------------------------------------------------------------
    # The mapping pipeline above with a sink in place of the host copies, then on device tensors only: sam_list_mapq, the primary
    # slots gathered (PrimarySink / sam_primaries), sam_records (measure -> scan -> emit -> one copy of the text).
    # scripts/measure_sam.py times these same methods.
    def sam_header(self, reference_name="ref", sort_order="unsorted") -> bytes:
        """The three header lines of this mapper's one reference: @HD (SO: sort_order, "unsorted" or "coordinate"), @SQ with its
        name and length, @PG."""
        name = _field_bytes("sam_header", "reference_name", reference_name).tobytes()
        return sort_order_line("sam_header", sort_order) + b"@SQ\tSN:" + name + b"\tLN:" + str(self.ref_len).encode() + b"\n@PG\tID:bgsa-hip\n"

    def bam_header(self, reference_name="ref", sort_order="unsorted") -> bytes:
        """The UNCOMPRESSED BAM header of this mapper's one reference: the magic, sam_header's text, one reference entry.  write_bam
        frames it.  sort_order="coordinate" is the header of a sort=True call's file."""
        name = _field_bytes("bam_header", "reference_name", reference_name).tobytes()
        return bam_header_bytes("bam_header", self.sam_header(reference_name, sort_order), [(name, self.ref_len)])

    def sam_list_mapq(self, scores, keep, bound: int) -> tuple:
        """bgsa_hip_sam_mapq_dev on device tensors scores, keep [ns, k]: (primary slot, mapq, n1, d2), int32[ns] each."""
        a = self.aligner
        torch = a.torch
        scores, keep = scores.contiguous(), keep.contiguous()
        ns, k = scores.shape
        out = tuple(torch.empty(ns, dtype=torch.int32, device=a.device) for _ in range(4))
        B.check(B.lib().bgsa_hip_sam_mapq_dev(scores.data_ptr(), keep.data_ptr(), ns, k, int(bound), *(x.data_ptr() for x in out), a._stream()),
                "sam_mapq_dev")
        return out

    @staticmethod
    def sam_primaries(torch, slot, arrays, n_ops, cigar) -> tuple:
        """The fields of slot[c] of every read's list, gathered on the device: (strand, ref_begin, ref_end, distance, n_ops,
        runs[ns, cap]); slot -1: strand -1, the rest of no meaning."""
        scores, strand, ref_begin, ref_end = arrays[:4]
        at = slot.clamp(min=0).to(torch.int64).unsqueeze(1)

        def pick(x):
            return x.gather(1, at).squeeze(1)
        runs = cigar.gather(1, at.unsqueeze(2).expand(-1, 1, cigar.shape[2])).squeeze(1)
        return pick(strand).masked_fill(slot < 0, -1), pick(ref_begin), pick(ref_end), -pick(scores), pick(n_ops), runs

    def sam_records(self, who: str, reads: np.ndarray, quals, names, name_offsets, rname, fields: dict, runs, read_label=None, fmt: str = "sam",
                    block_payload: int = BGZF_BLOCK_PAYLOAD, compress: bool = False, sort: bool = False, mark_duplicates: bool = False,
                    ends: int = 1, merge=None, pileup=None):
        """The two record passes.  reads [n_rows, stride] and quals (or None) are the host rows, names / name_offsets / rname what
        check_sam_call returned; fields holds the per-record DEVICE tensors read_row, name_of (int64), read_len, strand, ref_begin,
        ref_end, distance, n_ops, flag, mapq, rnext, pnext, tlen; runs [n, cap] int32 holds record i's runs in row i.  Measure, an
        exclusive scan of the lengths with its one scalar read back — it sizes the text —, emit, the text copied once.  A malformed
        record raises; read_label(i) names record i's read in the message.  fmt "bam": the same passes of the BAM stage, then the
        payload framed into BGZF blocks of block_payload bytes on the device (bgsa_hip_bgzf_frame_dev) and the blocks copied once:
        BamRecords, its offsets in payload coordinates.  compress (fmt "bam" only): the blocks deflated into slots
        (bgsa_hip_bgzf_deflate_dev), their lengths scanned, one more scalar read back, the blocks packed (bgsa_hip_bgzf_pack_dev) and
        copied once — fewer bytes than the payload.  sort (fmt "bam" only; include/bgsa_hip.h "BAM records: coordinate order and
        index"): the key pass on the batch as assembled, torch.sort(stable=True) of the keys, the per-record tensors gathered by the
        permutation — the runs stay where they are, d_runs_row is the permutation —, then the passes above on the permuted batch and
        the index (bam_index): SortedBamRecords, its columns in output order.  mark_duplicates (any fmt; include/bgsa_hip.h
        "Duplicate marking"): on a COPY of fields["flag"], right after the batch is assembled and before the sort, the duplicate
        records of this batch get bit 1024 (mark_duplicate_records; ends 2: records 2u and 2u + 1 are pair u) and
        last_duplicate_stats is filled; everything downstream reads the changed flags.  merge (fmt "bam" only; include/bgsa_hip.h
        "BAM records: merge"): the batch as assembled goes through the duplicate KEY kernel where the merge marks duplicates — no
        mark —, the key pass, then measure, scan and emit in INPUT order, and the device tensors are handed to the BamMerge;
        nothing is framed, no per-record array is copied, the number of records added is returned.  block_payload, compress, sort
        and mark_duplicates are the merge's then.  pileup (any fmt; include/bgsa_hip.h "Pileup"): the batch as assembled — its flags
        those duplicate marking left, before any sort — is counted into the Pileup once the call's last check has passed, so a
        call that raises leaves the pileup as it was; check_pileup_add refuses first."""
        if merge is not None and fmt != "bam":
            raise B.BgsaHipError(f"{who}: rc=-1: merge= needs fmt 'bam'")
        if merge is not None and (sort or compress or mark_duplicates):
            raise B.BgsaHipError(f"{who}: rc=-1: sort, compress and mark_duplicates belong to the merge")
        if sort and fmt != "bam":
            raise B.BgsaHipError(f"{who}: rc=-1: sort=True needs fmt 'bam'")
        if pileup is not None:
            check_pileup_add(who, pileup, self, merge)
        a = self.aligner
        torch, dev = a.torch, a.device
        measure, emit = self._sam_passes(fmt)
        n = int(fields["strand"].shape[0])

        def up(x):
            x = np.ascontiguousarray(x)
            return torch.from_numpy(x if x.flags.writeable else x.copy()).to(dev)
        d_reads, d_quals = up(reads), None if quals is None else up(quals)
        d_names, d_name_offsets, d_rname = up(names), up(name_offsets), up(rname)
        f = {key: value.contiguous() for key, value in fields.items()}
        runs = runs.contiguous()
        runs_row = torch.arange(n, dtype=torch.int64, device=dev)
        label = read_label if read_label is not None else (lambda i: f"read {i}")

        def malformed_error(count: int, i: int):
            return B.BgsaHipError(f"{who}: {count} malformed records, the first the one of {label(i)}: an interval outside "
                                  f"the reference, or runs that do not add up to it and to the read" +
                                  (", or a position, PNEXT or TLEN beyond int32, or more than 65,535 runs" if fmt == "bam" else ""))

        def batch_of(f, runs_row):
            return B.SamBatch(d_reads.data_ptr(), None if d_quals is None else d_quals.data_ptr(), reads.shape[1], reads.shape[0],
                              d_names.data_ptr(), d_name_offsets.data_ptr(), name_offsets.size - 1, names.size, d_rname.data_ptr(), rname.size,
                              self.d_reference.data_ptr(), self.ref_len, runs.data_ptr(), runs.shape[0], runs.shape[1],
                              f["read_row"].data_ptr(), f["name_of"].data_ptr(), runs_row.data_ptr(), f["read_len"].data_ptr(),
                              f["strand"].data_ptr(), f["ref_begin"].data_ptr(), f["ref_end"].data_ptr(), f["distance"].data_ptr(),
                              f["n_ops"].data_ptr(), f["flag"].data_ptr(), f["mapq"].data_ptr(), f["rnext"].data_ptr(), f["pnext"].data_ptr(),
                              f["tlen"].data_ptr())
        if mark_duplicates:
            f = dict(f, flag=f["flag"].clone())
            self.last_duplicate_stats = self.mark_duplicate_records(batch_of(f, runs_row), n, int(ends), f["flag"])
        assembled = (f, runs_row)                       # what the pileup counts: the flags as marked, the order as given
        coordinates, duplicate_keys = None, None
        if merge is not None and merge.mark_duplicates:
            key_counts = torch.zeros(3, dtype=torch.int32, device=dev)
            duplicate_keys = self.duplicate_keys(batch_of(f, runs_row), n, int(ends), key_counts)
        if sort or merge is not None:
            key, *coordinates = self.bam_coordinates(batch_of(f, runs_row), n)
            if int(coordinates[-1].item()):
                raise malformed_error(int(coordinates[-1].item()), int(torch.nonzero(key == torch.iinfo(torch.int64).max).reshape(-1)[0].item()))
        if sort:
            order = self.sort_permutation(key)
            f, coordinates = self.gather_records(f, coordinates[:4], order)
            runs_row, host_order, unsorted_label = order.contiguous(), order.cpu().numpy(), label
            label = lambda i: unsorted_label(int(host_order[i]))      # noqa: E731
        batch = batch_of(f, runs_row)
        malformed = torch.zeros(2, dtype=torch.int32, device=dev)
        lengths = torch.empty(n, dtype=torch.int64, device=dev)
        B.check(measure(batch, n, lengths.data_ptr(), malformed[0:].data_ptr(), a._stream()), f"{fmt}_measure_dev")
        offsets = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(lengths, 0)
        total = int(offsets[-1].item())                 # the one scalar read back: it sizes the text
        if int(malformed[0].item()):
            mapped = f["strand"] >= 0
            over = torch.nonzero(mapped & (f["n_ops"] > runs.shape[1])).reshape(-1)
            if over.numel():
                i = int(over[0].item())
                raise B.BgsaHipError(f"{who}: the hit of {label(i)} has {int(f['n_ops'][i].item())} runs, its row holds {runs.shape[1]} "
                                     f"(raise cigar_cap)")
            raise malformed_error(int(malformed[0].item()), int(torch.nonzero(lengths == 0).reshape(-1)[0].item()))
        text = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)
        B.check(emit(batch, n, offsets.data_ptr(), text.data_ptr(), total, malformed[1:].data_ptr(), a._stream()), f"{fmt}_emit_dev")
        if int(malformed[1].item()):
            raise B.BgsaHipError(f"{who}: the emit pass refused {int(malformed[1].item())} records the measure pass accepted")
        mapped = f["strand"] >= 0
        pos = torch.where(mapped, f["ref_begin"] + 1, f["pnext"] * f["rnext"])
        nm = f["distance"].masked_fill(~mapped, -1)
        mapq = f["mapq"].masked_fill(~mapped, 0)
        if merge is not None:       # the last check is behind us: only now do the merge and the pileup change
            if pileup is not None:
                pileup._add(batch_of(*assembled), n)
            columns = dict(zip(MERGE_COLUMNS, (lengths, key, *coordinates[:4], f["flag"], pos, mapq, nm)))
            if duplicate_keys is not None:
                columns.update(zip(MERGE_DUPLICATE_COLUMNS, duplicate_keys))
            return merge._append(int(ends), text, total, columns, None if duplicate_keys is None else key_counts.tolist())
        kind, payload_bytes, block_offsets = SamRecords, total, None
        if fmt == "bam" and compress:
            kind, (text, total, block_offsets) = BamRecords, self.bgzf_deflated(who, text, total, int(block_payload), with_offsets=True)
        elif fmt == "bam":
            framed = int(B.lib().bgsa_hip_bgzf_framed_bytes(total, int(block_payload)))
            blocks = torch.empty(max(framed, 1), dtype=torch.uint8, device=dev)
            B.check(B.lib().bgsa_hip_bgzf_frame_dev(text.data_ptr(), total, int(block_payload), blocks.data_ptr(), framed, a._stream()),
                    "bgzf_frame_dev")
            kind, text, total = BamRecords, blocks, framed
        index = self.bam_index(who, *coordinates, offsets, payload_bytes, int(block_payload), block_offsets) if sort else None
        if pileup is not None:      # the last check is behind us
            pileup._add(batch_of(*assembled), n)
        if sort:
            return SortedBamRecords(text[:total].cpu().numpy(), offsets.cpu().numpy(), f["flag"].cpu().numpy(), pos.cpu().numpy(),
                                    mapq.cpu().numpy(), nm.cpu().numpy(), coordinates[0].cpu().numpy(), host_order, index)
        return kind(text[:total].cpu().numpy(), offsets.cpu().numpy(), f["flag"].cpu().numpy(), pos.cpu().numpy(), mapq.cpu().numpy(),
                    nm.cpu().numpy())

    def duplicate_keys(self, batch, n: int, ends: int, counts) -> tuple:
        """The key kernel on a bgsa_hip_sam_batch_t of n records: the device tensors (end key int64[n], score int32[n / ends], the
        pair key's halves int64[n / ends] each); counts int32[3] += pair units, fragment units, skipped records."""
        a = self.aligner
        torch, dev = a.torch, a.device
        units = n // ends if ends in (1, 2) else 0
        end_key = torch.empty(max(n, 1), dtype=torch.int64, device=dev)
        score = torch.empty(max(units, 1), dtype=torch.int32, device=dev)
        key_a, key_b = (torch.empty(max(units, 1), dtype=torch.int64, device=dev) for _ in range(2))
        B.check(B.lib().bgsa_hip_dup_keys_dev(batch, n, ends, DUPLICATE_MIN_QUALITY, end_key.data_ptr(), score.data_ptr(), key_a.data_ptr(),
                                              key_b.data_ptr(), counts.data_ptr(), a._stream()), "dup_keys_dev")
        return end_key[:n], score[:units], key_a[:units], key_b[:units]

    def duplicate_order(self, score, *keys) -> tuple:
        """(the permutation, the keys gathered by it) that leaves the entries in (keys ascending, the first the most significant;
        score descending; index ascending) order: stable torch.sort passes, least significant key first — plumbing."""
        torch = self.aligner.torch
        order = torch.sort(-score.to(torch.int64), stable=True)[1]
        for key in reversed(keys):
            order = order[torch.sort(key[order], stable=True)[1]]
        return order.contiguous(), [key[order].contiguous() for key in keys]

    def duplicate_marks(self, keys, order, n: int, ends: int, flag, counts) -> None:
        """The mark kernel on sorted entries: ends 2 the pair pass (keys = the two halves), ends 1 the end pass (keys = the end
        keys); flag int32[n] gets bit 1024; counts int32[3] += duplicate pair units, duplicate fragment units, records flagged."""
        B.check(B.lib().bgsa_hip_dup_mark_dev(keys[0].data_ptr(), keys[1].data_ptr() if len(keys) > 1 else None, order.data_ptr(), n, ends,
                                              flag.data_ptr(), counts.data_ptr(), self.aligner._stream()), "dup_mark_dev")

    def mark_duplicate_records(self, batch, n: int, ends: int, flag) -> dict:
        """Duplicate marking of the batch as assembled (include/bgsa_hip.h "Duplicate marking"): keys and scores, for a paired
        batch the pair pass, then the end pass; the device tensor `flag` (the batch's d_flag) gets bit 1024 on the duplicates.  No
        per-record array goes to the host: the six counters come back in one small copy, as the dict last_duplicate_stats holds."""
        torch = self.aligner.torch
        counts = torch.zeros(6, dtype=torch.int32, device=self.aligner.device)
        end_key, score, key_a, key_b = self.duplicate_keys(batch, n, ends, counts[0:])
        if n and ends == 2:
            order, keys = self.duplicate_order(score, key_a, key_b)
            self.duplicate_marks(keys, order, n, 2, flag, counts[3:])
        if n:
            order, keys = self.duplicate_order(score.repeat_interleave(ends), end_key)
            self.duplicate_marks(keys, order, n, 1, flag, counts[3:])
        return dict(zip(DUPLICATE_STATS, counts.tolist()))

    def bam_coordinates(self, batch, n: int) -> tuple:
        """The key pass on a bgsa_hip_sam_batch_t of n records: the device tensors (key int64, ref_id, pos, end, bin int32, the
        malformed count int32[1])."""
        a = self.aligner
        torch, dev = a.torch, a.device
        key = torch.empty(n, dtype=torch.int64, device=dev)
        ref_id, pos, end, bin_ = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        malformed = torch.zeros(1, dtype=torch.int32, device=dev)
        B.check(self._coordinates_pass()(batch, n, key.data_ptr(), ref_id.data_ptr(), pos.data_ptr(), end.data_ptr(), bin_.data_ptr(),
                                         malformed.data_ptr(), a._stream()), "bam_coordinates_dev")
        return key, ref_id, pos, end, bin_, malformed

    def local_pos(self, pos: np.ndarray) -> np.ndarray:
        """The POS column as the caller sees it: on one sequence the linear positions are it."""
        return pos

    def local_sites(self, pos: np.ndarray) -> tuple:
        """(pos, contig) of a pileup's sites as the caller sees them: on one sequence the linear positions and no contig."""
        return pos, None

    def pileup(self, min_mapq: int = 0, min_base_quality: int = 13, exclude_flags: int = PILEUP_EXCLUDE_FLAGS) -> Pileup:
        """A pileup over this mapper's reference (Pileup; include/bgsa_hip.h "Pileup"): pass it as pileup= to map_reads_sam,
        map_reads_bam, map_pairs_sam or map_pairs_bam, call after call, then read stats(), depth(), counts_host() or sites().
        The count matrix [ref_len, 8] int32 is allocated and zeroed here; check_pileup refuses before that."""
        return Pileup(self, min_mapq, min_base_quality, exclude_flags)

    def bam_merge(self, block_payload: int = BGZF_BLOCK_PAYLOAD, compress: bool = False, mark_duplicates: bool = False, segment_blocks: int = 4096,
                  reserve_bytes=None) -> BamMerge:
        """A merge of this mapper's BAM records over many calls (BamMerge; include/bgsa_hip.h "BAM records: merge"): pass it as
        merge= to map_reads_bam or map_pairs_bam, batch after batch, then finish() or write().  block_payload, compress and
        mark_duplicates are those of a sort=True call and hold for every batch; segment_blocks blocks are gathered, framed or
        deflated and copied at a time; reserve_bytes sizes the payload buffer once (it doubles otherwise).  check_bam_merge
        refuses before anything is allocated."""
        return BamMerge(self, block_payload, compress, mark_duplicates, segment_blocks, reserve_bytes)

    def sort_permutation(self, key):
        """The permutation that puts the keys in order, ties in input order: torch.sort(stable=True), plumbing."""
        return self.aligner.torch.sort(key, stable=True)[1]

    @staticmethod
    def gather_records(fields: dict, coordinates, order) -> tuple:
        """The per-record field tensors and the coordinate tensors in the order of the permutation."""
        return {name: value[order].contiguous() for name, value in fields.items()}, [x[order].contiguous() for x in coordinates]

    def bam_index(self, who: str, ref_id, pos, end, bin_, offsets, payload_bytes: int, block_payload: int, block_offsets=None) -> BamIndex:
        """The BAI arrays of SORTED records on the device — their coordinates (int32[n] each), offsets int64[n + 1] into a payload of
        payload_bytes in blocks of block_payload, block_offsets the deflated blocks' scan or None for stored ones —: marks, one
        cumsum and its scalar, chunks, a stable sort of the chunks by ref << 32 | bin, the suffix minimum over the windows, one copy
        of each array."""
        a = self.aligner
        torch, dev, L = a.torch, a.device, B.lib()
        n, ref_lens = int(ref_id.shape[0]), self.index_ref_lens()
        n_refs = int(ref_lens.size)
        window_base = np.zeros(n_refs + 1, dtype=np.int64)
        windows = int(L.bgsa_hip_bam_index_windows(ref_lens.ctypes.data, n_refs, window_base.ctypes.data))
        if windows < 0:
            raise B.BgsaHipError(f"{who}: rc=-1: a reference shorter than 1 or longer than 2^29 bases has no BAI index")
        top = torch.iinfo(torch.int64).max
        d_base = torch.from_numpy(window_base).to(dev)
        linear = torch.full((max(windows, 1),), top, dtype=torch.int64, device=dev)
        voff_beg, voff_end = (torch.zeros(max(n, 1), dtype=torch.int64, device=dev) for _ in range(2))
        starts = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
        refused = torch.zeros(2, dtype=torch.int32, device=dev)
        n_blocks = (payload_bytes + block_payload - 1) // block_payload
        B.check(L.bgsa_hip_bam_index_marks_dev(ref_id.data_ptr(), pos.data_ptr(), end.data_ptr(), bin_.data_ptr(), n, offsets.data_ptr(),
                                               payload_bytes, block_payload, None if block_offsets is None else block_offsets.data_ptr(),
                                               n_blocks, d_base.data_ptr(), n_refs, voff_beg.data_ptr(), voff_end.data_ptr(),
                                               starts.data_ptr(), linear.data_ptr(), refused[0:].data_ptr(), a._stream()), "bam_index_marks_dev")
        chunk_of = torch.cumsum(starts, 0, dtype=torch.int64)
        n_chunks = int(chunk_of[-1].item()) if n else 0          # the one scalar read back: it sizes the chunk list
        chunk_ref, chunk_bin = (torch.empty(max(n_chunks, 1), dtype=torch.int32, device=dev) for _ in range(2))
        chunk_beg, chunk_end = (torch.empty(max(n_chunks, 1), dtype=torch.int64, device=dev) for _ in range(2))
        B.check(L.bgsa_hip_bam_index_chunks_dev(ref_id.data_ptr(), bin_.data_ptr(), voff_beg.data_ptr(), voff_end.data_ptr(), starts.data_ptr(),
                                                chunk_of.data_ptr(), n, n_chunks, chunk_ref.data_ptr(), chunk_bin.data_ptr(),
                                                chunk_beg.data_ptr(), chunk_end.data_ptr(), refused[1:].data_ptr(), a._stream()),
                "bam_index_chunks_dev")
        if int(refused.sum().item()):
            raise B.BgsaHipError(f"{who}: the index passes refused {refused.tolist()} records (marks, chunks): coordinates out of order or "
                                 f"beyond their reference, or offsets outside the payload")
        by = torch.sort(chunk_ref[:n_chunks].to(torch.int64) << 32 | chunk_bin[:n_chunks].to(torch.int64), stable=True)[1]
        linear = linear[:windows]
        window = torch.arange(windows, dtype=torch.int64, device=dev)
        of_ref = torch.searchsorted(d_base[1:].contiguous(), window, right=True).clamp(max=max(n_refs - 1, 0))
        filled = linear != top
        n_intv = torch.zeros(max(n_refs, 1), dtype=torch.int64, device=dev)
        if windows:
            n_intv.scatter_reduce_(0, of_ref[filled], (window - d_base[of_ref] + 1)[filled], "amax")
            linear = torch.flip(torch.cummin(torch.flip(linear, (0,)), 0)[0], (0,))      # an empty window takes the next filled one's
        return BamIndex(ref_lens, chunk_ref[:n_chunks][by].cpu().numpy(), chunk_bin[:n_chunks][by].cpu().numpy(), chunk_beg[:n_chunks][by].cpu().numpy(),
                        chunk_end[:n_chunks][by].cpu().numpy(), window_base, linear.cpu().numpy(), n_intv[:n_refs].cpu().numpy())

    def bgzf_deflated(self, who: str, payload, total: int, block_payload: int, with_offsets: bool = False) -> tuple:
        """(blocks, their bytes) of the first `total` bytes of the device tensor `payload`, deflated block by block on the device:
        deflate into slots, torch.cumsum of the block lengths, one scalar, pack.  A block that pack refuses raises.  with_offsets:
        the blocks' int64[n_blocks + 1] offsets on the device as a third value."""
        a = self.aligner
        torch, dev, L = a.torch, a.device, B.lib()
        n_blocks = (total + block_payload - 1) // block_payload
        slots = torch.empty(max(n_blocks * (block_payload + 31), 1), dtype=torch.uint8, device=dev)
        lengths = torch.empty(max(n_blocks, 1), dtype=torch.int64, device=dev)
        room = int(L.bgsa_hip_bgzf_deflate_workspace_bytes(total, block_payload))
        workspace = torch.empty(max(room // 4, 1), dtype=torch.int32, device=dev)
        B.check(L.bgsa_hip_bgzf_deflate_dev(payload.data_ptr(), total, block_payload, slots.data_ptr(), n_blocks * (block_payload + 31),
                                            lengths.data_ptr(), workspace.data_ptr(), room, a._stream()), "bgzf_deflate_dev")
        offsets = torch.zeros(n_blocks + 1, dtype=torch.int64, device=dev)
        offsets[1:] = torch.cumsum(lengths[:n_blocks], 0)
        out_bytes = int(offsets[-1].item())              # the one scalar read back: it sizes the packed blocks
        blocks = torch.empty(max(out_bytes, 1), dtype=torch.uint8, device=dev)
        refused = torch.zeros(1, dtype=torch.int32, device=dev)
        B.check(L.bgsa_hip_bgzf_pack_dev(slots.data_ptr(), block_payload, n_blocks, offsets.data_ptr(), blocks.data_ptr(), out_bytes,
                                         refused.data_ptr(), a._stream()), "bgzf_pack_dev")
        if int(refused.item()):
            raise B.BgsaHipError(f"{who}: the pack pass refused {int(refused.item())} of {n_blocks} deflated blocks")
        return (blocks, out_bytes, offsets) if with_offsets else (blocks, out_bytes)

    def _sam_rows(self, who: str, reads) -> tuple:
        """(rows, lens, ragged) of a SAM call's reads: a [ns, n] array as it is, anything else as a list of mixed lengths."""
        if isinstance(reads, np.ndarray) and reads.ndim == 2:
            rows = self._one_length(who, reads)
            return rows, np.full(rows.shape[0], rows.shape[1], dtype=np.int32), False
        return (*B.pad_ragged(reads), True)

    def _map_to(self, sink, rows: np.ndarray, lens: np.ndarray, ragged: bool, k_best, max_distance, seeded: bool, seed_len, max_candidates,
                block_rows: int, cigar_cap):
        """The pipeline of the four map_reads entry points — the one `ragged` and `seeded` name, with its refusals, its bins and its
        exhaustive pass over the reads the seed filter does not cover — with every bucket's device tensors handed to a sink and
        nothing decoded.  sink(ns, k_sel, cap) makes it once the call is accepted; it is returned."""
        who = "map_reads" + ("_seeded" if seeded else "") + ("_ragged" if ragged else "")
        ns, n = rows.shape

        def exhaustive(of_lens):
            return [(idx, None) for idx in B.bin_by_words(of_lens)] if ragged else [(np.arange(of_lens.size), None)]
        if seeded:
            plan_of = (lambda limit: seed_plan_ragged(lens, limit, seed_len)) if ragged else \
                (lambda limit: [(np.arange(ns), seed_plan(n, limit, seed_len)[2])])
            k_best, bound, cap, max_candidates, plan = self._check(who, n, ragged, k_best, max_distance, cigar_cap, True, max_candidates, plan_of)
            limit = int(max_distance) if ragged else bound
        else:
            k_best, bound, cap, _, _ = self._check(who, n, ragged, k_best, max_distance, cigar_cap)
            limit, plan = None if max_distance is None else int(max_distance), exhaustive(lens)
        k_sel = self.k_selected(k_best)
        sink = sink(ns, k_sel, cap)
        _, flags, totals, bins = self._map_bins(who, rows, lens, plan, k_sel, limit, cap, block_rows, max_candidates, sink=sink)
        if seeded:
            self.last_seed_stats = seed_stats(flags, totals, plan[0][1] if not ragged else None if seed_len is None else int(seed_len),
                                              max_candidates, bins if ragged else None)
            rest = np.flatnonzero(flags < 0)
            if rest.size:       # what _map_uncovered does: the exhaustive pass of the same kind, blanked beyond the bound
                self._map_bins(who.replace("_seeded", ""), rows[rest], lens[rest], exhaustive(lens[rest]), k_sel, int(max_distance), cap,
                               block_rows, sink=BeyondSink(self.aligner.torch, sink, rest, limit))
        return sink

    def map_reads_sam(self, reads, names=None, quals=None, reference_name="ref", k_best: int = 2, max_distance=None, seeded: bool = True,
                      seed_len=None, max_candidates=None, block_rows: int = 1000, cigar_cap=None, mark_duplicates: bool = False,
                      pileup=None) -> SamRecords:
        """Single-end reads to SAM records, formatted on the device (include/bgsa_hip.h "SAM records").  reads: a [ns, n] uint8 array
        or a list of byte strings of mixed lengths; the mapping is that of the matching entry point of the four — map_reads_seeded
        (seeded=True: max_distance is required), map_reads, or their _ragged forms — with its refusals.  Every read gives ONE record,
        its first kept hit (flag 0 or 16) or an unmapped record (flag 4): no secondary lines.  MAPQ is the list heuristic: at bound
        max_distance for a seeded call, whose filter makes the list complete within it, at -1 (no bound) for an exhaustive one, whose
        list is its best windows whatever their distance; a second locus is only sure to be listed with k_best >= 2, hence the default.  names=None: r0,
        r1, ...; quals=None: '*'.  check_sam_call refuses before anything is launched.  Nothing but the text, its offsets and four
        columns is copied back; no CIGAR string is made on the host.  mark_duplicates=True: the duplicate reads among THIS call's
        records carry flag bit 1024 (include/bgsa_hip.h "Duplicate marking": mapped reads of equal 5' coordinate — of the record
        as written — and strand; the highest sum of base qualities >= 15 stays, ties the first read); nothing else changes, and
        last_duplicate_stats holds the counts.  Duplicates are found within one call only.  pileup=a Pileup (self.pileup(...);
        include/bgsa_hip.h "Pileup"): the records of this call — the duplicates just marked left out under the default
        exclude_flags — are added to its counts on the device; the call returns what it returns without it."""
        return self._map_reads_records("sam", None, reads, names, quals, reference_name, k_best, max_distance, seeded, seed_len, max_candidates,
                                       block_rows, cigar_cap, mark_duplicates=mark_duplicates, pileup=pileup)

    def map_reads_bam(self, reads, names=None, quals=None, reference_name="ref", k_best: int = 2, max_distance=None, seeded: bool = True,
                      seed_len=None, max_candidates=None, block_rows: int = 1000, cigar_cap=None,
                      block_payload: int = BGZF_BLOCK_PAYLOAD, compress: bool = False, sort: bool = False, mark_duplicates: bool = False,
                      merge=None, pileup=None):
        """map_reads_sam — the same arguments, mapping and record selection — with the records in BAM's layout inside BGZF blocks of
        stored deflate, block_payload bytes of records each (include/bgsa_hip.h "BAM records"): measure, scan, emit, frame, all on the
        device, one copy of the blocks.  A record may straddle blocks.  compress=True: every block deflated on the device instead (LZ77
        and dynamic Huffman codes, or stored where that is no shorter), the blocks packed and copied once — fewer bytes than the
        payload; the same records inflate from them.  check_bam_call refuses before anything is launched; with bam_header and
        write_bam the blocks of one or more calls, compressed or not, make a file.  sort=True: the records of this call leave the
        device in coordinate order (the `samtools sort` key, ties in input order, records without coordinates last) with the arrays
        of a BAI index beside them — SortedBamRecords; bam_header(sort_order="coordinate") and write_bam(index=True) then write
        x.bam and x.bam.bai (include/bgsa_hip.h "BAM records: coordinate order and index").  A sorted call holds ONE call's records;
        many calls go into one sorted file through a merge.
        mark_duplicates=True: map_reads_sam's, independent of compress and sort — the flags change before the records are sorted and
        written, so order and index are those of the unmarked call; duplicates are found within one call only — across calls by a
        merge.  merge=a BamMerge (self.bam_merge(...); include/bgsa_hip.h "BAM records: merge"): the records of this call stay on the
        device behind those of the merge's earlier calls and the number of records added is returned; block_payload, compress, sort
        and mark_duplicates are the merge's and stay at their defaults here; merge.finish() or merge.write() then give the sorted,
        indexed records of all calls as ONE sort=True call on all reads would.  pileup=a Pileup: map_reads_sam's, independent of
        compress and sort; beside a merge that marks duplicates it is refused (the merge flags them at finish())."""
        return self._map_reads_records("bam", block_payload, reads, names, quals, reference_name, k_best, max_distance, seeded, seed_len,
                                       max_candidates, block_rows, cigar_cap, compress, sort, mark_duplicates, merge, pileup)

    def _check_records_call(self, fmt: str, who: str, lens, names, quals, reference_name, block_payload, compress=False, sort=False) -> tuple:
        if fmt == "bam":
            return check_bam_call(who, lens, names, quals, reference_name, block_payload, compress, sort, self.index_ref_lens())
        return check_sam_call(who, lens, names, quals, reference_name)

    def _map_reads_records(self, fmt: str, block_payload, reads, names, quals, reference_name, k_best, max_distance, seeded, seed_len,
                           max_candidates, block_rows, cigar_cap, compress=False, sort=False, mark_duplicates=False, merge=None, pileup=None):
        """What map_reads_sam and map_reads_bam share: everything but the format of the records."""
        who = f"map_reads_{fmt}"
        mark_duplicates = check_mark_duplicates(who, mark_duplicates)
        if merge is not None:
            check_bam_merge_add(who, merge, self, 1, block_payload, compress, sort, mark_duplicates)
        if pileup is not None:
            check_pileup_add(who, pileup, self, merge)
        rows, lens, ragged = self._sam_rows(who, reads)
        rname, flat, name_offsets, qual_rows = self._check_records_call(fmt, who, lens, names, quals, reference_name, block_payload,
                                                                        compress, sort)
        bound = int(max_distance) if seeded and max_distance is not None else -1
        sink = self._map_to(lambda ns, k_sel, cap: PrimarySink(self, ns, cap, bound), rows, lens, ragged, k_best, max_distance, seeded, seed_len,
                            max_candidates, block_rows, cigar_cap)
        self.aligner.check_faults()
        return self.sam_single_records(who, sink, rows, lens, qual_rows, flat, name_offsets, rname, fmt=fmt, block_payload=block_payload,
                                       compress=compress, sort=sort, mark_duplicates=mark_duplicates, merge=merge, pileup=pileup)

    def sam_single_records(self, who: str, sink: "PrimarySink", rows: np.ndarray, lens, qual_rows, names, name_offsets, rname, **form):
        """The records of single-end reads from their primaries on the device: flag 0, 16 or 4, no mate fields.  form: sam_records'
        fmt, block_payload, compress, sort, mark_duplicates, merge and pileup (every mapped record a fragment unit: ends 1)."""
        torch, dev = self.aligner.torch, self.aligner.device
        ns = rows.shape[0]
        index = torch.arange(ns, dtype=torch.int64, device=dev)
        zero = torch.zeros(ns, dtype=torch.int64, device=dev)
        flag = (4 * (sink.strand < 0) + 16 * (sink.strand == 1)).to(torch.int32)
        fields = dict(read_row=index, name_of=index, read_len=torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).to(dev),
                      strand=sink.strand, ref_begin=sink.ref_begin, ref_end=sink.ref_end, distance=sink.distance, n_ops=sink.n_ops,
                      flag=flag, mapq=sink.mapq, rnext=torch.zeros(ns, dtype=torch.int32, device=dev), pnext=zero, tlen=zero)
        return self.sam_records(who, rows, qual_rows, names, name_offsets, rname, fields, sink.runs, ends=1, **form)

    def map_pairs_sam(self, reads1: np.ndarray, reads2: np.ndarray, insert_min: int, insert_max: int, names=None, quals1=None, quals2=None,
                      reference_name="ref", k_best: int = 1, max_distance=None, rescue_distance=None, seeded: bool = True, seed_len=None,
                      max_candidates=None, block_rows: int = 1000, cigar_cap=None, mark_duplicates: bool = False,
                      pileup=None) -> SamRecords:
        """map_pairs to SAM records, formatted on the device: two records per pair, end 1 then end 2, each the slot pair_select chose
        (a proper pair: flag 2) or the end's first kept hit, else unmapped.  Flags 1, 2, 4, 8, 16, 32, 64 / 128; RNEXT '=' and PNEXT
        where the mate is mapped; TLEN where both are; an unmapped end beside a mapped mate takes the mate's RNAME and POS.  MAPQ:
        pair_mapq.  One name per pair.  The stages are map_pairs' own (stage A through the same pipeline, without its strings);
        last_pair_stats is not touched.  check_sam_call and check_pair_call refuse before anything is launched.  mark_duplicates=True:
        both records of every duplicate pair among THIS call's pairs carry flag bit 1024 (include/bgsa_hip.h "Duplicate marking":
        pairs with both ends mapped, of equal 5' coordinates — of the records as written — and strands; the highest sum of base
        qualities >= 15 over both ends stays, ties the first pair), and so does a mapped end whose mate is unmapped where it stands on
        an end of such a pair or behind a better end of its kind; an unmapped mate is not flagged.  last_duplicate_stats holds the
        counts.  Duplicates are found within one call only.  pileup=a Pileup: map_reads_sam's; both records of a pair are counted,
        where the mates overlap both of them."""
        return self._map_pairs_records("sam", None, reads1, reads2, insert_min, insert_max, names, quals1, quals2, reference_name, k_best,
                                       max_distance, rescue_distance, seeded, seed_len, max_candidates, block_rows, cigar_cap,
                                       mark_duplicates=mark_duplicates, pileup=pileup)

    def map_pairs_bam(self, reads1: np.ndarray, reads2: np.ndarray, insert_min: int, insert_max: int, names=None, quals1=None, quals2=None,
                      reference_name="ref", k_best: int = 1, max_distance=None, rescue_distance=None, seeded: bool = True, seed_len=None,
                      max_candidates=None, block_rows: int = 1000, cigar_cap=None, block_payload: int = BGZF_BLOCK_PAYLOAD,
                      compress: bool = False, sort: bool = False, mark_duplicates: bool = False, merge=None, pileup=None):
        """map_pairs_sam — the same arguments, stages and records — in BAM's layout inside BGZF blocks, stored or, with compress=True,
        deflated on the device (map_reads_bam).  sort=True: coordinate order and a BAI index, as map_reads_bam's; of two ends at one
        position end 1 stays in front, and an unmapped end stays right behind the mate whose position it takes.
        mark_duplicates=True: map_pairs_sam's, independent of compress and sort; duplicates are found within one call only — across
        calls by a merge.  merge=a BamMerge: map_reads_bam's, two records per pair; a merge takes paired batches or single-end
        ones, not both.  pileup=a Pileup: map_pairs_sam's."""
        return self._map_pairs_records("bam", block_payload, reads1, reads2, insert_min, insert_max, names, quals1, quals2, reference_name,
                                       k_best, max_distance, rescue_distance, seeded, seed_len, max_candidates, block_rows, cigar_cap,
                                       compress, sort, mark_duplicates, merge, pileup)

    def _map_pairs_records(self, fmt: str, block_payload, reads1, reads2, insert_min, insert_max, names, quals1, quals2, reference_name, k_best,
                           max_distance, rescue_distance, seeded, seed_len, max_candidates, block_rows, cigar_cap, compress=False, sort=False,
                           mark_duplicates=False, merge=None, pileup=None):
        """What map_pairs_sam and map_pairs_bam share: everything but the format of the records."""
        who = f"map_pairs_{fmt}"
        mark_duplicates = check_mark_duplicates(who, mark_duplicates)
        if merge is not None:
            check_bam_merge_add(who, merge, self, 2, block_payload, compress, sort, mark_duplicates)
        if pileup is not None:
            check_pileup_add(who, pileup, self, merge)
        reads = (self._one_length(who, reads1), self._one_length(who, reads2))
        ns = reads[0].shape[0]
        if (quals1 is None) != (quals2 is None):
            raise B.BgsaHipError(f"{who}: rc=-1: quals1 and quals2 come together")
        checked = [self._check_records_call(fmt, who, np.full(ns, rows.shape[1]), names, quals, reference_name, block_payload, compress, sort)
                   for rows, quals in zip(reads, (quals1, quals2))]
        call = check_pair_call(self.both_strands, reads[0].shape, reads[1].shape, insert_min, insert_max, k_best, max_distance,
                               rescue_distance, seeded, seed_len, max_candidates, cigar_cap, self.window_len, self.stride, self.ref_len,
                               self.n_ids)
        a = self.aligner
        single = []
        for rows in reads:      # stage A, the lists copied as map_pairs' stage B takes them, no script decoded
            sink = self._map_to(lambda n, k_sel, cap: ListSink(n, k_sel), rows, np.full(ns, rows.shape[1], dtype=np.int32), False, call["k_best"],
                                int(max_distance), seeded, seed_len, max_candidates, block_rows, cigar_cap)
            single.append(sink.hits if seeded else blank_beyond(sink.hits, min(int(max_distance), rows.shape[1])))
        ends = [self._rescue_checked(e, reads, single, call, insert_max, block_rows) for e in range(2)]      # stage B
        chosen = self.pair_select(ends[0][0][:5], ends[1][0][:5], insert_min, insert_max, block_rows)      # stage C
        a.check_faults()
        return self.sam_pair_records(who, reads, ends, chosen, call, checked, fmt=fmt, block_payload=block_payload, compress=compress,
                                     sort=sort, mark_duplicates=mark_duplicates, merge=merge, pileup=pileup)

    def sam_pair_records(self, who: str, reads, ends, chosen, call: dict, checked, **form):
        """The records of pairs from the device results of map_pairs' stages: ends[e] = rescue_end's return for end e, chosen =
        pair_select's, call = check_pair_call's dict, checked[e] = check_sam_call's return for end e.  form: sam_records' fmt,
        block_payload, compress, sort, mark_duplicates, merge and pileup (records 2u and 2u + 1 are pair u: ends 2)."""
        torch, dev = self.aligner.torch, self.aligner.device
        ns = reads[0].shape[0]
        lists = [final for final, _, _, _ in ends]
        proper, slot1, slot2, _, cost, n_best, next_cost = chosen
        alone = [self.sam_list_mapq(final[0], final[4], call["bounds"][e])[1] for e, final in enumerate(lists)]
        mapq = pair_mapq(torch, proper, n_best, cost, next_cost, *alone)
        cap = max(call["caps"])
        picked = []
        for (final, n_ops, cigar, _), slot in zip(ends, (slot1, slot2)):
            strand, begin, end, distance, ops, runs = self.sam_primaries(torch, slot, final, n_ops, cigar)
            picked.append((strand, begin, end, distance, ops, torch.nn.functional.pad(runs, (0, cap - runs.shape[1]))))
        mapped = [x[0] >= 0 for x in picked]
        pos = [torch.where(m, x[1] + 1, torch.zeros_like(x[1])) for m, x in zip(mapped, picked)]
        both = mapped[0] & mapped[1]
        span = torch.maximum(picked[0][2], picked[1][2]) - torch.minimum(picked[0][1], picked[1][1])
        first_left = picked[0][1] <= picked[1][1]
        tlen1 = torch.where(both, torch.where(first_left, span, -span), torch.zeros_like(span))

        def interleave(one, two):
            return torch.stack((one, two), dim=1).reshape(-1, *one.shape[1:]).contiguous()
        flags = [(1 + 2 * (proper != 0) + 4 * ~mapped[e] + 8 * ~mapped[1 - e] + 16 * (picked[e][0] == 1) + 32 * (picked[1 - e][0] == 1) +
                  (64, 128)[e]).to(torch.int32) for e in range(2)]
        stride = max(reads[0].shape[1], reads[1].shape[1])
        rows = np.full((ns, 2, stride), ord("N"), dtype=np.uint8)
        qual_rows = None if checked[0][3] is None else np.full((ns, 2, stride), ord("!"), dtype=np.uint8)
        for e in range(2):
            rows[:, e, : reads[e].shape[1]] = reads[e]
            if qual_rows is not None:
                qual_rows[:, e, : reads[e].shape[1]] = checked[e][3]
        index = torch.arange(2 * ns, dtype=torch.int64, device=dev)
        read_len = torch.tensor([reads[0].shape[1], reads[1].shape[1]], dtype=torch.int32, device=dev).repeat(ns)
        fields = dict(read_row=index, name_of=index // 2, read_len=read_len, flag=interleave(*flags), mapq=interleave(*mapq),
                      rnext=interleave(mapped[1].to(torch.int32), mapped[0].to(torch.int32)), pnext=interleave(pos[1], pos[0]),
                      tlen=interleave(tlen1, -tlen1),
                      **{key: interleave(picked[0][i], picked[1][i]) for i, key in enumerate(("strand", "ref_begin", "ref_end", "distance", "n_ops"))})
        rname, flat, name_offsets, _ = checked[0]
        return self.sam_records(who, rows.reshape(2 * ns, stride), None if qual_rows is None else qual_rows.reshape(2 * ns, stride), flat,
                                name_offsets, rname, fields, interleave(picked[0][5], picked[1][5]),
                                read_label=lambda i: f"end {i % 2 + 1} of pair {i // 2}", ends=2, **form)


# ---- the sinks of ReferenceMapper._map_bins: what the SAM entry points keep of a bucket's device tensors ---------------------------
class ListSink:
    """The six arrays of every bucket copied into one host result in the caller's order, cigars None: map_pairs' stage A lists."""

    def __init__(self, ns: int, k_sel: int):
        self.hits = blank_hits(ns, k_sel, None)

    def add(self, idx, arrays, n_ops, cigar) -> None:
        for field, theirs in zip(hit_arrays(self.hits), arrays):
            field[idx] = theirs.cpu().numpy()


class PrimarySink:
    """Per read, on the device: the primary slot of its list (bgsa_hip_sam_mapq_dev at `bound`), its MAPQ, and that slot's strand,
    interval, distance, n_ops and runs, gathered bucket by bucket into the caller's order.  Nothing is copied to the host."""

    def __init__(self, mapper: "ReferenceMapper", ns: int, cap: int, bound: int):
        torch, dev = mapper.aligner.torch, mapper.aligner.device
        self.mapper, self.bound = mapper, int(bound)
        self.mapq = torch.zeros(ns, dtype=torch.int32, device=dev)
        self.strand = torch.full((ns,), -1, dtype=torch.int32, device=dev)
        self.ref_begin = torch.full((ns,), -1, dtype=torch.int64, device=dev)
        self.ref_end = torch.full((ns,), -1, dtype=torch.int64, device=dev)
        self.distance = torch.zeros(ns, dtype=torch.int32, device=dev)
        self.n_ops = torch.zeros(ns, dtype=torch.int32, device=dev)
        self.runs = torch.zeros((ns, cap), dtype=torch.int32, device=dev)

    def add(self, idx, arrays, n_ops, cigar) -> None:
        torch = self.mapper.aligner.torch
        slot, mapq, _, _ = self.mapper.sam_list_mapq(arrays[0], arrays[4], self.bound)
        picked = self.mapper.sam_primaries(torch, slot, arrays, n_ops, cigar)
        at = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(self.mapq.device)
        self.mapq[at] = mapq
        for mine, theirs in zip((self.strand, self.ref_begin, self.ref_end, self.distance, self.n_ops, self.runs), picked):
            mine[at] = theirs


class BeyondSink:
    """A sink for the exhaustive pass over the reads `rest` of a seeded call: every slot beyond `bound` blanked on the device, as
    blank_beyond does on the host, and the bucket's indices taken through rest."""

    def __init__(self, torch, sink, rest, bound: int):
        self.torch, self.sink, self.rest, self.bound = torch, sink, np.asarray(rest), int(bound)

    def add(self, idx, arrays, n_ops, cigar) -> None:
        scores, strand, ref_begin, ref_end, keep, ids = arrays
        gone = (ids < 0) | (-scores.to(self.torch.int64) > self.bound)
        blanked = (scores.masked_fill(gone, INT32_MIN), strand.masked_fill(gone, -1), ref_begin.masked_fill(gone, -1),
                   ref_end.masked_fill(gone, -1), keep.masked_fill(gone, 0), ids.masked_fill(gone, -1))
        self.sink.add(self.rest[idx], blanked, n_ops, cigar)


# ---- a reference of several contigs: include/bgsa_hip.h "a reference of several contigs" -------------------------------------------
def contig_layout(lens, window_len: int, padding=None) -> tuple[np.ndarray, int]:
    """(starts int64[C], total) of contigs of the lengths `lens` laid out in one reference with `padding` bytes of 'N' between
    neighbours (None: window_len): start_0 = 0, start_{i+1} = start_i + len_i + padding, total = start_{C-1} + len_{C-1}.  Refused:
    no contig, a length below 1, padding < window_len, a total beyond int64.  Pure Python: no device, no library (it restates
    bgsa_hip_contig_layout)."""
    W = int(window_len)
    P = W if padding is None else int(padding)
    sizes = [int(n) for n in lens]
    if len(sizes) < 1:
        raise B.BgsaHipError("contig_layout: rc=-1: n_contigs is not positive")
    if W < 1 or P < W:
        raise B.BgsaHipError(f"contig_layout: rc=-1: contig_padding {P} is below window_len {W}: a window would hold bases of two contigs")
    starts, at = [], 0
    for i, n in enumerate(sizes):
        if n < 1:
            raise B.BgsaHipError(f"contig_layout: rc=-1: contig {i} is empty (a contig length is below 1)")
        at += P if i else 0
        starts.append(at)
        at += n
        if at > 2 ** 63 - 1:
            raise B.BgsaHipError("contig_layout: rc=-1: the padded contigs do not fit int64")
    return np.array(starts, dtype=np.int64), at


def read_fasta(data) -> tuple[list, list]:
    """(names, sequences) of FASTA text: `data` is the text as bytes, or a path.  A record's name is its header up to the first
    blank; its sequence the lines below, joined, blanks dropped.  Refused: text in front of the first header, no record, an empty
    name, an empty record, a name given twice."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        with open(data, "rb") as handle:
            data = handle.read()
    names, parts = [], []
    for line in bytes(data).splitlines():
        line = line.strip()
        if line.startswith(b">"):
            words = line[1:].split()
            if not words:
                raise B.BgsaHipError(f"read_fasta: rc=-1: record {len(names)} has no name")
            names.append(words[0].decode("ascii", "replace"))
            parts.append([])
        elif line:
            if not parts:
                raise B.BgsaHipError("read_fasta: rc=-1: text in front of the first '>' header")
            parts[-1].append(b"".join(line.split()))
    if not names:
        raise B.BgsaHipError("read_fasta: rc=-1: no record")
    sequences = [b"".join(lines) for lines in parts]
    for name, sequence in zip(names, sequences):
        if not sequence:
            raise B.BgsaHipError(f"read_fasta: rc=-1: record {name} is empty")
    if len(set(names)) != len(names):
        twice = next(name for i, name in enumerate(names) if name in names[:i])
        raise B.BgsaHipError(f"read_fasta: rc=-1: the name {twice} is given twice")
    return names, sequences


class ContigHits(NamedTuple):
    """What ContigMapper's map_reads entry points return: ReferenceHits with the contig of every slot, the interval LOCAL to it."""
    scores: np.ndarray      # [ns, k_sel] int32: minus the distance AFTER the clip; INT32_MIN = unused slot
    strand: np.ndarray
    ref_begin: np.ndarray   # [ns, k_sel] int64: half-open interval on the forward contig, -1 where the hit is not placed
    ref_end: np.ndarray
    keep: np.ndarray
    cigars: list
    windows: np.ndarray     # window ids of the padded reference
    contig: np.ndarray      # [ns, k_sel] int32: the contig's index, -1 where the hit is not placed


class ContigPlacement(NamedTuple):
    contig: int
    strand: int
    ref_begin: int
    ref_end: int
    distance: int
    cigar: str


class ContigMapper(ReferenceMapper):
    """A reference of several contigs: names[i] and sequences[i] (bytes, str or 1-D uint8 arrays of ASCII bases) are laid out in ONE
    padded reference (contig_layout; contig_padding=None: window_len bytes of 'N' between neighbours, and behind the last contig
    where the whole is shorter than a window), on which ReferenceMapper's pipeline runs unchanged.  Right after every placement the
    hits are clipped to their contigs on the device (bgsa_hip_contig_clip_dev), so every reported hit lies inside ONE contig: the
    map_reads entry points return ContigHits, map_pairs PairedHits whose ends are ContigHits, the SAM entry points records with the
    contig's name and local positions; sam_header writes one @SQ per contig.  contig_starts / contig_lens are the layout.

    Limits: those of ReferenceMapper, and the clip's: the lists are not sorted again, so a hit whose 'N' bases stood on padding can
    carry a distance above its neighbour's and above max_distance; windows and rescue regions on padding cost time, not correctness;
    map_pairs refuses insert_max > contig_padding, so mates on different contigs are never proper."""

    def __init__(self, names, sequences, window_len: int, stride: int, contig_padding=None, device: str = "cuda:0", both_strands: bool = True,
                 segment_windows: int = 65536):
        who = "ContigMapper"
        names, sequences = list(names), list(sequences)
        if len(names) != len(sequences):
            raise B.BgsaHipError(f"{who}: rc=-1: {len(names)} names for {len(sequences)} sequences")
        self.contig_names = [_field_bytes(who, f"the name of contig {i}", name).tobytes() for i, name in enumerate(names)]
        if len(set(self.contig_names)) != len(self.contig_names):
            twice = next(name for i, name in enumerate(self.contig_names) if name in self.contig_names[:i])
            raise B.BgsaHipError(f"{who}: rc=-1: the contig name {twice.decode()} is given twice")
        bases = []
        for i, sequence in enumerate(sequences):
            if isinstance(sequence, str):
                sequence = sequence.encode("ascii")
            one = np.frombuffer(sequence, dtype=np.uint8) if isinstance(sequence, (bytes, bytearray, memoryview)) else \
                np.ascontiguousarray(sequence, dtype=np.uint8)
            if one.ndim != 1 or (one == ord("\n")).any():
                raise B.BgsaHipError(f"{who}: rc=-1: contig {i} is not the bases of one sequence (1-D, no newline: read_fasta reads a file)")
            bases.append(one)
        self.contig_padding = int(window_len) if contig_padding is None else int(contig_padding)
        self.contig_starts, total = contig_layout([one.size for one in bases], window_len, self.contig_padding)
        self.contig_lens = np.array([one.size for one in bases], dtype=np.int64)
        padded = np.full(max(total, int(window_len)), ord("N"), dtype=np.uint8)
        for at, one in zip(self.contig_starts.tolist(), bases):
            padded[at: at + one.size] = one
        super().__init__(padded, window_len, stride, device, both_strands, segment_windows)
        torch, dev = self.aligner.torch, self.aligner.device
        self.d_contig_starts = torch.from_numpy(self.contig_starts).to(dev)
        self.d_contig_lens = torch.from_numpy(self.contig_lens).to(dev)
        offsets = np.zeros(len(names) + 1, dtype=np.int64)
        np.cumsum([len(name) for name in self.contig_names], out=offsets[1:])
        self.d_contig_names = torch.from_numpy(np.frombuffer(b"".join(self.contig_names), dtype=np.uint8).copy()).to(dev)
        self.d_contig_name_offsets = torch.from_numpy(offsets).to(dev)
        self.contig_table = B.SamContigs(self.d_contig_names.data_ptr(), self.d_contig_name_offsets.data_ptr(), int(offsets[-1]),
                                         self.d_contig_starts.data_ptr(), self.d_contig_lens.data_ptr(), len(names))

    # ---- the clip, and the way back to the contigs' own coordinates -----------------------------------------------------------
    def _after_place(self, scores, ids, strand, ref_begin, ref_end, keep, n_ops, cigar) -> None:
        a = self.aligner
        ns, k = ids.shape
        if not all(x.is_contiguous() for x in (scores, strand, ref_begin, ref_end, keep, n_ops, cigar)):
            raise B.BgsaHipError("contig_clip_dev: the lists of a placement are not contiguous")
        contig = a.torch.empty((ns, k), dtype=a.torch.int32, device=a.device)
        B.check(B.lib().bgsa_hip_contig_clip_dev(self.d_contig_starts.data_ptr(), self.d_contig_lens.data_ptr(), self.contig_lens.size,
                                                 self.ref_len, ns, k, scores.data_ptr(), strand.data_ptr(), ref_begin.data_ptr(),
                                                 ref_end.data_ptr(), keep.data_ptr(), n_ops.data_ptr(), cigar.data_ptr(), cigar.shape[2],
                                                 contig.data_ptr(), a._stream()), "contig_clip_dev")

    def contig_of(self, linear) -> np.ndarray:
        """The contig whose start is the last one at or below every linear position (int32; -1 for a negative position)."""
        linear = np.asarray(linear, dtype=np.int64)
        return np.where(linear >= 0, np.searchsorted(self.contig_starts, linear, side="right") - 1, -1).astype(np.int32)

    def localise(self, hits: ReferenceHits) -> ContigHits:
        """A result in the padded reference's coordinates — clipped: every placed interval inside one contig — as ContigHits."""
        contig = self.contig_of(hits.ref_begin)
        shift = np.where(contig >= 0, self.contig_starts[np.maximum(contig, 0)], 0)
        return ContigHits(hits.scores, hits.strand, hits.ref_begin - shift, hits.ref_end - shift, hits.keep, hits.cigars, hits.windows, contig)

    def _linear(self, call, *args, **kwargs):
        """A base-class entry point run with this class's overrides answering in LINEAR coordinates: the base pipeline calls the
        entry points from one another (the exhaustive pass of a seeded call, stage A of map_pairs) and reads what they return."""
        self._nested = getattr(self, "_nested", 0) + 1
        try:
            return call(*args, **kwargs)
        finally:
            self._nested -= 1

    def _contig_hits(self, call, args, kwargs):
        hits = self._linear(call, *args, **kwargs)
        return hits if getattr(self, "_nested", 0) else self.localise(hits)

    def map_reads(self, *args, **kwargs) -> ContigHits:
        """ReferenceMapper.map_reads on the padded reference, clipped: ContigHits."""
        return self._contig_hits(super().map_reads, args, kwargs)

    def map_reads_ragged(self, *args, **kwargs) -> ContigHits:
        """ReferenceMapper.map_reads_ragged on the padded reference, clipped: ContigHits."""
        return self._contig_hits(super().map_reads_ragged, args, kwargs)

    def map_reads_seeded(self, *args, **kwargs) -> ContigHits:
        """ReferenceMapper.map_reads_seeded on the padded reference, clipped: ContigHits."""
        return self._contig_hits(super().map_reads_seeded, args, kwargs)

    def map_reads_seeded_ragged(self, *args, **kwargs) -> ContigHits:
        """ReferenceMapper.map_reads_seeded_ragged on the padded reference, clipped: ContigHits."""
        return self._contig_hits(super().map_reads_seeded_ragged, args, kwargs)

    def _check_insert(self, who: str, insert_max) -> None:
        if int(insert_max) > self.contig_padding:
            raise B.BgsaHipError(f"{who}: rc=-1: insert_max {int(insert_max)} exceeds contig_padding {self.contig_padding}: mates on "
                                 f"neighbouring contigs could pass for a proper pair (build the mapper with contig_padding >= insert_max)")

    def map_pairs(self, reads1, reads2, insert_min: int, insert_max: int, *args, **kwargs) -> PairedHits:
        """ReferenceMapper.map_pairs on the padded reference: the pair is chosen on the clipped linear coordinates, the ends come
        back as ContigHits.  insert_max > contig_padding is refused first."""
        self._check_insert("map_pairs", insert_max)
        paired = self._linear(super().map_pairs, reads1, reads2, insert_min, insert_max, *args, **kwargs)
        return paired._replace(end1=self.localise(paired.end1), end2=self.localise(paired.end2))

    @staticmethod
    def pairs_of(paired: PairedHits) -> list:
        """ReferenceMapper.pairs_of with ContigPlacements."""
        def chosen(hits: ContigHits, c: int, r: int):
            if r < 0:
                return None
            return ContigPlacement(int(hits.contig[c, r]), int(hits.strand[c, r]), int(hits.ref_begin[c, r]), int(hits.ref_end[c, r]),
                                   -int(hits.scores[c, r]), hits.cigars[c][r])
        return [(chosen(paired.end1, c, int(paired.slot1[c])), chosen(paired.end2, c, int(paired.slot2[c])), bool(paired.proper[c]))
                for c in range(paired.proper.shape[0])]

    @staticmethod
    def placements_of(hits: ContigHits, k_best: int = 1) -> list:
        """ReferenceMapper.placements_of with ContigPlacements."""
        out = []
        for c in range(hits.keep.shape[0]):
            rows = np.flatnonzero(hits.keep[c])[: int(k_best)]
            out.append([ContigPlacement(int(hits.contig[c, r]), int(hits.strand[c, r]), int(hits.ref_begin[c, r]), int(hits.ref_end[c, r]),
                                        -int(hits.scores[c, r]), hits.cigars[c][r]) for r in rows])
        return out

    # ---- SAM records: the contig form ------------------------------------------------------------------------------------------
    def sam_header(self, reference_name=None, sort_order="unsorted") -> bytes:
        """@HD (SO: sort_order, "unsorted" or "coordinate"), one @SQ per contig in order — its name and its own length —, @PG.
        reference_name is not used."""
        lines = [b"@SQ\tSN:" + name + b"\tLN:" + str(int(n)).encode() + b"\n" for name, n in zip(self.contig_names, self.contig_lens)]
        return sort_order_line("sam_header", sort_order) + b"".join(lines) + b"@PG\tID:bgsa-hip\n"

    def _sam_passes(self, fmt: str = "sam") -> tuple:
        L, table = B.lib(), self.contig_table
        measure, emit = getattr(L, f"bgsa_hip_{fmt}_measure_contigs_dev"), getattr(L, f"bgsa_hip_{fmt}_emit_contigs_dev")
        return (lambda batch, *rest: measure(batch, table, *rest), lambda batch, *rest: emit(batch, table, *rest))

    def bam_header(self, reference_name=None, sort_order="unsorted") -> bytes:
        """The UNCOMPRESSED BAM header: sam_header's text and one reference entry per contig, in the order refID counts them.
        reference_name is not used."""
        return bam_header_bytes("bam_header", self.sam_header(sort_order=sort_order), list(zip(self.contig_names, self.contig_lens.tolist())))

    def _coordinates_pass(self):
        call, table = B.lib().bgsa_hip_bam_coordinates_contigs_dev, self.contig_table
        return lambda batch, *rest: call(batch, table, *rest)

    def index_ref_lens(self) -> np.ndarray:
        return np.asarray(self.contig_lens, dtype=np.int64)

    def sam_records(self, who: str, reads, quals, names, name_offsets, rname, fields: dict, runs, read_label=None, **form):
        """ReferenceMapper.sam_records through the contig passes: the fields are linear, the device localises them; TLEN is set to 0
        where the mate lies on another contig; the pos column comes back local.  rname is not used.  form: fmt, block_payload, compress, sort,
        mark_duplicates, ends, merge and pileup (the duplicate keys and the pileup's rows are linear coordinates: equal local
        positions on two contigs are two keys, two rows)."""
        torch = self.aligner.torch
        own = torch.searchsorted(self.d_contig_starts, fields["ref_begin"].contiguous(), right=True)
        mate = torch.searchsorted(self.d_contig_starts, (fields["pnext"] - 1).contiguous(), right=True)
        fields = dict(fields, tlen=torch.where(own == mate, fields["tlen"], torch.zeros_like(fields["tlen"])))
        records = super().sam_records(who, reads, quals, names, name_offsets, rname, fields, runs, read_label, **form)
        if form.get("merge") is not None:
            return records                       # the number of records added: the merge localises at finish
        return records._replace(pos=self.local_pos(records.pos))

    def local_pos(self, pos: np.ndarray) -> np.ndarray:
        at = np.maximum(self.contig_of(pos - 1), 0)
        return np.where(pos > 0, pos - self.contig_starts[at], 0)

    def local_sites(self, pos: np.ndarray) -> tuple:
        """(pos local to its contig, contig) of a pileup's sites: the device side stays linear."""
        contig = self.contig_of(pos)
        return pos - self.contig_starts[np.maximum(contig, 0)], contig

    def map_reads_sam(self, reads, names=None, quals=None, reference_name="ref", **kwargs) -> SamRecords:
        """ReferenceMapper.map_reads_sam with RNAME the contig's name and POS local to it.  reference_name is not used."""
        return super().map_reads_sam(reads, names, quals, reference_name, **kwargs)

    def map_pairs_sam(self, reads1, reads2, insert_min: int, insert_max: int, *args, **kwargs) -> SamRecords:
        """ReferenceMapper.map_pairs_sam in the contig form: RNEXT '=' or the mate's contig, PNEXT local, TLEN 0 across contigs; an
        unmapped end takes its mate's contig.  insert_max > contig_padding is refused first."""
        self._check_insert("map_pairs_sam", insert_max)
        return super().map_pairs_sam(reads1, reads2, insert_min, insert_max, *args, **kwargs)

    def map_reads_bam(self, reads, names=None, quals=None, reference_name="ref", **kwargs):
        """ReferenceMapper.map_reads_bam with refID the contig's index in bam_header's order and pos local to it.  reference_name is not
        used."""
        return super().map_reads_bam(reads, names, quals, reference_name, **kwargs)

    def map_pairs_bam(self, reads1, reads2, insert_min: int, insert_max: int, *args, **kwargs):
        """ReferenceMapper.map_pairs_bam in the contig form: next_refID the mate's contig, next_pos local, tlen 0 across contigs.
        insert_max > contig_padding is refused first."""
        self._check_insert("map_pairs_bam", insert_max)
        return super().map_pairs_bam(reads1, reads2, insert_min, insert_max, *args, **kwargs)

"""Reads mapped onto ONE reference sequence: the windows are cut on the device, on both strands, and the hits come back in
reference coordinates (include/bgsa_hip.h "a reference as the query set").

The geometry is stated once in the header and restated here (window_plan, max_stride): L mapped bytes, 1 <= S <= W <= L,
n_windows = 1 + ceil((L - W) / S), start(w) = min(w * S, L - W); forward window w has id w, its reverse complement id
n_windows + w.
"""
from __future__ import annotations

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
    strand, ref_begin and ref_end -1, keep 0, cigar None.  This is what map_reads_seeded returns, bit for bit."""
    gone = (hits.windows < 0) | (-hits.scores.astype(np.int64) > int(bound))
    cigars = [[None if gone[c, r] else text for r, text in enumerate(row)] for c, row in enumerate(hits.cigars)]
    return ReferenceHits(np.where(gone, INT32_MIN, hits.scores).astype(np.int32), np.where(gone, -1, hits.strand).astype(np.int32),
                         np.where(gone, -1, hits.ref_begin).astype(np.int64), np.where(gone, -1, hits.ref_end).astype(np.int64),
                         np.where(gone, 0, hits.keep).astype(np.int32), cigars, np.where(gone, -1, hits.windows).astype(np.int32))


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
        self.last_seed_stats = None

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
        a = self.aligner
        torch = a.torch
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        if reads.ndim != 2 or reads.shape[0] < 1 or reads.shape[1] < 1:
            raise B.BgsaHipError("map_reads: rc=-1: reads must be [ns, n] with ns, n >= 1 (one read length per call)")
        ns, n = reads.shape
        k_best = int(k_best)
        if not 1 <= k_best <= B.V_NUM:
            raise B.BgsaHipError(f"map_reads: rc=-1: k_best must lie in 1..{B.V_NUM}")
        if max_distance is not None and int(max_distance) < 0:
            raise B.BgsaHipError("map_reads: rc=-1: max_distance is negative")
        bound = 0 if max_distance is None else min(int(max_distance), n)
        largest = max_stride(self.window_len, n, bound)
        if self.stride > largest:
            allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
            raise B.BgsaHipError(f"map_reads: rc=-1: at stride {self.stride} a placement of a {n} bp read within distance {bound} can lie in "
                                 f"no window of {self.window_len} bp: {allowed}")
        k_sel = self.k_selected(k_best)
        W = self.window_len
        cap = W + n if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise B.BgsaHipError("map_reads: rc=-1: cigar_cap is not positive")

        a.set_subjects(reads, qlen=W)
        scores, ids = self.select_windows(k_sel, block_rows)
        if max_distance is None:
            max_distance = -int(torch.where(ids >= 0, scores, torch.zeros_like(scores)).min().item())
        strand, ref_begin, ref_end, keep, n_ops, cigar = self.place_hits(ids, int(max_distance), cap, block_rows)
        a.check_faults()

        kept = keep.cpu().numpy()
        counts, runs = n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32)
        cigars = [[None] * k_sel for _ in range(ns)]
        for c, r in zip(*np.nonzero(kept)):
            if counts[c, r] > cap:
                raise B.BgsaHipError(f"map_reads: hit {r} of read {c} has {counts[c, r]} runs, its row holds {cap} (raise cigar_cap)")
            cigars[c][r] = "".join(f"{w >> 4}{B.CIGAR_OPS[w & 15]}" for w in runs[c, r, : counts[c, r]].tolist())
        return ReferenceHits(scores.cpu().numpy(), strand.cpu().numpy(), ref_begin.cpu().numpy(), ref_end.cpu().numpy(), kept, cigars,
                             ids.cpu().numpy())

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
        a, L = self.aligner, B.lib()
        torch, dev, W, S = a.torch, a.device, self.window_len, self.stride
        offsets, positions = self.seed_index(seed_len)
        n_ids2 = 2 * self.n_windows
        scores = torch.empty((n_reads, k_sel), dtype=torch.int32, device=dev)
        ids = torch.empty((n_reads, k_sel), dtype=torch.int32, device=dev)
        counts = torch.empty(n_reads, dtype=torch.int32, device=dev)
        emitted = torch.zeros((), dtype=torch.int64, device=dev)
        unique, within = torch.zeros_like(emitted), torch.zeros_like(emitted)
        shape = (self.ref_len, W, S, offsets.data_ptr(), positions.data_ptr(), int(seed_len))
        block = max(1, min(int(block_rows), n_reads))
        for lo in range(0, n_reads, block):
            hi = min(lo + block, n_reads)
            rows = d_rows.data_ptr() + lo * (read_len + 1)
            reads = (rows, read_len, hi - lo, bound, int(self.both_strands))
            count, emit, verify, lens_arg = L.bgsa_hip_seed_count_candidates_dev, L.bgsa_hip_seed_emit_candidates_dev, \
                L.bgsa_hip_reference_verify_pairs_dev, ()
            if d_lens is not None:
                reads = (rows, d_lens[lo:hi].data_ptr()) + reads[1:]
                count, emit, verify, lens_arg = L.bgsa_hip_seed_count_candidates_lens_dev, L.bgsa_hip_seed_emit_candidates_lens_dev, \
                    L.bgsa_hip_reference_verify_pairs_lens_dev, (d_lens.data_ptr(),)
            B.check(count(*shape, *reads, int(max_candidates), counts[lo:hi].data_ptr(), a._stream()), "seed_count_candidates_dev")
            ends = counts[lo:hi].clamp(min=0).to(torch.int64).cumsum(0)
            total = int(ends[-1].item())                    # the one scalar read back per block: it sizes the candidate arrays
            prefix = (ends - counts[lo:hi].clamp(min=0)).contiguous()
            cand_read = torch.empty(total, dtype=torch.int32, device=dev)
            cand_window = torch.empty(total, dtype=torch.int32, device=dev)
            if total:
                B.check(emit(*shape, *reads, counts[lo:hi].data_ptr(), prefix.data_ptr(), 0, cand_read.data_ptr(), cand_window.data_ptr(),
                             a._stream()), "seed_emit_candidates_dev")
            keys = torch.unique(cand_read.to(torch.int64) * n_ids2 + cand_window)      # sorted by (read, id), every pair once
            pair_read = keys // n_ids2
            pair_window = (keys - pair_read * n_ids2).to(torch.int32)
            distance = torch.full((keys.numel(),), -1, dtype=torch.int32, device=dev)
            pair_subject = pair_read + lo
            if keys.numel():
                need = int(L.bgsa_hip_reference_verify_workspace_bytes(W, read_len, keys.numel()))
                if need and (getattr(self, "d_verify_work", None) is None or self.d_verify_work.numel() < need):
                    self.d_verify_work = torch.empty(need, dtype=torch.uint8, device=dev)
                work = self.d_verify_work if need else None
                B.check(verify(self.d_reference.data_ptr(), self.ref_len, W, S, a.d_peq.data_ptr(), *lens_arg, read_len, a.ns, a.wn,
                               pair_window.data_ptr(), pair_subject.data_ptr(), keys.numel(), 0, distance.data_ptr(),
                               None if work is None else work.data_ptr(), 0 if work is None else work.numel(), a._stream()),
                        "reference_verify_pairs_dev")
            segments = torch.searchsorted(pair_read, torch.arange(hi - lo + 1, dtype=torch.int64, device=dev)).contiguous()
            B.check(L.bgsa_hip_seed_select_dev(pair_window.data_ptr() if keys.numel() else None, distance.data_ptr() if keys.numel() else None,
                                               segments.data_ptr(), hi - lo, bound, k_sel, scores[lo:hi].data_ptr(), ids[lo:hi].data_ptr(),
                                               a._stream()), "seed_select_dev")
            emitted += total
            unique += keys.numel()
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
        a = self.aligner
        torch = a.torch
        reads = np.ascontiguousarray(reads, dtype=np.uint8)
        if reads.ndim != 2 or reads.shape[0] < 1 or reads.shape[1] < 1:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: reads must be [ns, n] with ns, n >= 1 (one read length per call)")
        ns, n = reads.shape
        if n > 1024:
            raise B.BgsaHipError("map_reads_seeded: rc=-2: reads beyond 1,024 bp have no verify kernel (map_reads takes them)")
        k_best = int(k_best)
        if not 1 <= k_best <= B.V_NUM:
            raise B.BgsaHipError(f"map_reads_seeded: rc=-1: k_best must lie in 1..{B.V_NUM}")
        if max_distance is None:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: max_distance is required: the seed filter is derived from it (map_reads "
                                 "takes max_distance=None)")
        if int(max_distance) < 0:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: max_distance is negative")
        bound, _, q = seed_plan(n, int(max_distance), seed_len)
        largest = max_stride(self.window_len, n, bound)
        if self.stride > largest:
            allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
            raise B.BgsaHipError(f"map_reads_seeded: rc=-1: at stride {self.stride} a placement of a {n} bp read within distance {bound} can "
                                 f"lie in no window of {self.window_len} bp: {allowed}")
        if self.ref_len > INT32_MAX:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: the index holds int32 positions: a reference beyond 2^31 - 1 bases goes in parts")
        k_sel = self.k_selected(k_best)
        cap = self.window_len + n if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: cigar_cap is not positive")
        max_candidates = max(self.n_ids // SEED_CAP_FRACTION, SEED_MIN_CANDIDATES) if max_candidates is None else int(max_candidates)
        if max_candidates < 0:
            raise B.BgsaHipError("map_reads_seeded: rc=-1: max_candidates is negative")

        # set_subjects(reads, qlen=W), keeping the ASCII rows: the candidate kernels read them
        padded, a.extra = B.pad_rows(reads)
        a.ns_real = ns
        d_rows = torch.from_numpy(B.rows_to_buffer(padded)).to(a.device)
        a.set_subject_rows_device(d_rows, padded.shape[0], n, self.window_len)
        scores, ids, counts, totals = self.select_seeded(d_rows, ns, n, bound, q, k_sel, max_candidates, block_rows)
        strand, ref_begin, ref_end, keep, n_ops, cigar = self.place_hits(ids, bound, cap, block_rows)
        a.check_faults()

        flags = counts.cpu().numpy()
        self.last_seed_stats = dict(reads_seeded=int((flags >= 0).sum()), reads_fallback_n=int((flags == -1).sum()),
                                    reads_fallback_cap=int((flags == -2).sum()), candidates_emitted=int(totals[0].item()),
                                    candidates_unique=int(totals[1].item()), candidates_within_bound=int(totals[2].item()),
                                    seed_len=q, max_candidates=max_candidates)
        kept = keep.cpu().numpy()
        runs_n, runs = n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32)
        cigars = [[None] * k_sel for _ in range(ns)]
        for c, r in zip(*np.nonzero(kept)):
            if runs_n[c, r] > cap:
                raise B.BgsaHipError(f"map_reads_seeded: hit {r} of read {c} has {runs_n[c, r]} runs, its row holds {cap} (raise cigar_cap)")
            cigars[c][r] = "".join(f"{w >> 4}{B.CIGAR_OPS[w & 15]}" for w in runs[c, r, : runs_n[c, r]].tolist())
        out = ReferenceHits(scores.cpu().numpy(), strand.cpu().numpy(), ref_begin.cpu().numpy(), ref_end.cpu().numpy(), kept, cigars,
                            ids.cpu().numpy())
        rest = np.flatnonzero(flags < 0)
        if rest.size:        # the reads the filter does not cover: the exhaustive path, blanked, into the caller's order
            full = blank_beyond(self.map_reads(reads[rest], k_best, int(max_distance), block_rows, cigar_cap), bound)
            for mine, theirs in zip(out[:5] + (out.windows,), full[:5] + (full.windows,)):
                mine[rest] = theirs
            for at, row in zip(rest.tolist(), full.cigars):
                out.cigars[at] = row
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
        a = self.aligner
        torch = a.torch
        rows, lens = B.pad_ragged(reads)
        ns, longest = rows.shape
        if longest > 1024:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-2: reads beyond 1,024 bp have no per-lane form (one length per call: map_reads)")
        k_best = int(k_best)
        if not 1 <= k_best <= B.V_NUM:
            raise B.BgsaHipError(f"map_reads_seeded_ragged: rc=-1: k_best must lie in 1..{B.V_NUM}")
        if max_distance is None:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-1: max_distance is required: the seed filter is derived from it "
                                 "(map_reads_ragged takes max_distance=None)")
        limit = int(max_distance)
        if limit < 0:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-1: max_distance is negative")
        plan = seed_plan_ragged(lens, limit, seed_len)
        largest = max_stride(self.window_len, longest, min(limit, longest))
        if self.stride > largest:
            allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
            raise B.BgsaHipError(f"map_reads_seeded_ragged: rc=-1: at stride {self.stride} a placement of the longest read ({longest} bp) "
                                 f"within distance {min(limit, longest)} can lie in no window of {self.window_len} bp: {allowed}")
        if self.ref_len > INT32_MAX:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-1: the index holds int32 positions: a reference beyond 2^31 - 1 bases goes "
                                 "in parts")
        k_sel = self.k_selected(k_best)
        cap = self.window_len + longest if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-1: cigar_cap is not positive")
        max_candidates = max(self.n_ids // SEED_CAP_FRACTION, SEED_MIN_CANDIDATES) if max_candidates is None else int(max_candidates)
        if max_candidates < 0:
            raise B.BgsaHipError("map_reads_seeded_ragged: rc=-1: max_candidates is negative")

        scores = np.full((ns, k_sel), INT32_MIN, dtype=np.int32)
        strand, windows = np.full_like(scores, -1), np.full_like(scores, -1)
        keep = np.zeros_like(scores)
        ref_begin, ref_end = np.full((ns, k_sel), -1, dtype=np.int64), np.full((ns, k_sel), -1, dtype=np.int64)
        cigars = [[None] * k_sel for _ in range(ns)]
        flags = np.zeros(ns, dtype=np.int32)
        totals, bins = [0, 0, 0], []
        for idx, q in plan:
            mine = lens[idx]
            width, mixed = int(mine.max()), bool((mine != mine[0]).any())
            bound = min(limit, width)
            bins.append(dict(words=(width + 31) // 32, reads=int(idx.size), q=q, emitted=0, unique=0))
            if not mixed and width // (bound + 1) < q:      # a bin of one length too short for its seed: the C call would refuse it
                flags[idx] = -3
                continue
            padded, a.extra = B.pad_rows(rows[idx, :width])
            a.ns_real = int(idx.size)
            d_rows = torch.from_numpy(B.rows_to_buffer(padded)).to(a.device)
            d_lens = None
            if mixed:
                d_lens = torch.from_numpy(np.concatenate([mine, np.full(a.extra, width, dtype=np.int32)]).astype(np.int32)).to(a.device)
            a.set_subject_rows_device(d_rows, padded.shape[0], width, self.window_len, d_lens=d_lens)
            if mixed:
                a.mark_reads_ragged()
            d_scores, d_ids, d_counts, stats = self.select_seeded(d_rows, int(idx.size), width, bound, q, k_sel, max_candidates, block_rows,
                                                                  d_lens=d_lens)
            d_strand, d_begin, d_end, d_keep, d_n_ops, d_cigar = self.place_hits(d_ids, limit, cap, block_rows, ragged=mixed)
            a.check_faults()
            flags[idx] = d_counts.cpu().numpy()
            kept = d_keep.cpu().numpy()
            scores[idx], strand[idx], keep[idx], windows[idx] = d_scores.cpu().numpy(), d_strand.cpu().numpy(), kept, d_ids.cpu().numpy()
            ref_begin[idx], ref_end[idx] = d_begin.cpu().numpy(), d_end.cpu().numpy()
            runs_n, runs = d_n_ops.cpu().numpy(), d_cigar.cpu().numpy().view(np.uint32)
            for c, r in zip(*np.nonzero(kept)):
                if runs_n[c, r] > cap:
                    raise B.BgsaHipError(f"map_reads_seeded_ragged: hit {r} of read {idx[c]} has {runs_n[c, r]} runs, its row holds {cap} "
                                         "(raise cigar_cap)")
                cigars[idx[c]][r] = "".join(f"{w >> 4}{B.CIGAR_OPS[w & 15]}" for w in runs[c, r, : runs_n[c, r]].tolist())
            emitted, unique, within = (int(x.item()) for x in stats)
            bins[-1].update(emitted=emitted, unique=unique)
            totals = [totals[0] + emitted, totals[1] + unique, totals[2] + within]
        out = ReferenceHits(scores, strand, ref_begin, ref_end, keep, cigars, windows)
        rest = np.flatnonzero(flags < 0)
        if rest.size:        # the reads the filter does not cover: the exhaustive path, blanked, into the caller's order
            full = blank_beyond(self.map_reads_ragged([rows[i, : lens[i]] for i in rest], k_best, limit, block_rows, cigar_cap), limit)
            for field, theirs in zip(out[:5] + (out.windows,), full[:5] + (full.windows,)):
                field[rest] = theirs
            for at, row in zip(rest.tolist(), full.cigars):
                out.cigars[at] = row
        self.last_seed_stats = dict(reads_seeded=int((flags >= 0).sum()), reads_fallback_n=int((flags == -1).sum()),
                                    reads_fallback_cap=int((flags == -2).sum()), reads_fallback_short=int((flags == -3).sum()),
                                    candidates_emitted=totals[0], candidates_unique=totals[1], candidates_within_bound=totals[2],
                                    seed_len=None if seed_len is None else int(seed_len), max_candidates=max_candidates, bins=bins)
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
        a = self.aligner
        rows, lens = B.pad_ragged(reads)
        ns, longest = rows.shape
        if longest > 1024:
            raise B.BgsaHipError("map_reads_ragged: rc=-2: reads beyond 1,024 bp have no per-lane form (one length per call: map_reads)")
        k_best = int(k_best)
        if not 1 <= k_best <= B.V_NUM:
            raise B.BgsaHipError(f"map_reads_ragged: rc=-1: k_best must lie in 1..{B.V_NUM}")
        if max_distance is not None and int(max_distance) < 0:
            raise B.BgsaHipError("map_reads_ragged: rc=-1: max_distance is negative")
        bound = 0 if max_distance is None else min(int(max_distance), longest)
        largest = max_stride(self.window_len, longest, bound)
        if self.stride > largest:
            allowed = f"the largest stride allowed is {largest}" if largest >= 1 else "no stride is (a longer window)"
            raise B.BgsaHipError(f"map_reads_ragged: rc=-1: at stride {self.stride} a placement of the longest read ({longest} bp) within "
                                 f"distance {bound} can lie in no window of {self.window_len} bp: {allowed}")
        k_sel = self.k_selected(k_best)
        cap = self.window_len + longest if cigar_cap is None else int(cigar_cap)
        if cap < 1:
            raise B.BgsaHipError("map_reads_ragged: rc=-1: cigar_cap is not positive")

        scores = np.empty((ns, k_sel), dtype=np.int32)
        strand, keep, windows = np.empty_like(scores), np.empty_like(scores), np.empty_like(scores)
        ref_begin, ref_end = np.empty((ns, k_sel), dtype=np.int64), np.empty((ns, k_sel), dtype=np.int64)
        cigars = [[None] * k_sel for _ in range(ns)]
        for idx in B.bin_by_words(lens):
            a.set_reads_ragged([rows[i, : lens[i]] for i in idx], qlen=self.window_len)
            d_scores, d_ids = self.select_windows(k_sel, block_rows)
            limit = None if max_distance is None else int(max_distance)
            if a.reads_ragged:
                d_strand, d_begin, d_end, d_keep, d_n_ops, d_cigar = self.place_hits(d_ids, limit, cap, block_rows, ragged=True)
            else:   # a bin of one length: map_reads' own placement
                if limit is None:
                    limit = -int(a.torch.where(d_ids >= 0, d_scores, a.torch.zeros_like(d_scores)).min().item())
                d_strand, d_begin, d_end, d_keep, d_n_ops, d_cigar = self.place_hits(d_ids, limit, cap, block_rows)
            a.check_faults()
            kept = d_keep.cpu().numpy()
            scores[idx], strand[idx], keep[idx], windows[idx] = d_scores.cpu().numpy(), d_strand.cpu().numpy(), kept, d_ids.cpu().numpy()
            ref_begin[idx], ref_end[idx] = d_begin.cpu().numpy(), d_end.cpu().numpy()
            counts, runs = d_n_ops.cpu().numpy(), d_cigar.cpu().numpy().view(np.uint32)
            for c, r in zip(*np.nonzero(kept)):
                if counts[c, r] > cap:
                    raise B.BgsaHipError(f"map_reads_ragged: hit {r} of read {idx[c]} has {counts[c, r]} runs, its row holds {cap} (raise cigar_cap)")
                cigars[idx[c]][r] = "".join(f"{w >> 4}{B.CIGAR_OPS[w & 15]}" for w in runs[c, r, : counts[c, r]].tolist())
        return ReferenceHits(scores, strand, ref_begin, ref_end, keep, cigars, windows)

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

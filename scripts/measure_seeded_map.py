#!/usr/bin/env python3
"""What seeded read mapping costs, step by step, beside the exhaustive map_reads on the same box in the same run
(profiles/seeded_map.txt), and where the two meet.

    python scripts/measure_seeded_map.py [--out profiles/seeded_map.txt] [--ref-len 10000000] [--reads 100000]
                                         [--window 400] [--stride 239] [--read-len 150] [--bound 12] [--seed-len 11]

One process.  The job of scripts/measure_reference_map.py: a random reference, reads of --read-len bp taken from random places
with two substitutions each, half of them reverse-complemented.  The two results are compared, blanked beyond the bound, before
any time is printed.  HIP events, median of 5:

  index build          bgsa_hip_seed_index_build_dev (once per reference and seed length)
  count + emit         the candidate kernels and the scan between them, all blocks of 1,000 reads
  sort / deduplicate   torch.unique over the (read, window id) keys
  verify               bgsa_hip_reference_verify_pairs_dev over the unique candidates, with the pair row's GCUPS
  select               bgsa_hip_seed_select_dev
  placement            ReferenceMapper.place_hits on the seeded hit lists
  map_reads_seeded     the whole call with its host side, wall clock
  map_reads            the exhaustive call, its selection (select_windows) and placement timed the same way

Break-even: every read of a sample paired with C distinct random windows — what a read from a repeat with C copies emits —, for
C doubling; sort + verify + select per read against the exhaustive selection per read.  The largest n_ids / 2^j below the
crossing is what the default max_candidates should be.
"""
from __future__ import annotations

import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from measure_reference_map import REPS, box_tag, event_ms, make_job  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seeded_map.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--seed-len", type=int, default=11)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=4096, help="reads of the break-even sweep")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    L = B.lib()
    ref, reads, at, strand = make_job(args)
    W, S, n, q = args.window, args.stride, args.read_len, args.seed_len
    mapper = B.ReferenceMapper(ref, W, S)
    a = mapper.aligner
    dev, stream = a.device, a._stream()
    ns, k_sel = reads.shape[0], mapper.k_selected(1)
    bound = B.seed_plan(n, args.bound, q)[0]

    # both whole calls first: the comparison is the check that the job is what it says
    t0 = time.perf_counter()
    full = mapper.map_reads(reads, k_best=1, max_distance=args.bound, cigar_cap=args.cigar_cap)
    wall_full = time.perf_counter() - t0
    mapper.map_reads_seeded(reads[:1000], k_best=1, max_distance=args.bound, seed_len=q, cigar_cap=args.cigar_cap)     # builds the index
    walls = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        seeded = mapper.map_reads_seeded(reads, k_best=1, max_distance=args.bound, seed_len=q, cigar_cap=args.cigar_cap)
        walls.append(time.perf_counter() - t0)
    stats = dict(mapper.last_seed_stats)
    want = B.blank_beyond(full, bound)
    for name in ("scores", "windows", "strand", "ref_begin", "ref_end", "keep"):
        assert np.array_equal(getattr(seeded, name), getattr(want, name)), f"map_reads_seeded differs from the blanked map_reads in {name}"
    assert seeded.cigars == want.cigars, "map_reads_seeded differs from the blanked map_reads in the cigars"
    found = (seeded.keep[:, 0] == 1) & (seeded.strand[:, 0] == strand) & (seeded.ref_begin[:, 0] <= at + 2) & (seeded.ref_end[:, 0] >= at + n - 2)

    lines = ["seeded read mapping, step by step, beside the exhaustive map_reads (scripts/measure_seeded_map.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {S}: {mapper.n_ids:,} ids on two strands; {ns:,} reads of {n} bp, half from each strand, "
             f"B = {args.bound}, q = {q}, k_sel = {k_sel}, blocks of {args.block_rows:,} reads; box {box_tag()}",
             f"the two results agree field by field, blanked beyond B; {int(found.sum()):,} of {ns:,} reads lead with their own locus and strand",
             f"reads seeded {stats['reads_seeded']:,}, N fallbacks {stats['reads_fallback_n']:,}, cap fallbacks {stats['reads_fallback_cap']:,} "
             f"(max_candidates {stats['max_candidates']:,}); candidates per read: emitted {stats['candidates_emitted'] / ns:.1f}, unique "
             f"{stats['candidates_unique'] / ns:.1f}, within the bound {stats['candidates_within_bound'] / ns:.2f}",
             f"HIP events, median (min .. max) of {REPS} runs, one process:"]

    def line(name, m, note=""):
        lines.append(f"  {name:<58s} {m['median']:10.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {note}")

    # index build
    n_offsets = int(L.bgsa_hip_seed_index_offsets(q))
    offsets = torch.empty(n_offsets, dtype=torch.int32, device=dev)
    positions = torch.empty(max(mapper.ref_len - q + 1, 1), dtype=torch.int32, device=dev)
    work = torch.empty(int(L.bgsa_hip_seed_index_workspace_bytes(mapper.ref_len, q)), dtype=torch.uint8, device=dev)
    line(f"index build, q = {q}: {n_offsets:,} offsets", event_ms(torch, lambda: B.check(L.bgsa_hip_seed_index_build_dev(
        mapper.d_reference.data_ptr(), mapper.ref_len, q, offsets.data_ptr(), positions.data_ptr(), work.data_ptr(), work.numel(), stream), "index")))
    del offsets, positions, work

    # the steps of select_seeded, one after the other over all blocks, each kept for the next
    d_rows, _ = a._set_bucket(reads, qlen=W)
    job = mapper.seed_bucket(d_rows, n, bound, q)
    blocks = [(lo, min(lo + args.block_rows, ns)) for lo in range(0, ns, args.block_rows)]
    counts = torch.empty(ns, dtype=torch.int32, device=dev)
    kept = {}
    line("count + emit (with the scan and its scalar read back)", event_ms(torch, lambda: kept.__setitem__(
        "cand", [mapper.seed_candidates(job, lo, hi, stats["max_candidates"], counts) for lo, hi in blocks])))
    line("sort / deduplicate (torch.unique)", event_ms(torch, lambda: kept.__setitem__("pairs", [mapper.seed_dedupe(*cand) for cand in kept["cand"]])))
    n_unique = sum(pair_read.numel() for pair_read, _ in kept["pairs"])
    m_verify = event_ms(torch, lambda: kept.__setitem__(
        "distance", [mapper.seed_verify(job, lo, *pairs) for (lo, _), pairs in zip(blocks, kept["pairs"])]))
    line(f"verify: {n_unique:,} pairs of {n} x {W} cells", m_verify, f"{n_unique * n * W / m_verify['median'] / 1e6:,.0f} GCUPS")
    scores = torch.empty((ns, k_sel), dtype=torch.int32, device=dev)
    ids = torch.empty((ns, k_sel), dtype=torch.int32, device=dev)

    def select():
        for (lo, hi), pairs, distance in zip(blocks, kept["pairs"], kept["distance"]):
            mapper.seed_select(job, lo, hi, *pairs, distance, k_sel, scores, ids)
    line("select (with the segment bounds by searchsorted)", event_ms(torch, select))
    m_place = event_ms(torch, lambda: mapper.place_hits(ids, bound, args.cigar_cap, args.block_rows))
    line(f"placement: {ns * k_sel:,} slots in blocks of {args.block_rows:,} reads", m_place)
    a.check_faults()
    lines.append(f"  map_reads_seeded, the whole call with the host side (wall)       {statistics.median(walls) * 1e3:10.1f} ms  "
                 f"({min(walls) * 1e3:.1f} .. {max(walls) * 1e3:.1f})")

    # the exhaustive path, same run, same box
    m_select = event_ms(torch, lambda: kept.__setitem__("full", mapper.select_windows(k_sel, args.block_rows)), warmup=0)
    m_full_place = event_ms(torch, lambda: mapper.place_hits(kept["full"][1], bound, args.cigar_cap, args.block_rows))
    lines += ["", "the exhaustive map_reads on the same reads:"]
    line(f"selection: {mapper.n_ids:,} windows x {ns:,} reads, top_queries({k_sel})", m_select)
    line(f"placement: {ns * k_sel:,} hits", m_full_place)
    lines.append(f"  map_reads, the whole call with the host side (one run, wall)     {wall_full * 1e3:10.1f} ms   "
                 f"seeded / exhaustive, whole calls: {statistics.median(walls) / wall_full:.3f}")

    # break-even: C distinct random windows per read
    per_read_full = m_select["median"] / ns
    sample = min(args.sample, ns)
    lines += ["", f"break-even, {sample:,} reads, C distinct random windows each; sort + verify + select per read beside the exhaustive "
                  f"selection per read ({per_read_full * 1e3:.2f} us):"]
    rng = np.random.default_rng(args.seed + 1)
    crossing, c = None, 64
    while c <= mapper.n_ids // 2:
        window_np = np.stack([rng.choice(mapper.n_ids, size=c, replace=False) for _ in range(min(sample, 64))])
        window_np = window_np[np.arange(sample) % window_np.shape[0]]
        cand_window = torch.from_numpy(window_np.reshape(-1).astype(np.int32)).to(dev)
        cand_read = torch.arange(sample, dtype=torch.int32, device=dev).repeat_interleave(c)
        out_scores = torch.empty((sample, k_sel), dtype=torch.int32, device=dev)
        out_ids = torch.empty((sample, k_sel), dtype=torch.int32, device=dev)

        def sweep():      # the first `sample` reads of the resident bucket as one block
            pairs = mapper.seed_dedupe(cand_read, cand_window)
            mapper.seed_select(job, 0, sample, *pairs, mapper.seed_verify(job, 0, *pairs), k_sel, out_scores, out_ids)
        m = event_ms(torch, sweep)
        per_read = m["median"] / sample
        lines.append(f"  C = {c:>7,}   {per_read * 1e3:10.2f} us per read  ({m['median']:.3f} ms)   {per_read / per_read_full:.3f} x the exhaustive selection")
        if crossing is None and per_read >= per_read_full:
            crossing = c
        if crossing is not None and c >= 2 * crossing:      # one point beyond the crossing is enough
            break
        c *= 2
    a.check_faults()
    if crossing is None:
        lines.append("  no crossing up to n_ids / 2: the seeded path wins at every C measured")
    else:
        below = crossing // 2
        j = 0
        while mapper.n_ids >> j > below and mapper.n_ids >> j > 1:
            j += 1
        lines.append(f"  the exhaustive selection is reached between C = {below:,} and C = {crossing:,}: n_ids / 2^{j} = {mapper.n_ids >> j:,} is the "
                     f"largest power-of-two fraction of n_ids at which the seeded path was still measured ahead")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

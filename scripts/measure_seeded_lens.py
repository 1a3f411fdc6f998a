#!/usr/bin/env python3
"""What seeded read mapping costs for reads of MIXED lengths, bin by bin and step by step, beside the exhaustive map_reads_ragged
on the same box in the same run (profiles/seeded_lens.txt), and what the per-lane verify instance costs beside the equal-length one.

    python scripts/measure_seeded_lens.py [--out profiles/seeded_lens.txt] [--ref-len 10000000] [--reads 100000]
                                          [--window 400] [--stride 239] [--min-len 100] [--read-len 150] [--bound 12]

One process.  A random reference; reads of --read-len bp taken from random places with two substitutions each, half of them
reverse-complemented (scripts/measure_reference_map.py's job), then trimmed to lengths uniform in --min-len .. --read-len.  The two
results are compared field by field, blanked beyond the bound, before any time is printed.  HIP events, median of 5, per bin of
seed_plan_ragged:

  count + emit         the per-read candidate kernels and the scan between them, all blocks of 1,000 reads
  sort / deduplicate   torch.unique over the (read, window id) keys
  verify (lens)        bgsa_hip_reference_verify_pairs_lens_dev over the unique candidates, with the pair row's GCUPS at the width
  select               bgsa_hip_seed_select_dev
  placement            the placement map_reads_seeded_ragged makes for the bin

then both whole calls with their host side, wall clock, and the lens verify instance with every length --read-len beside the
equal-length instance on the same pairs of the same bucket.
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seeded_lens.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--min-len", type=int, default=100)
    ap.add_argument("--read-len", type=int, default=150, help="the longest read")
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    L = B.lib()
    ref, full_reads, at, strand = make_job(args)
    rng = np.random.default_rng(args.seed + 2)
    lens = rng.integers(args.min_len, args.read_len + 1, size=args.reads)
    # trimming keeps the read's first bases: a reverse-complemented read then covers the END of its source interval
    reads = [full_reads[i, : lens[i]] for i in range(args.reads)]
    W, S, bound = args.window, args.stride, args.bound
    mapper = B.ReferenceMapper(ref, W, S)
    a = mapper.aligner
    dev, stream = a.device, a._stream()
    ns, k_sel = len(reads), mapper.k_selected(1)
    plan = B.seed_plan_ragged(lens, bound)

    # both whole calls first: the comparison is the check that the job is what it says
    t0 = time.perf_counter()
    full = mapper.map_reads_ragged(reads, k_best=1, max_distance=bound, cigar_cap=args.cigar_cap)
    wall_full = time.perf_counter() - t0
    mapper.map_reads_seeded_ragged(reads[:1000], k_best=1, max_distance=bound, cigar_cap=args.cigar_cap)
    for _, q in plan:
        mapper.seed_index(q)                             # every bin's index exists before a wall clock starts
    walls = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        seeded = mapper.map_reads_seeded_ragged(reads, k_best=1, max_distance=bound, cigar_cap=args.cigar_cap)
        walls.append(time.perf_counter() - t0)
    stats = dict(mapper.last_seed_stats)
    want = B.blank_beyond(full, bound)
    for name in ("scores", "windows", "strand", "ref_begin", "ref_end", "keep"):
        assert np.array_equal(getattr(seeded, name), getattr(want, name)), f"map_reads_seeded_ragged differs from the blanked map_reads_ragged in {name}"
    assert seeded.cigars == want.cigars, "map_reads_seeded_ragged differs from the blanked map_reads_ragged in the cigars"
    begin = np.where(strand == 1, at + args.read_len - lens, at)          # where the trimmed read lies on the forward reference
    found = (seeded.keep[:, 0] == 1) & (seeded.strand[:, 0] == strand) & (seeded.ref_begin[:, 0] <= begin + 2) & (seeded.ref_end[:, 0] >= begin + lens - 2)

    lines = ["seeded read mapping for reads of mixed lengths, bin by bin, beside the exhaustive map_reads_ragged (scripts/measure_seeded_lens.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {S}: {mapper.n_ids:,} ids on two strands; {ns:,} reads of {args.min_len}..{args.read_len} bp "
             f"(uniform), half from each strand, B = {bound}, k_sel = {k_sel}, blocks of {args.block_rows:,} reads; box {box_tag()}",
             f"the two results agree field by field, blanked beyond B; {int(found.sum()):,} of {ns:,} reads lead with their own locus and strand",
             f"reads seeded {stats['reads_seeded']:,}, N fallbacks {stats['reads_fallback_n']:,}, cap fallbacks {stats['reads_fallback_cap']:,}, "
             f"short fallbacks {stats['reads_fallback_short']:,} (max_candidates {stats['max_candidates']:,}); candidates per read: emitted "
             f"{stats['candidates_emitted'] / ns:.1f}, unique {stats['candidates_unique'] / ns:.1f}, within the bound "
             f"{stats['candidates_within_bound'] / ns:.2f}",
             f"HIP events, median (min .. max) of {REPS} runs, one process:"]

    def line(name, m, note=""):
        lines.append(f"  {name:<58s} {m['median']:10.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {note}")

    rows_all, _ = B.pad_ragged(reads)
    for (idx, q), seen in zip(plan, stats["bins"]):
        mine = lens[idx].astype(np.int32)
        width, n_bin = int(mine.max()), int(idx.size)
        mixed = bool((mine != mine[0]).any())
        lines += ["", f"bin of {seen['words']} words: {n_bin:,} reads of {int(mine.min())}..{width} bp, q = {q}; emitted {seen['emitted']:,}, unique "
                      f"{seen['unique']:,}"]
        d_rows, d_lens = a._set_bucket(rows_all[idx, :width], mine if mixed else None, qlen=W, reads_ragged=mixed)
        job = mapper.seed_bucket(d_rows, width, min(bound, width), q, d_lens)
        blocks = [(lo, min(lo + args.block_rows, n_bin)) for lo in range(0, n_bin, args.block_rows)]
        counts = torch.empty(n_bin, dtype=torch.int32, device=dev)
        kept = {}
        line("count + emit, per read (with the scan and its read back)", event_ms(torch, lambda: kept.__setitem__(
            "cand", [mapper.seed_candidates(job, lo, hi, stats["max_candidates"], counts) for lo, hi in blocks])))
        flags = counts.cpu().numpy()
        lines.append(f"    flags: seeded {int((flags >= 0).sum()):,}, -1 {int((flags == -1).sum()):,}, -2 {int((flags == -2).sum()):,}, "
                     f"-3 {int((flags == -3).sum()):,}; blocks without a candidate: {sum(1 for c in kept['cand'] if not c[0].numel())}")
        line("sort / deduplicate (torch.unique)", event_ms(torch, lambda: kept.__setitem__("pairs", [mapper.seed_dedupe(*cand) for cand in kept["cand"]])))
        n_unique = sum(pair_read.numel() for pair_read, _ in kept["pairs"])
        m_verify = event_ms(torch, lambda: kept.__setitem__(
            "distance", [mapper.seed_verify(job, lo, *pairs) for (lo, _), pairs in zip(blocks, kept["pairs"])]))
        line(f"verify (lens): {n_unique:,} pairs of <= {width} x {W} cells", m_verify,
             f"{n_unique * width * W / m_verify['median'] / 1e6:,.0f} GCUPS at the width")
        scores = torch.empty((n_bin, k_sel), dtype=torch.int32, device=dev)
        ids = torch.empty((n_bin, k_sel), dtype=torch.int32, device=dev)

        def select():
            for (lo, hi), pairs, distance in zip(blocks, kept["pairs"], kept["distance"]):
                mapper.seed_select(job, lo, hi, *pairs, distance, k_sel, scores, ids)
        line("select (with the segment bounds by searchsorted)", event_ms(torch, select))
        line(f"placement ({'trace_pairs, per read' if mixed else 'banded'}): {n_bin * k_sel:,} slots",
             event_ms(torch, lambda: mapper.place_hits(ids, bound, args.cigar_cap, args.block_rows, ragged=mixed)))
        a.check_faults()

        if width == args.read_len:
            # the lens instance with every length the width beside the equal-length instance: same bucket planes, same pairs, the two
            # C calls side by side
            whole = torch.full((a.ns,), width, dtype=torch.int32, device=dev)

            def verify(*lens_arg):
                call = L.bgsa_hip_reference_verify_pairs_lens_dev if lens_arg else L.bgsa_hip_reference_verify_pairs_dev
                kept["distance"] = []
                for (lo, _), (pair_read, window) in zip(blocks, kept["pairs"]):
                    subject = pair_read + lo
                    distance = torch.full((subject.numel(),), -1, dtype=torch.int32, device=dev)
                    kept["distance"].append(distance)
                    if subject.numel():                      # a block whose reads are all flagged: nothing to verify
                        B.check(call(mapper.d_reference.data_ptr(), mapper.ref_len, W, S, a.d_peq.data_ptr(), *lens_arg, width, a.ns, a.wn,
                                     window.data_ptr(), subject.data_ptr(), subject.numel(), 0, distance.data_ptr(), None, 0, stream), "verify")
            m_whole = event_ms(torch, lambda: verify(whole.data_ptr()))
            got = torch.cat(kept["distance"])
            m_equal = event_ms(torch, verify)
            assert torch.equal(got, torch.cat(kept["distance"])), "the lens instance at the full width differs from the equal-length one"
            lines.append(f"  the same {n_unique:,} pairs with every length {width}: lens instance {m_whole['median']:.3f} ms ({m_whole['min']:.3f} .. "
                         f"{m_whole['max']:.3f}), equal-length instance {m_equal['median']:.3f} ms ({m_equal['min']:.3f} .. {m_equal['max']:.3f}): "
                         f"ratio {m_whole['median'] / m_equal['median']:.3f}")

    lines += ["", f"map_reads_seeded_ragged, the whole call with the host side (wall)  {statistics.median(walls) * 1e3:10.1f} ms  "
                  f"({min(walls) * 1e3:.1f} .. {max(walls) * 1e3:.1f})",
              f"map_reads_ragged, the whole call with the host side (one run, wall) {wall_full * 1e3:10.1f} ms   "
              f"seeded / exhaustive, whole calls: {statistics.median(walls) / wall_full:.3f}"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

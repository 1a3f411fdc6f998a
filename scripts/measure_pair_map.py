#!/usr/bin/env python3
"""What paired-end mapping costs, step by step, beside the two map_reads_seeded calls that exist without it, on the same box in
the same run (profiles/pair_map.txt).

    python scripts/measure_pair_map.py [--out profiles/pair_map.txt] [--ref-len 10000000] [--pairs 100000] [--window 400]
                                       [--stride 239] [--read-len 150] [--bound 6] [--rescue 12] [--insert-min 200] [--insert-max 600]

One process.  The reference of scripts/measure_seeded_map.py; pairs of 2 x --read-len bp cut from random fragments of a length in
the insert range, the forward end upstream, end 1 forward in half of them; two substitutions per end, and in every fifth pair
nine in end 2 — beyond the single-end bound, within the rescue bound.  S = 239 is the largest stride the rule allows at bound 12.
Before any time is printed a fixed sample of pairs is compared with the host model (tests/pair_reference.py): the final lists'
ids and scores from the single-end lists, the rescue windows and a DP over exactly those windows, and the seven outputs of the
pairing rule.  HIP events, median of 5, over all blocks of 1,000 pairs, both ends:

  rescue windows       bgsa_hip_pair_rescue_windows_dev
  union                the own ids and the rescue windows as one list, the unused entries left out
  sort / deduplicate   torch.unique over the (pair, window id) keys
  verify               bgsa_hip_reference_verify_pairs_dev over the unique pairs
  select               bgsa_hip_seed_select_dev at the rescue bound, k_pair slots
  placement            ReferenceMapper.place_hits on the final lists
  pair select          bgsa_hip_pair_select_dev
  map_pairs            the whole call with its host side, wall clock
  2 x map_reads_seeded the two single-end calls, wall clock: the work that exists without the feature
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
sys.path.insert(0, str(ROOT / "tests"))

from measure_reference_map import COMPLEMENT, REPS, box_tag, event_ms, make_job  # noqa: E402


def make_pairs(ref, args):
    rng = np.random.default_rng(args.seed + 2)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    n, ns = args.read_len, args.pairs
    insert = rng.integers(args.insert_min, args.insert_max + 1, size=ns)
    begin = rng.integers(0, ref.size - insert + 1)
    up = ref[begin[:, None] + np.arange(n)[None, :]].copy()
    down = ref[(begin + insert - n)[:, None] + np.arange(n)[None, :]].copy()
    first_forward = np.arange(ns) % 2 == 0
    far = np.arange(ns) % 5 == 4
    ends = [np.where(first_forward[:, None], up, down), np.where(first_forward[:, None], down, up)]
    for e, rows in enumerate(ends):
        for j in range(9):
            hit = np.ones(ns, bool) if j < 2 else far & (e == 1)
            col = rng.integers(n, size=ns)
            new = acgt[rng.integers(4, size=ns)]
            rows[np.flatnonzero(hit), col[hit]] = new[hit]
    reverse = [~first_forward, first_forward]      # the downstream end is the reverse one
    for rows, flip in zip(ends, reverse):
        rows[flip] = COMPLEMENT[rows[flip][:, ::-1]]
    return ends[0], ends[1], begin, insert, far


def host_check(B, mapper, ref, reads, single, paired, args, sample):
    """Stages B and C of the host model on the pairs `sample`: returns how many of them are proper."""
    import pair_reference as P
    import reference_map_reference as M
    import seed_map_reference as S
    from align_reference import classes
    W, stride, L = args.window, args.stride, ref.size
    n_windows, starts = B.window_plan(L, W, stride)
    codes = classes(ref)
    k_pair = paired.end1.scores.shape[1]
    final = (paired.end1, paired.end2)
    for e in (0, 1):
        own, mate = single[e], single[1 - e]
        bound = min(args.rescue, reads[e].shape[1])
        for c in sample:
            ids = {int(g) for g in own.windows[c] if g >= 0}
            for r in np.flatnonzero(mate.keep[c])[:1]:
                lo, hi = B.rescue_region(int(mate.strand[c, r]), int(mate.ref_begin[c, r]), int(mate.ref_end[c, r]), args.insert_max, L)
                meets = np.flatnonzero((starts < hi) & (starts + W > lo))
                assert meets.size <= B.rescue_slots(L, W, stride, args.insert_max)
                ids.update(int((1 - mate.strand[c, r]) * n_windows + w) for w in meets)
            ids = sorted(ids)
            rows = M.window_rows(codes, W, stride, ids).astype(np.int64)
            read = classes(reads[e][c])
            ramp = np.arange(read.size + 1, dtype=np.int64)
            d = np.tile(ramp, (len(ids), 1))
            best = d[:, -1].copy()
            for i in range(W):
                t = np.empty_like(d)
                t[:, 0] = 0
                np.minimum(d[:, 1:] + 1, d[:, :-1] + (rows[:, i: i + 1] != read[None, :]), out=t[:, 1:])
                d = np.minimum.accumulate(t - ramp, axis=1) + ramp
                np.minimum(best, d[:, -1], out=best)
            scores, windows = S.select(ids, best, bound, k_pair)
            assert np.array_equal(final[e].scores[c], scores) and np.array_equal(final[e].windows[c], windows), f"end {e + 1} of pair {c}"
            assert np.array_equal(getattr(paired, f"rescued{e + 1}")[c], P.rescued_of(windows, own.windows[c])), f"end {e + 1} of pair {c}"
    want = P.choose_all(*({f: getattr(h, f)[sample] for f in P.FIELDS} for h in final), args.insert_min, args.insert_max)
    for name in P.OUTPUTS:
        assert np.array_equal(getattr(paired, name)[sample], want[name]), name
    return int(want["proper"].sum())


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pair_map.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=6)
    ap.add_argument("--rescue", type=int, default=12)
    ap.add_argument("--insert-min", type=int, default=200)
    ap.add_argument("--insert-max", type=int, default=600)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=64, help="pairs compared with the host model")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()
    args.reads = 1      # make_job: only its reference is used

    import torch

    import bgsa_amd as B
    ref = make_job(args)[0]
    reads1, reads2, begin, insert, far = make_pairs(ref, args)
    reads = (reads1, reads2)
    W, S, n, ns = args.window, args.stride, args.read_len, args.pairs
    assert B.max_stride(W, n, args.rescue) >= S
    mapper = B.ReferenceMapper(ref, W, S)
    a = mapper.aligner
    kw = dict(k_best=1, max_distance=args.bound, cigar_cap=args.cigar_cap, block_rows=args.block_rows)

    mapper.map_reads_seeded(reads1[:1000], **kw)      # builds the index
    walls_single, walls_pair = [], []
    for _ in range(REPS):
        t0 = time.perf_counter()
        single = [mapper.map_reads_seeded(rows, **kw) for rows in reads]
        walls_single.append(time.perf_counter() - t0)
    for _ in range(REPS):
        t0 = time.perf_counter()
        paired = mapper.map_pairs(reads1, reads2, args.insert_min, args.insert_max, rescue_distance=args.rescue, **kw)
        walls_pair.append(time.perf_counter() - t0)
    stats = dict(mapper.last_pair_stats)
    sample = np.arange(0, ns, max(1, ns // args.sample))[: args.sample]
    sample_proper = host_check(B, mapper, ref, reads, single, paired, args, sample)
    found = (paired.proper == 1) & (paired.insert == insert)
    k_pair = stats["k_pair"]

    lines = ["paired-end mapping, step by step, beside two map_reads_seeded calls (scripts/measure_pair_map.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {S}: {mapper.n_ids:,} ids on two strands; {ns:,} pairs of 2 x {n} bp, insert "
             f"{args.insert_min}..{args.insert_max}, max_distance {args.bound}, rescue_distance {args.rescue}, k_sel = {mapper.k_selected(1)}, "
             f"R = {stats['rescue_slots']}, k_pair = {k_pair}, blocks of {args.block_rows:,} pairs; box {box_tag()}",
             f"{len(sample)} pairs agree with the host model in both final lists and in the seven outputs of the pair ({sample_proper} of them proper)",
             f"proper {stats['proper']:,} of {ns:,} ({int(found.sum()):,} at the planted insert), {stats['proper_through_rescue']:,} only through a "
             f"rescued slot ({int(far.sum()):,} pairs carry an end beyond max_distance); anchors {stats['anchors']:,}, rescue windows "
             f"{stats['rescue_windows']:,}, unique pairs verified {stats['pairs_verified']:,}, slots rescued {stats['slots_rescued']:,}",
             f"HIP events, median (min .. max) of {REPS} runs, one process, both ends:"]

    def line(name, m, note=""):
        lines.append(f"  {name:<58s} {m['median']:10.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {note}")

    # the steps of stage B, end by end, one step after the other over all blocks, each kept for the next
    blocks = [(lo, min(lo + args.block_rows, ns)) for lo in range(0, ns, args.block_rows)]
    totals = {}
    lists = []
    for e in (0, 1):
        bound = min(args.rescue, n)
        d_rows, _ = a._set_bucket(reads[e], None, qlen=W)
        job = mapper.verify_bucket(d_rows, n, bound)
        own_ids = torch.from_numpy(single[e].windows).to(a.device)
        mate = single[1 - e]
        anchors = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(a.device) for x in (mate.strand, mate.ref_begin, mate.ref_end, mate.keep))
        kept = {}
        steps = [("rescue windows", lambda: kept.__setitem__("rescue", [mapper.pair_rescue_windows(anchors, lo, hi, 1, args.insert_max) for lo, hi in blocks])),
                 ("union", lambda: kept.__setitem__("cand", [mapper.pair_union(own_ids[lo:hi], r) for (lo, hi), r in zip(blocks, kept["rescue"])])),
                 ("sort / deduplicate (torch.unique)", lambda: kept.__setitem__("pairs", [mapper.seed_dedupe(*c) for c in kept["cand"]])),
                 ("verify", lambda: kept.__setitem__("distance", [mapper.seed_verify(job, lo, *p) for (lo, _), p in zip(blocks, kept["pairs"])]))]
        scores = torch.empty((ns, k_pair), dtype=torch.int32, device=a.device)
        ids = torch.empty((ns, k_pair), dtype=torch.int32, device=a.device)

        def select():
            for (lo, hi), pairs, distance in zip(blocks, kept["pairs"], kept["distance"]):
                mapper.seed_select(job, lo, hi, *pairs, distance, k_pair, scores, ids)
        steps += [("select (with the segment bounds by searchsorted)", select),
                  ("placement", lambda: kept.__setitem__("placed", mapper.place_hits(ids, bound, args.cigar_cap, args.block_rows)))]
        for name, fn in steps:
            m = event_ms(torch, fn)
            totals[name] = [x + y for x, y in zip(totals.get(name, [0.0, 0.0, 0.0]), (m["median"], m["min"], m["max"]))]
        lists.append((scores, *kept["placed"][:4]))
        assert torch.equal(ids.cpu(), torch.from_numpy((paired.end1, paired.end2)[e].windows)), "the steps do not compose to map_pairs' lists"
    n_unique = stats["pairs_verified"]
    for name, (median, low, high) in totals.items():
        note = f"{n_unique:,} pairs of {n} x {W} cells: {n_unique * n * W / median / 1e6:,.0f} GCUPS" if name == "verify" else ""
        line(name, dict(median=median, min=low, max=high), note)
    line(f"pair select: {ns:,} pairs of {k_pair} x {k_pair} slots", event_ms(torch, lambda: mapper.pair_select(lists[0], lists[1], args.insert_min,
                                                                                                             args.insert_max, args.block_rows)))
    a.check_faults()
    pair_ms, single_ms = statistics.median(walls_pair) * 1e3, statistics.median(walls_single) * 1e3
    lines += [f"  map_pairs, the whole call with the host side (wall)              {pair_ms:10.1f} ms  ({min(walls_pair) * 1e3:.1f} .. {max(walls_pair) * 1e3:.1f})",
              f"  2 x map_reads_seeded at max_distance {args.bound} (wall)                 {single_ms:10.1f} ms  "
              f"({min(walls_single) * 1e3:.1f} .. {max(walls_single) * 1e3:.1f})   map_pairs / the two calls: {pair_ms / single_ms:.2f}"]
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

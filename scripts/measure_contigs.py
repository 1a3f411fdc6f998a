#!/usr/bin/env python3
"""What a reference of several contigs costs beside the same bases as ONE sequence, on the same box in the same run
(profiles/contig_map.txt).

    python scripts/measure_contigs.py [--out profiles/contig_map.txt] [--ref-len 10000000] [--reads 100000] [--contigs 20]
                                      [--window 400] [--stride 239] [--read-len 150] [--bound 12] [--sample 256]

One process.  The shape is scripts/measure_sam.py's: its 100,000 reads of 150 bp (two substitutions, both strands) on its 10 Mbp
reference, k_best = 2, QUAL given.  The baseline is ReferenceMapper.map_reads_sam on the reference as one sequence — the path that
exists without the feature; beside it ContigMapper.map_reads_sam on the same bases cut into 20 contigs of equal length, padding =
the window.  Before any time is printed a fixed sample of the contig records is compared, byte for byte, with the host model
(tests/contig_reference.py) fed with ContigMapper.map_reads_seeded's result for those reads.

  whole call           wall clock of map_reads_sam, five ALTERNATING pairs (one sequence, contigs, one sequence, ...): median
                       (min .. max) of each, and the ratio of the medians.  Expected above 1 by the padding's share of the windows
                       (20 x 400 of 10 M) and one pass over the lists: a few percent, to be read against the baseline's own spread.
  clip kernel          HIP events around bgsa_hip_contig_clip_dev on the lists of the whole batch, as the pipeline calls it
  record stage         HIP events around the list MAPQ, the gather and the two record passes (sam_single_records), both forms
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

from measure_reference_map import REPS, box_tag, event_ms, make_job  # noqa: E402
from measure_sam import Recorder, lines_at  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "contig_map.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--contigs", type=int, default=20)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--seed-len", type=int, default=11)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=256, help="records compared with the host model")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    import contig_reference as C
    from bgsa_amd import reference as R
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns = args.window, args.stride, args.read_len, args.reads
    cuts = np.linspace(0, ref.size, args.contigs + 1).astype(np.int64)
    names = [f"c{i}" for i in range(args.contigs)]
    sequences = [ref[lo:hi].tobytes() for lo, hi in zip(cuts[:-1], cuts[1:])]
    one, cut = B.ReferenceMapper(ref, W, stride), B.ContigMapper(names, sequences, W, stride)
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    kw = dict(k_best=2, max_distance=args.bound, seed_len=args.seed_len, cigar_cap=args.cigar_cap, block_rows=args.block_rows)

    # ---- the sample against the host model, before any time ----------------------------------------------------------------------
    records = cut.map_reads_sam(reads, None, quals, **kw)
    sample = np.arange(0, ns, max(1, ns // args.sample))[: args.sample]
    picked = cut.map_reads_seeded(reads[sample], **kw)
    want = C.single_records(picked, reads[sample], [f"r{c}".encode() for c in sample], quals[sample], sequences, [x.encode() for x in names],
                            args.bound)[0]
    assert lines_at(records, sample) == want, "the sample differs from the host model"
    plain = one.map_reads_sam(reads, None, quals, **kw)
    across = int((plain.flag != records.flag).sum())

    # ---- the whole call, alternating ---------------------------------------------------------------------------------------------
    def wall(mapper):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        mapper.map_reads_sam(reads, None, quals, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    times = {"one": [], "cut": []}
    for _ in range(REPS):
        times["one"].append(wall(one))
        times["cut"].append(wall(cut))

    def stats(xs):
        return dict(median=statistics.median(xs), min=min(xs), max=max(xs))
    m_one, m_cut = stats(times["one"]), stats(times["cut"])

    # ---- the clip kernel and the record stage, by events -----------------------------------------------------------------------------
    lens = np.full(ns, n, dtype=np.int32)
    seen = []
    cut._after_place = lambda *lists: seen.append(tuple(x.clone() for x in lists))      # the lists as place_hits leaves them
    recorded = cut._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    del cut._after_place
    m_clip = event_ms(torch, lambda: [B.ContigMapper._after_place(cut, *lists) for lists in seen])
    for bucket in recorded.buckets:       # the recorded buckets were not clipped: clip them as the pipeline would have
        scores, strand, ref_begin, ref_end, keep, ids = bucket[1]
        B.ContigMapper._after_place(cut, scores, ids, strand, ref_begin, ref_end, keep, bucket[2], bucket[3])
    stage = {}
    for key, mapper in (("one", one), ("cut", cut)):
        rec = recorded if key == "cut" else mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None,
                                                         args.block_rows, args.cigar_cap)
        rname, flat, name_offsets, qual_rows = B.check_sam_call("measure_contigs", lens, None, quals, "ref10M")
        cap = rec.buckets[0][3].shape[2]

        def run(mapper=mapper, rec=rec, cap=cap, flat=flat, name_offsets=name_offsets, rname=rname, qual_rows=qual_rows):
            sink = R.PrimarySink(mapper, ns, cap, args.bound)
            for bucket in rec.buckets:
                sink.add(*bucket)
            return mapper.sam_single_records("measure_contigs", sink, reads, lens, qual_rows, flat, name_offsets, rname)
        stage[key] = event_ms(torch, run)
    cut.aligner.check_faults()

    padding_windows = (cut.n_windows - one.n_windows) / one.n_windows
    lines = ["Reads mapped onto 20 contigs beside the same bases as one sequence (scripts/measure_contigs.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap "
             f"{args.cigar_cap}, QUAL given; {args.contigs} contigs of {len(sequences[0]):,} bp, padding {cut.contig_padding}: "
             f"{cut.n_windows:,} windows beside {one.n_windows:,} (+{100 * padding_windows:.2f} %); box {box_tag()}",
             f"{len(sample)} contig records agree with the host model byte for byte; {int((records.flag != 4).sum()):,} of {ns:,} mapped "
             f"({int((plain.flag != 4).sum()):,} on one sequence; {across:,} records differ in FLAG: reads across a cut)",
             f"map_reads_sam, wall clock, {REPS} alternating pairs, one process: median (min .. max)"]

    def row(name, m, note=""):
        lines.append(f"  {name:<66s} {m['median']:10.1f} ms  ({m['min']:.1f} .. {m['max']:.1f})  {note}")
    row("one sequence: ReferenceMapper.map_reads_sam (the baseline)", m_one, f"spread {100 * (m_one['max'] - m_one['min']) / m_one['median']:.1f} % of the median")
    row("20 contigs: ContigMapper.map_reads_sam", m_cut, f"contigs / one sequence: {m_cut['median'] / m_one['median']:.3f}")
    lines.append(f"by HIP events, median (min .. max) of {REPS}:")
    row("clip kernel, the lists of all reads (bgsa_hip_contig_clip_dev)", m_clip)
    row("record stage, one sequence (mapq, gather, measure, scan, emit, copy)", stage["one"])
    row("record stage, contigs", stage["cut"], f"contigs / one sequence: {stage['cut']['median'] / stage['one']['median']:.3f}")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

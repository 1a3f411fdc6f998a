#!/usr/bin/env python3
"""What marking the duplicates of a call on the device costs beside the same record stage without it, on the same box in the same
run (profiles/markdup.txt).

    python scripts/measure_markdup.py [--out profiles/markdup.txt] [--ref-len 10000000] [--reads 100000] [--window 400]
                                      [--stride 239] [--read-len 150] [--bound 12] [--sample 256] [--share 0.1]

One process.  The job of scripts/measure_bam.py: 100,000 reads of 150 bp on a 10 Mbp reference, mapped once by the seeded pipeline
with k_best = 2, QUAL uniform over '!'..'~' — with a planted share of repeats: the last --share (0.1) of the reads are copies of the
first ones, each with a QUAL of its own, so that many reads are duplicates of an earlier one.  The bucket's device tensors are kept,
so every call starts from the same hits.  Before any time is printed a call of --sample (at least 256) reads, a tenth of them
copies, is marked and compared with the host model's reading of the unmarked call's SAM lines (tests/markdup_reference.py): the
same lines flagged, the same counts; the full job's flags must differ from the unmarked call's in bit 1024 only.  Then

  wall clock  the BAM record stage (stored blocks) with mark_duplicates off and on, the two calls alternating, median and
              min .. max of 5: the baseline is the same call without the option, never a remembered figure
  events      by device events inside the marking calls: the key kernel, the stable sorts with their gathers, the mark kernel
No time is a threshold: the figures are recorded, not claimed in advance.  The Python model is no tuned host baseline and is not
timed.
"""
from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from measure_bam import alternate, summary  # noqa: E402
from measure_reference_map import REPS, box_tag, make_job  # noqa: E402
from measure_sam import RNAME, Recorder  # noqa: E402

STEPS = (("keys", "dup_keys_kernel: end keys, unit scores over QUAL, pair keys"),
         ("sorts", "the stable torch.sort passes by score and key, and the gathers between them"),
         ("mark", "dup_mark_kernel: predecessor compare, 1024 ORed into the flags"))


def plant_copies(reads, quals, share: float) -> int:
    """The last share of the reads become copies of the first ones (their QUAL stays their own); returns their number."""
    copies = int(reads.shape[0] * share)
    if copies:
        reads[-copies:] = reads[:copies]
    return copies


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "markdup.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--seed-len", type=int, default=11)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--block-payload", type=int, default=65280)
    ap.add_argument("--sample", type=int, default=256, help="reads of the call compared with the host model (at least 256)")
    ap.add_argument("--share", type=float, default=0.1, help="the share of the reads that are copies of earlier reads")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    import markdup_reference as MD
    from bgsa_amd import reference as ref_module
    assert torch.cuda.is_available(), "no GPU visible: nothing here can be measured without one"
    assert 0.0 <= args.share <= 0.5, "--share lies in 0 .. 0.5"
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns, P = args.window, args.stride, args.read_len, args.reads, args.block_payload
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    mapper = B.ReferenceMapper(ref, W, stride)
    a, L = mapper.aligner, B.lib()
    lens = np.full(ns, n, dtype=np.int32)

    # ---- the marking agrees with the model before any time is taken -------------------------------------------------------------------
    few = max(args.sample, 256)
    some, some_quals = reads[:few].copy(), quals[:few]
    plant_copies(some, some_quals, args.share)
    call = dict(k_best=2, max_distance=args.bound, seed_len=args.seed_len, cigar_cap=args.cigar_cap)
    plain = mapper.map_reads_sam(some, None, some_quals, RNAME, **call)
    marked = mapper.map_reads_sam(some, None, some_quals, RNAME, mark_duplicates=True, **call)
    text = plain.text.tobytes()
    flagged, want = MD.duplicates_of_sam([text[plain.offsets[i]: plain.offsets[i + 1]] for i in range(few)], False)
    assert set(np.flatnonzero(marked.flag & 1024).tolist()) == flagged and np.array_equal(marked.flag & ~1024, plain.flag), "the flags are not the model's"
    assert mapper.last_duplicate_stats == want, (mapper.last_duplicate_stats, want)
    sample_flagged = len(flagged)

    copies = plant_copies(reads, quals, args.share)
    rname, flat, name_offsets, qual_rows = B.check_bam_call("measure_markdup", lens, None, quals, RNAME, P)
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def stage(**form):
        sink = ref_module.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_markdup", sink, reads, lens, qual_rows, flat, name_offsets, rname, fmt="bam", block_payload=P, **form)

    # ---- device events around the three steps, taken inside the marking calls ------------------------------------------------------------
    pending = {name: [] for name, _ in STEPS}

    def timed(name, fn):
        def wrapper(*args_, **kwargs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args_, **kwargs)
            e1.record()
            pending[name].append((e0, e1))
            return out
        return wrapper
    L.bgsa_hip_dup_keys_dev = timed("keys", L.bgsa_hip_dup_keys_dev)
    mapper.duplicate_order = timed("sorts", mapper.duplicate_order)
    L.bgsa_hip_dup_mark_dev = timed("mark", L.bgsa_hip_dup_mark_dev)

    calls = {"unmarked": lambda: stage(), "marked": lambda: stage(mark_duplicates=True)}
    first = {name: fn() for name, fn in calls.items()}
    stats = dict(mapper.last_duplicate_stats)
    assert np.array_equal(first["marked"].flag & ~1024, first["unmarked"].flag) and not (first["unmarked"].flag & 1024).any()
    assert int((first["marked"].flag & 1024 != 0).sum()) == stats["records_flagged"] >= int(0.9 * copies) and stats["records_skipped"] == 0
    assert np.array_equal(first["marked"].offsets, first["unmarked"].offsets)
    torch.cuda.synchronize()
    for events in pending.values():
        events.clear()                                        # the warm-up calls are not counted
    wall, results = alternate(calls)
    torch.cuda.synchronize()
    events = {name: summary([e0.elapsed_time(e1) for e0, e1 in pairs]) for name, pairs in pending.items()}
    n_events = {name: len(pairs) for name, pairs in pending.items()}
    for name in calls:
        assert results[name].blocks.tobytes() == first[name].blocks.tobytes(), f"{name}: a repeated call gives other bytes"
    a.check_faults()

    lines = ["Duplicate marking on the device, beside the same BAM record stage without it (scripts/measure_markdup.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap {cap}, "
             f"QUAL uniform over 94 values, block_payload {P:,}, stored blocks; box {box_tag()}; one run on one box",
             f"planted: the last {copies:,} reads ({args.share:.0%}) are copies of the first {copies:,}, each with its own QUAL",
             f"{few} reads, {int(few * args.share)} of them copies: the flagged lines ({sample_flagged}) and the counts equal the host model's reading of the "
             f"unmarked SAM lines; the full job: flags differ from the unmarked call's in bit 1024 only, the same bytes on every repeat",
             "counts of the full job: " + ", ".join(f"{key} {value:,}" for key, value in stats.items()),
             f"wall clock of the BAM record stage, the two calls alternating, median (min .. max) of {REPS}, one process:"]
    for name in calls:
        m = wall[name]
        lines.append(f"  {name:<20s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append(f"  marked / unmarked: {wall['marked']['median'] / wall['unmarked']['median']:.2f}")
    lines.append("device events inside the marking calls, median (min .. max):")
    for name, what in STEPS:
        m = events[name]
        lines.append(f"  {what:<88s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  of {n_events[name]}")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

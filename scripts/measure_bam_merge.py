#!/usr/bin/env python3
"""What merging the BAM records of many calls into one coordinate-sorted, indexed result costs beside the one-call sorted stage of the
same reads, on the same box in the same run, and what the gather kernel moves per second (profiles/bam_merge.txt).

    python scripts/measure_bam_merge.py [--out profiles/bam_merge.txt] [--ref-len 10000000] [--reads 100000] [--adds 10]
                                        [--window 400] [--stride 239] [--read-len 150] [--bound 12] [--block-payload 65280]
                                        [--segment-blocks 4096] [--launches 50]

One process.  The job of scripts/measure_bam_sort.py: 100,000 reads of 150 bp on a 10 Mbp reference, mapped once by the seeded pipeline
with k_best = 2, QUAL uniform over '!'..'~', here as --adds batches of equal size; every batch's device tensors are kept, so every
add starts from the same hits.  mark_duplicates=True on both sides.  Before any time is printed the finished merge — stored and
deflated — is compared with the one-call sort=True result of the same reads: the blocks byte for byte, every column, the index
arrays and the .bai bytes.  Then

  wall clock  the one-call sorted stage, the ten adds and finish(), the calls alternating, median and min .. max of 5: the
              comparison is between calls of this run, never with a remembered figure
  events      by device events: an add's append, and inside finish the sort, the marking, the gather kernel, framing or deflate,
              the index — summed per finish
  bandwidth   the gather kernel alone on the whole payload — its output compared with the one-call payload first —, --launches
              launches per event pair, alternating with as many device-to-device copy_ of the same bytes: payload bytes read +
              written per second, and the gather's time as a ratio to the copy's
No time is a threshold: the figures are recorded, not claimed in advance.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from measure_bam import alternate_events, summary  # noqa: E402
from measure_reference_map import REPS, box_tag, make_job  # noqa: E402
from measure_sam import RNAME, Recorder  # noqa: E402

STEPS = (("append", "an add: the emitted payload copied behind the others, the columns kept (of the ten adds, summed)"),
         ("sort", "torch.sort(stable=True) of all keys"),
         ("marking", "duplicate_order + duplicate_marks over all records"),
         ("gather", "bam_gather_kernel: the record bytes into coordinate order, flags patched"),
         ("blocks", "framing, or deflate + scan + pack, of every segment"),
         ("index", "bam_index: marks, chunks, the chunk sort, the suffix minimum, the copies"))


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bam_merge.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--adds", type=int, default=10)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--seed-len", type=int, default=11)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--block-payload", type=int, default=65280)
    ap.add_argument("--segment-blocks", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50, help="launches per event pair in the gather / copy comparison")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bam_reference as M
    import bgsa_amd as B
    from bgsa_amd import reference as ref_module
    assert torch.cuda.is_available(), "no GPU visible: nothing here can be measured without one"
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns, P = args.window, args.stride, args.read_len, args.reads, args.block_payload
    assert ns % args.adds == 0, "--reads is a multiple of --adds"
    per = ns // args.adds
    mapper = B.ReferenceMapper(ref, W, stride)
    a, L = mapper.aligner, B.lib()
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    names = [f"r{i}".encode() for i in range(ns)]              # the names of the one call, so a batch's records are the call's

    class Part:
        """One batch (or all reads): its rows, what check_bam_call returned, the recorded hits."""

        def __init__(self, lo: int, hi: int):
            self.rows, self.lens = reads[lo:hi], np.full(hi - lo, n, dtype=np.int32)
            self.checked = B.check_bam_call("measure_bam_merge", self.lens, names[lo:hi], quals[lo:hi], RNAME, P, True, True, [mapper.ref_len])
            self.recorder = mapper._map_to(lambda *_: Recorder(), self.rows, self.lens, False, 2, args.bound, True, args.seed_len, None,
                                           args.block_rows, args.cigar_cap)
            self.cap = self.recorder.buckets[0][3].shape[2]

        def stage(self, **form):
            rname, flat, name_offsets, qual_rows = self.checked
            sink = ref_module.PrimarySink(mapper, self.rows.shape[0], self.cap, args.bound)
            for bucket in self.recorder.buckets:
                sink.add(*bucket)
            return mapper.sam_single_records("measure_bam_merge", sink, self.rows, self.lens, qual_rows, flat, name_offsets, rname, fmt="bam", **form)
    whole = Part(0, ns)
    parts = [Part(lo, lo + per) for lo in range(0, ns, per)]

    # ---- device events, summed per finish (per merge for the appends) -----------------------------------------------------------------
    pending = {name: [] for name, _ in STEPS}
    state = dict(inside=False)

    def timed(name, fn):
        def wrapper(*args_, **kwargs):
            if not state["inside"]:
                return fn(*args_, **kwargs)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*args_, **kwargs)
            e1.record()
            pending[name][-1].append((e0, e1))
            return out
        return wrapper
    ref_module.BamMerge._append = timed("append", ref_module.BamMerge._append)
    mapper.sort_permutation = timed("sort", mapper.sort_permutation)
    mapper.duplicate_order = timed("marking", mapper.duplicate_order)
    mapper.duplicate_marks = timed("marking", mapper.duplicate_marks)
    L.bgsa_hip_bam_gather_dev = timed("gather", L.bgsa_hip_bam_gather_dev)
    L.bgsa_hip_bgzf_frame_dev = timed("blocks", L.bgsa_hip_bgzf_frame_dev)
    mapper.bgzf_deflated = timed("blocks", mapper.bgzf_deflated)
    mapper.bam_index = timed("index", mapper.bam_index)

    def one_call(compress: bool):
        return whole.stage(block_payload=P, compress=compress, sort=True, mark_duplicates=True)

    def merged(compress: bool) -> tuple:
        """(the finished records, the wall ms of the adds, the wall ms of finish, the merge), its steps under events."""
        for events in pending.values():
            events.append([])
        state["inside"] = True
        merge = mapper.bam_merge(block_payload=P, compress=compress, mark_duplicates=True, segment_blocks=args.segment_blocks)
        t0 = time.perf_counter()
        for part in parts:
            part.stage(merge=merge)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        got = merge.finish()
        t2 = time.perf_counter()
        state["inside"] = False
        return got, (t1 - t0) * 1e3, (t2 - t1) * 1e3, merge

    # ---- the merge equals the one call before any time is taken -----------------------------------------------------------------------
    stats = {}
    for compress in (False, True):
        want = one_call(compress)
        stats[compress] = dict(mapper.last_duplicate_stats)
        got = merged(compress)[0]
        assert got.blocks.tobytes() == want.blocks.tobytes(), f"compress={compress}: the merged blocks are not the one call's"
        for name in B.SortedBamRecords._fields[1:-1]:
            assert np.array_equal(getattr(got, name), getattr(want, name)), f"compress={compress}: {name} differs"
        assert all(np.array_equal(x, y) for x, y in zip(got.index, want.index)), f"compress={compress}: the index arrays differ"
        assert B.bai_bytes(got.index, got.flag, got.ref_id, 99) == B.bai_bytes(want.index, want.flag, want.ref_id, 99)
        assert mapper.last_duplicate_stats == stats[compress], f"compress={compress}: the duplicate counters differ"
    total = int(want.offsets[-1])
    for events in pending.values():
        events.clear()                                        # the comparison runs are the warm-up and are not counted

    wall = {name: [] for name in ("one call, stored", "ten adds, stored", "finish, stored", "one call, deflate", "ten adds, deflate", "finish, deflate")}
    for _ in range(REPS):
        for compress, tag in ((False, "stored"), (True, "deflate")):
            t0 = time.perf_counter()
            one_call(compress)
            wall[f"one call, {tag}"].append((time.perf_counter() - t0) * 1e3)
            _, adds_ms, finish_ms, _ = merged(compress)
            wall[f"ten adds, {tag}"].append(adds_ms)
            wall[f"finish, {tag}"].append(finish_ms)
    torch.cuda.synchronize()
    events = {}
    for name, runs in pending.items():
        for k, tag in ((0, "stored"), (1, "deflate")):        # the runs alternate: stored, deflate, stored, ...
            sums = [sum(e0.elapsed_time(e1) for e0, e1 in run) for run in runs[k::2] if run]
            if sums:
                events[name, tag] = summary(sums)

    # ---- the gather kernel beside a device copy of the same bytes: the whole payload in one window, --launches launches per event pair,
    # the two alternating; the replayed call's output is the one-call payload before a time is taken -------------------------------------
    got, _, _, merge = merged(False)
    order, dst_offsets = torch.from_numpy(got.order).to(a.device), torch.from_numpy(got.offsets).to(a.device)
    lengths = torch.empty(ns, dtype=torch.int64, device=a.device)
    lengths[order] = dst_offsets[1:] - dst_offsets[:-1]
    src_offsets = torch.zeros(ns + 1, dtype=torch.int64, device=a.device)
    src_offsets[1:] = torch.cumsum(lengths, 0)
    flag = torch.empty(ns, dtype=torch.int32, device=a.device)
    flag[order] = torch.from_numpy(got.flag).to(a.device)
    out, other = torch.zeros(total, dtype=torch.uint8, device=a.device), torch.empty(total, dtype=torch.uint8, device=a.device)
    refused = torch.zeros(1, dtype=torch.int32, device=a.device)
    gather_call = L.bgsa_hip_bam_gather_dev

    def gather_once():
        B.check(gather_call(merge.payload.data_ptr(), total, src_offsets.data_ptr(), ns, order.data_ptr(), dst_offsets.data_ptr(), ns, 0, ns, 0, total,
                            flag.data_ptr(), out.data_ptr(), refused.data_ptr(), a._stream()), "bam_gather_dev")
    gather_once()
    assert out.cpu().numpy().tobytes() == b"".join(M.walk_blocks(got.blocks.tobytes())) and int(refused.item()) == 0, "the replayed gather differs"
    many = {"gather": lambda: [gather_once() for _ in range(args.launches)], "copy": lambda: [other.copy_(out) for _ in range(args.launches)]}
    per_launch = {name: {k: v / args.launches for k, v in m.items()} for name, m in alternate_events(torch, many, reps=max(REPS, 5)).items()}
    a.check_faults()

    lines = ["BAM records of many calls merged into one coordinate-sorted, indexed result, beside the one-call sorted stage (scripts/measure_bam_merge.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp as {args.adds} adds of {per:,}, max_distance {args.bound}, "
             f"k_best 2, QUAL uniform over 94 values, block_payload {P:,}, segment_blocks {args.segment_blocks:,}, mark_duplicates=True; "
             f"box {box_tag()}; one run on one box",
             f"the finished merge equals the one-call sort=True result of the same reads — blocks byte for byte, columns, index arrays, .bai, "
             f"duplicate counters ({stats[False]['records_flagged']:,} records flagged) — stored and deflated; payload {total:,} bytes",
             f"wall clock, the calls alternating, median (min .. max) of {REPS}, one process:"]
    for name, times in wall.items():
        m = summary(times)
        lines.append(f"  {name:<20s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append("device events, summed per merge, median (min .. max):")
    for name, what in STEPS:
        for tag in ("stored", "deflate"):
            if (name, tag) in events:
                m = events[name, tag]
                lines.append(f"  {tag:<8s} {what:<100s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})")
    gather, copy = per_launch["gather"], per_launch["copy"]
    lines.append(f"the gather kernel alone, the whole payload in one window, {args.launches} launches per event pair, alternating with as many "
                 f"device-to-device copy_ of the same {total:,} bytes, median (min .. max) of {max(REPS, 5)} per launch:")
    lines.append(f"  gather {gather['median']:.4f} ms ({gather['min']:.4f} .. {gather['max']:.4f}), {2 * total / gather['median'] / 1e6:.1f} GB/s of payload "
                 f"(read + written); copy_ {copy['median']:.4f} ms ({copy['min']:.4f} .. {copy['max']:.4f}), {2 * total / copy['median'] / 1e6:.1f} GB/s: "
                 f"the gather takes {gather['median'] / copy['median']:.2f}x a copy")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

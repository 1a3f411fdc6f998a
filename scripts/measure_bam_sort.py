#!/usr/bin/env python3
"""What sorting a call's BAM records by coordinate and building their BAI index on the device costs beside the unsorted stage of the
same records, on the same box in the same run (profiles/bam_sort.txt).

    python scripts/measure_bam_sort.py [--out profiles/bam_sort.txt] [--ref-len 10000000] [--reads 100000] [--window 400]
                                       [--stride 239] [--read-len 150] [--bound 12] [--sample 256] [--block-payload 65280]

One process.  The job of scripts/measure_bam.py: 100,000 reads of 150 bp on a 10 Mbp reference, mapped once by the seeded pipeline
with k_best = 2, QUAL uniform over '!'..'~'; the bucket's device tensors are kept, so every call starts from the same hits.  Before
any time is printed a call of --sample (at least 256) reads with sort=True, stored and deflated, is inflated and decoded on the host,
its records must be the unsorted call's in key order, and its index arrays and .bai bytes must equal the host model's
(tests/bai_reference.py); the full job's sorted records must be a permutation of the unsorted ones with keys in order.  Then

  wall clock  the record stage with sort=False and sort=True, compress=False and compress=True, the four calls alternating, median
              and min .. max of 5: the comparison is between calls of this run, never with a remembered figure
  events      by device events inside the sort=True calls: the key kernel, torch.sort, the gather of the per-record tensors, the
              marks kernel and the chunks kernel
No time is a threshold: the figures are recorded, not claimed in advance.
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

STEPS = (("coordinates", "bam_coordinates_kernel: key, refID, pos, end, bin of every record"),
         ("sort", "torch.sort(key, stable=True)"),
         ("gather", "the per-record tensors and the coordinates gathered by the permutation"),
         ("marks", "bam_index_marks_kernel: virtual offsets, chunk starts, the linear minima by atomicMin"),
         ("chunks", "bam_index_chunks_kernel: ref, bin, begin and end of every chunk"))


def check_against_the_model(B, M, R, got, plain, ref_len: int, P: int, compress: bool, what: str) -> None:
    """The sorted call's records are the unsorted call's in key order, and its index and .bai are the model's."""
    blocks = got.blocks.tobytes()
    records = M.split_records(b"".join(M.walk_blocks(blocks, stored=not compress)))
    unsorted = M.split_records(b"".join(M.walk_blocks(plain.blocks.tobytes())))
    assert records == [unsorted[i] for i in got.order], f"{what}: the sorted records are not the unsorted ones permuted"
    coords = [R.decoded_coordinates(M.decode(x, [RNAME])) for x in records]
    keys = [c[0] for c in coords]
    assert all(a < b or (a == b and i < j) for a, b, i, j in zip(keys, keys[1:], got.order, got.order[1:])), f"{what}: the keys are not in stable order"
    starts, at = [0], 0
    while at < len(blocks):
        at += int.from_bytes(blocks[at + 16: at + 18], "little") + 1
        starts.append(at)
    want = R.build_index([c[1] for c in coords], [c[2] for c in coords], [c[3] for c in coords], [c[4] for c in coords], got.offsets, P,
                         starts if compress else None, [ref_len])
    index = got.index
    assert list(zip(index.chunk_ref.tolist(), index.chunk_bin.tolist(), index.chunk_beg.tolist(), index.chunk_end.tolist())) == want["chunks"], what
    assert index.linear.tolist() == want["linear"] and index.n_intv.tolist() == want["n_intv"] and index.window_base.tolist() == want["window_base"], what
    assert B.bai_bytes(index, got.flag, got.ref_id, 99) == R.bai_bytes(want, got.flag.tolist(), got.ref_id.tolist(), 99), f"{what}: the .bai bytes differ"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bam_sort.txt"))
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
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bai_reference as R
    import bam_reference as M
    import bgsa_amd as B
    from bgsa_amd import reference as ref_module
    assert torch.cuda.is_available(), "no GPU visible: nothing here can be measured without one"
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns, P = args.window, args.stride, args.read_len, args.reads, args.block_payload
    mapper = B.ReferenceMapper(ref, W, stride)
    a, L = mapper.aligner, B.lib()
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    lens = np.full(ns, n, dtype=np.int32)

    # ---- the index agrees with the model before any time is taken ---------------------------------------------------------------------
    few = max(args.sample, 256)
    call = dict(k_best=2, max_distance=args.bound, seed_len=args.seed_len, cigar_cap=args.cigar_cap, block_payload=P)
    plain = mapper.map_reads_bam(reads[:few], None, quals[:few], RNAME, **call)
    for compress in (False, True):
        got = mapper.map_reads_bam(reads[:few], None, quals[:few], RNAME, compress=compress, sort=True, **call)
        check_against_the_model(B, M, R, got, plain, mapper.ref_len, P, compress, f"{few} reads, compress={compress}")

    rname, flat, name_offsets, qual_rows = B.check_bam_call("measure_bam_sort", lens, None, quals, RNAME, P, True, True, [mapper.ref_len])
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def stage(**form):
        sink = ref_module.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_bam_sort", sink, reads, lens, qual_rows, flat, name_offsets, rname, fmt="bam", block_payload=P, **form)

    # ---- device events around the five steps, taken inside the sort=True calls ----------------------------------------------------------
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
    mapper.bam_coordinates = timed("coordinates", mapper.bam_coordinates)
    mapper.sort_permutation = timed("sort", mapper.sort_permutation)
    mapper.gather_records = timed("gather", mapper.gather_records)
    L.bgsa_hip_bam_index_marks_dev = timed("marks", L.bgsa_hip_bam_index_marks_dev)
    L.bgsa_hip_bam_index_chunks_dev = timed("chunks", L.bgsa_hip_bam_index_chunks_dev)

    calls = {"stored": lambda: stage(), "stored, sorted": lambda: stage(sort=True), "deflate": lambda: stage(compress=True),
             "deflate, sorted": lambda: stage(compress=True, sort=True)}
    first = {name: fn() for name, fn in calls.items()}
    for name in ("stored", "deflate"):
        got, base = first[name + ", sorted"], first[name]
        assert sorted(got.order.tolist()) == list(range(ns)) and np.array_equal(got.flag, base.flag[got.order]), name
        assert np.array_equal(np.diff(got.offsets), np.diff(base.offsets)[got.order]) and np.array_equal(got.pos, base.pos[got.order]), name
        key = np.where(got.ref_id < 0, 0x7fffffff, got.ref_id).astype(np.int64) << 32 | got.pos << 1 | (got.flag >> 4 & 1)
        assert (np.diff(key) >= 0).all() and (np.diff(got.order)[np.diff(key) == 0] > 0).all(), f"{name}: the keys are not in stable order"
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
    index = results["stored, sorted"].index
    bai = B.bai_bytes(index, results["stored, sorted"].flag, results["stored, sorted"].ref_id, 0)

    lines = ["BAM records sorted by coordinate with a BAI index built on the device, beside the unsorted stage (scripts/measure_bam_sort.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap {cap}, "
             f"QUAL uniform over 94 values, block_payload {P:,}; box {box_tag()}; one run on one box",
             f"{few} reads: the sorted records are the unsorted call's in stable key order, the index arrays and the .bai bytes equal the host "
             f"model's, stored and deflated; the full job: a permutation with keys in order, the same bytes on every repeat",
             f"index: {index.chunk_ref.size:,} chunks, {int(index.n_intv.sum()):,} of {index.linear.size:,} windows written, the .bai {len(bai):,} bytes; "
             f"{int((results['stored, sorted'].ref_id < 0).sum()):,} records without coordinates",
             f"wall clock of the BAM record stage, the four calls alternating, median (min .. max) of {REPS}, one process:"]
    for name in calls:
        m = wall[name]
        lines.append(f"  {name:<20s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append(f"  sorted / unsorted: stored {wall['stored, sorted']['median'] / wall['stored']['median']:.2f}, "
                 f"deflate {wall['deflate, sorted']['median'] / wall['deflate']['median']:.2f}")
    lines.append("device events inside the sort=True calls, median (min .. max):")
    for name, what in STEPS:
        m = events[name]
        lines.append(f"  {what:<96s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  of {n_events[name]}")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

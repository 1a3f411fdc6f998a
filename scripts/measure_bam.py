#!/usr/bin/env python3
"""What the BAM stage costs beside the SAM stage of the same records, on the same box in the same run (profiles/bam_records.txt).

    python scripts/measure_bam.py [--out profiles/bam_records.txt] [--ref-len 10000000] [--reads 100000] [--window 400] [--stride 239]
                                  [--read-len 150] [--bound 12] [--sample 256] [--block-payload 65280]

One process.  The 100,000 reads of scripts/measure_sam.py (150 bp, two substitutions, both strands) on its 10 Mbp reference, mapped
once by the seeded pipeline with k_best = 2; the bucket's device tensors are kept, so both stages start from the same hits.  Before
any time is printed a fixed sample of BAM records is inflated, decoded by the host model (tests/bam_reference.py) and compared with
the lines of the SAM text, byte for byte.  The calls alternate — SAM, BAM, SAM, BAM, ... —, median and min .. max of 5:

  SAM stage   the list MAPQ and the primaries gathered, measure, scan, emit, the text and the four columns copied to the host
              (ReferenceMapper.sam_single_records): the path that exists without the feature
  BAM stage   the same with fmt="bam": measure, scan, emit, the BGZF framing, the blocks and the four columns copied
  passes      by device events around the calls inside the stages: the measure and the emit pass of either format
  framing     by device events: bgsa_hip_bgzf_frame_dev alone on the payload of that call, and its payload bytes per second beside a
              device-to-device copy of the same bytes taken in the same loop
No time is a threshold: the figures are recorded, not claimed in advance.
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

from measure_reference_map import REPS, box_tag, make_job  # noqa: E402
from measure_sam import RNAME, Recorder  # noqa: E402


def summary(times) -> dict:
    return dict(median=statistics.median(times), min=min(times), max=max(times))


def alternate(calls: dict, reps: int = REPS) -> tuple:
    """Every call once to warm up, then reps rounds in which the calls follow one another: ({name: times in ms}, {name: last result})."""
    results = {name: fn() for name, fn in calls.items()}
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            t0 = time.perf_counter()
            results[name] = fn()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: summary(t) for name, t in times.items()}, results


def alternate_events(torch, calls: dict, reps: int = REPS) -> dict:
    """The same by device events around each call."""
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in calls}
    for _ in range(reps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    return {name: summary(t) for name, t in times.items()}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bam_records.txt"))
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
    ap.add_argument("--sample", type=int, default=256, help="records decoded and compared with the SAM text (at least 256)")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bam_reference as M
    import bgsa_amd as B
    from bgsa_amd import reference as R
    assert torch.cuda.is_available(), "no GPU visible: nothing here can be measured without one"
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns, P = args.window, args.stride, args.read_len, args.reads, args.block_payload
    mapper = B.ReferenceMapper(ref, W, stride)
    a = mapper.aligner
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    lens = np.full(ns, n, dtype=np.int32)
    rname, flat, name_offsets, qual_rows = B.check_bam_call("measure_bam", lens, None, quals, RNAME, P)
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def stage(**form):
        sink = R.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_bam", sink, reads, lens, qual_rows, flat, name_offsets, rname, **form)

    # ---- the records agree before any time is taken ---------------------------------------------------------------------------
    sam, bam = stage(), stage(fmt="bam", block_payload=P)
    payload = b"".join(M.walk_blocks(bam.blocks.tobytes()))
    assert payload and len(payload) == int(bam.offsets[-1]) and len(bam.blocks) == len(payload) + 31 * -(-len(payload) // P)
    sample = np.arange(0, ns, max(1, ns // max(args.sample, 256)))[: max(args.sample, 256)]
    text = sam.text.tobytes()
    for i in sample:
        line = M.decode(payload[bam.offsets[i]: bam.offsets[i + 1]], [RNAME])["line"]
        assert line == text[sam.offsets[i]: sam.offsets[i + 1]], f"record {i} decodes to another line than the SAM stage wrote"
    for name in ("flag", "pos", "mapq", "nm"):
        assert np.array_equal(getattr(sam, name), getattr(bam, name)), name

    # ---- the two stages, alternating ------------------------------------------------------------------------------------------------
    wall, results = alternate({"sam": stage, "bam": lambda: stage(fmt="bam", block_payload=P)})
    assert results["bam"].blocks.tobytes() == bam.blocks.tobytes() and results["sam"].text.tobytes() == text, "a repeated call gives other bytes"

    # ---- the two record passes of either format, by device events around the calls inside the stage -----------------------------
    spans, plain_passes = [], mapper._sam_passes

    def timed_passes(fmt="sam"):
        def timed(name, call):
            def run(*call_args):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                rc = call(*call_args)
                e1.record()
                spans.append((f"{fmt} {name}", e0, e1))
                return rc
            return run
        measure, emit = plain_passes(fmt)
        return timed("measure", measure), timed("emit", emit)
    mapper._sam_passes = timed_passes
    try:
        for _ in range(REPS):
            stage()
            stage(fmt="bam", block_payload=P)
    finally:
        del mapper._sam_passes
    torch.cuda.synchronize()
    passes = {name: summary([e0.elapsed_time(e1) for which, e0, e1 in spans if which == name]) for name in sorted({s[0] for s in spans})}

    # ---- the framing kernel alone, beside a device-to-device copy of the same bytes ---------------------------------------------
    d_payload = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(a.device)
    framed = int(B.lib().bgsa_hip_bgzf_framed_bytes(len(payload), P))
    d_out, d_copy = torch.empty(framed, dtype=torch.uint8, device=a.device), torch.empty(len(payload), dtype=torch.uint8, device=a.device)

    def frame():
        B.check(B.lib().bgsa_hip_bgzf_frame_dev(d_payload.data_ptr(), len(payload), P, d_out.data_ptr(), framed, a._stream()), "bgzf_frame_dev")
    events = alternate_events(torch, {"frame": frame, "copy": lambda: d_copy.copy_(d_payload)})
    assert d_out.cpu().numpy().tobytes() == bam.blocks.tobytes(), "the framing alone gives other blocks than the stage"
    a.check_faults()

    mapped = int((sam.flag != 4).sum())
    lines = ["BAM records and BGZF blocks written on the device, beside the SAM stage of the same records (scripts/measure_bam.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap {cap}, "
             f"QUAL given, block_payload {P:,}; box {box_tag()}; one run on one box",
             f"{len(sample)} BAM records, inflated and decoded on the host, equal their SAM lines byte for byte; the four columns are equal; "
             f"{mapped:,} of {ns:,} reads mapped",
             f"bytes: SAM text {sam.text.size:,} ({sam.text.size / ns:.0f} per record); BAM payload {len(payload):,} ({len(payload) / ns:.0f} per "
             f"record), {framed:,} in {-(-len(payload) // P):,} BGZF blocks of stored deflate ({framed / sam.text.size:.2f} of the text)",
             f"wall clock, the calls alternating, median (min .. max) of {REPS}, one process:"]
    for name, what in (("sam", "SAM stage: mapq + gather, measure, scan, emit, copy of the text"),
                       ("bam", "BAM stage: mapq + gather, measure, scan, emit, frame, copy of the blocks")):
        m = wall[name]
        lines.append(f"  {what:<74s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append(f"  BAM stage / SAM stage: {wall['bam']['median'] / wall['sam']['median']:.2f}")
    lines.append(f"device events around the record passes inside the stages, alternating, median (min .. max) of {REPS}:")
    for name, m in passes.items():
        lines.append(f"  {name + ' pass':<74s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})")
    lines.append(f"device events, alternating, median (min .. max) of {REPS}, on the {len(payload):,} payload bytes:")
    for name, what in (("frame", "bgzf_frame_kernel: copy + CRC-32 + 31 bytes of framing per block"), ("copy", "device-to-device copy of the payload")):
        m = events[name]
        lines.append(f"  {what:<74s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {len(payload) / m['median'] / 1e6:8.1f} GB/s of payload")
    lines.append(f"  framing / copy: {events['frame']['median'] / events['copy']['median']:.1f}")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

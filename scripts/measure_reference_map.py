#!/usr/bin/env python3
"""What mapping reads onto a reference costs, piece by piece, beside the same job through host-cut windows
(profiles/reference_map.txt).

    python scripts/measure_reference_map.py [--out profiles/reference_map.txt] [--ref-len 10000000] [--reads 100000]
                                            [--window 400] [--stride 239] [--read-len 150] [--bound 12]

One process.  A random reference, reads of --read-len bp taken from random places with two substitutions each, half of them
reverse-complemented.  HIP events around each piece, median of 5:

  windows, range form     every window id of both strands written as query rows (bgsa_hip_reference_windows_dev)
  windows, id-list form   the k_sel hit windows of every read gathered by id
  device-to-device copy   of the same number of bytes as each of the two: the yardstick for the window kernel
  selection               ReferenceMapper.select_windows: rows built segment by segment, scored, top_queries
  placement               ReferenceMapper.place_hits: gather, place_pairs_banded, reference coordinates, block by block
  placements kernel       bgsa_hip_reference_placements_dev alone over all reads
  parent's API            windows cut on the host (forward strand only), set_queries, top_queries, place_pairs_banded — the
                          steps of place_top_queries_banded — with the host cut and the upload timed apart (wall clock)

The default stride is the largest the completeness rule allows for these reads, max_stride(400, 150, 12) = 239.
"""
from __future__ import annotations

import argparse
import hashlib
import socket
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

REPS = 5
COMPLEMENT = np.zeros(256, np.uint8)
COMPLEMENT[list(b"ACGT")] = list(b"TGCA")


def box_tag() -> str:
    """Which box a line was measured on, without naming it: runs on one box carry one tag."""
    return hashlib.sha1(socket.gethostname().encode()).hexdigest()[:6]


def event_ms(torch, fn, reps: int = REPS, warmup: int = 1) -> dict:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median": statistics.median(out), "min": min(out), "max": max(out)}


def make_job(args):
    rng = np.random.default_rng(args.seed)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    ref = acgt[rng.integers(4, size=args.ref_len)]
    at = rng.integers(0, args.ref_len - args.read_len + 1, size=args.reads)
    reads = ref[at[:, None] + np.arange(args.read_len)[None, :]].copy()
    for _ in range(2):
        col = rng.integers(args.read_len, size=args.reads)
        reads[np.arange(args.reads), col] = acgt[rng.integers(4, size=args.reads)]
    strand = (np.arange(args.reads) % 2).astype(np.int32)
    reads[strand == 1] = COMPLEMENT[reads[strand == 1][:, ::-1]]
    return ref, reads, at, strand


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "reference_map.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    L = B.lib()
    ref, reads, at, strand = make_job(args)
    W, S, n = args.window, args.stride, args.read_len
    mapper = B.ReferenceMapper(ref, W, S)
    a = mapper.aligner
    stream = a._stream()
    k_sel = mapper.k_selected(1)
    ns = reads.shape[0]
    lines = ["reads mapped onto a reference, piece by piece (scripts/measure_reference_map.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {S} (max_stride {B.max_stride(W, n, args.bound)}): {mapper.n_windows:,} windows, "
             f"{mapper.n_ids:,} ids on two strands; {ns:,} reads of {n} bp, half from each strand, B = {args.bound}, k_sel = {k_sel}; box {box_tag()}",
             f"HIP events, median (min .. max) of {REPS} runs, one process:"]

    def line(name, m, note=""):
        lines.append(f"  {name:<58s} {m['median']:10.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {note}")

    # the whole call first: it is also the check that the job is what it says
    t0 = time.perf_counter()
    hits = mapper.map_reads(reads, k_best=1, max_distance=args.bound, cigar_cap=args.cigar_cap)
    wall_map = time.perf_counter() - t0
    found = (hits.keep[:, 0] == 1) & (hits.strand[:, 0] == strand) & (hits.ref_begin[:, 0] <= at + 2) & (hits.ref_end[:, 0] >= at + n - 2)
    lines.append(f"  map_reads, the whole call with the host side (one run, wall)   {wall_map * 1e3:10.1f} ms   "
                 f"{int(found.sum()):,} of {ns:,} reads lead with their own locus and strand")

    # window rows
    range_bytes = mapper.n_ids * (W + 1)
    d_range = torch.zeros(range_bytes + 8, dtype=torch.uint8, device=a.device)
    d_copy = torch.zeros(range_bytes + 8, dtype=torch.uint8, device=a.device)

    def build(d_ids, rows, out):
        B.check(L.bgsa_hip_reference_windows_dev(mapper.d_reference.data_ptr(), mapper.ref_len, W, S, None if d_ids is None else d_ids.data_ptr(),
                                                 0, rows, out.data_ptr(), stream), "reference_windows_dev")
    m_range = event_ms(torch, lambda: build(None, mapper.n_ids, d_range))
    m_copy = event_ms(torch, lambda: d_copy[:range_bytes].copy_(d_range[:range_bytes]))
    line("windows, range form", m_range, f"{range_bytes / 1e6:.1f} MB written, {range_bytes / m_range['median'] / 1e6:.0f} GB/s")
    line("  device-to-device copy of as many bytes", m_copy, f"{m_range['median'] / m_copy['median']:.2f} x the copy")
    del d_range, d_copy

    a.set_subjects(reads, qlen=W)
    scores, ids = mapper.select_windows(k_sel)
    list_bytes = ns * k_sel * (W + 1)
    d_list = torch.zeros(list_bytes + 8, dtype=torch.uint8, device=a.device)
    d_copy = torch.zeros(list_bytes + 8, dtype=torch.uint8, device=a.device)
    m_list = event_ms(torch, lambda: build(ids, ns * k_sel, d_list))
    m_copy = event_ms(torch, lambda: d_copy[:list_bytes].copy_(d_list[:list_bytes]))
    line("windows, id-list form (the hit windows of every read)", m_list, f"{list_bytes / 1e6:.1f} MB written, {list_bytes / m_list['median'] / 1e6:.0f} GB/s")
    line("  device-to-device copy of as many bytes", m_copy, f"{m_list['median'] / m_copy['median']:.2f} x the copy")
    del d_list, d_copy

    m_select = event_ms(torch, lambda: mapper.select_windows(k_sel), warmup=0)
    line(f"selection: {mapper.n_ids:,} windows x {ns:,} reads, top_queries({k_sel})", m_select)
    placed = {}

    def place():
        placed["out"] = mapper.place_hits(ids, args.bound, args.cigar_cap)
    m_place = event_ms(torch, place)
    line(f"placement: {ns * k_sel:,} hits in blocks of 1,000 reads", m_place)
    strand_t, begin_t, end_t, keep_t, n_ops_t, cigar_t = placed["out"]
    span = torch.full((ns, k_sel, 4), -1, dtype=torch.int32, device=a.device)      # spans of the right shape: begin 0 .. n inside the window
    span[:, :, 0], span[:, :, 1] = 100, 100 + n

    def placements():
        B.check(L.bgsa_hip_reference_placements_dev(mapper.ref_len, W, S, ids.data_ptr(), ns, k_sel, span.data_ptr(), n_ops_t.data_ptr(),
                                                    cigar_t.data_ptr(), args.cigar_cap, strand_t.data_ptr(), begin_t.data_ptr(),
                                                    end_t.data_ptr(), keep_t.data_ptr(), stream), "reference_placements_dev")
    line("placements kernel alone, all reads in one call", event_ms(torch, placements))
    a.check_faults()

    # the same job through the parent's API: windows cut on the host, forward strand only
    t0 = time.perf_counter()
    starts = B.window_plan(args.ref_len, W, S)[1]
    windows = ref[starts[:, None] + np.arange(W)[None, :]]
    wall_cut = time.perf_counter() - t0
    old = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True)
    t0 = time.perf_counter()
    old.set_queries(windows)
    torch.cuda.synchronize()
    wall_upload = time.perf_counter() - t0
    old.set_subjects(reads)
    old_hits = {}

    def old_select():
        old_hits["out"] = old.top_queries(k_sel)
    m_old_select = event_ms(torch, old_select, warmup=0)

    def old_place():
        pq, ps = old.query_hits_as_pairs(old_hits["out"][1])
        old.place_pairs_banded(pq, ps, args.bound, cigar_cap=args.cigar_cap)
    m_old_place = event_ms(torch, old_place)
    old.check_faults()
    lines += ["", f"the same reads through host-cut windows, FORWARD strand only ({windows.shape[0]:,} windows, {windows.nbytes / 1e6:.1f} MB cut from "
                  f"{args.ref_len / 1e6:.1f} MB): host cut {wall_cut * 1e3:.1f} ms, set_queries (row buffer, upload, map) {wall_upload * 1e3:.1f} ms, wall"]
    line(f"selection: {windows.shape[0]:,} windows x {ns:,} reads, top_queries({k_sel})", m_old_select,
         f"both strands cost {m_select['median'] / m_old_select['median']:.2f} x")
    line(f"placement: {ns * k_sel:,} hits, place_pairs_banded in one call", m_old_place, f"blocks + coordinates cost {m_place['median'] / m_old_place['median']:.2f} x")
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

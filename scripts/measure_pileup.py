#!/usr/bin/env python3
"""What the pileup of a call's records costs on the device, beside three yardsticks measured on the same box in the same run
(profiles/pileup.txt).

    python scripts/measure_pileup.py [--out profiles/pileup.txt] [--ref-len 10000000] [--reads 100000] [--window 400]
                                     [--stride 239] [--read-len 150] [--bound 12] [--sample 256]

One process.  The job of scripts/measure_bam.py: 100,000 reads of 150 bp on a 10 Mbp reference, mapped once by the seeded pipeline
with k_best = 2, QUAL uniform over '!'..'~'.  The bucket's device tensors are kept, so every call starts from the same hits.
Before any time is printed a call of --sample (at least 256) reads goes through map_reads_sam(pileup=...) and is compared with the
host model's reading of that call's own SAM lines (tests/pileup_reference.py): the same rows, the same five counters, the same
sites; the flattened indices the yardstick uses are checked against the same model there.  Then

  events      by device events: the counts kernel inside the record stage's calls, and the two site passes inside Pileup.sites()
  yardsticks  torch's index_add_ of int32 ones over the same flattened indices (computed once on the host, not timed), for the
              counts kernel; a device-to-device copy_ of the count matrix's bytes, for the site passes, which read it once each
  wall clock  the BAM record stage (stored blocks) without and with pileup=, the two calls alternating, median and min .. max of 5
No time is a threshold: the figures are recorded, not claimed in advance.  The Python model is no tuned host baseline and is not
timed.
"""
from __future__ import annotations

import argparse
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from measure_bam import alternate, alternate_events, summary  # noqa: E402
from measure_reference_map import REPS, box_tag, make_job  # noqa: E402
from measure_sam import RNAME, Recorder  # noqa: E402

STEPS = (("counts", "pileup_kernel: the runs walked, one integer atomic per counted base (two on the reverse strand)"),
         ("sites_count", "sites_count_kernel: the site test per position, the workgroups' counts"),
         ("sites_emit", "sites_emit_kernel: the test again, ranks by ballot, the sites written in order"))
CLASS = np.full(256, 4, np.int64)
CLASS[list(b"ACGT")] = range(4)


def indices_of_sam(lines, min_base_quality: int, exclude_flags: int) -> np.ndarray:
    """The flattened indices position * 8 + column of every addition the model makes for these SAM lines, record after record
    (numpy per run instead of Python per base; checked against the model on the sample)."""
    out = []
    for line in lines:
        f = line.rstrip(b"\n").split(b"\t")
        flag = int(f[1])
        if flag & 4 or flag & exclude_flags:
            continue
        seq, qual = np.frombuffer(f[9], np.uint8), None if f[10] == b"*" else np.frombuffer(f[10], np.uint8).astype(np.int64) - 33
        begin = p = int(f[3]) - 1
        runs = [(int(n), op) for n, op in re.findall(r"(\d+)([=XDI])", f[5].decode())]
        end, j, reverse = begin + sum(n for n, op in runs if op != "I"), 0, bool(flag & 16)
        for n, op in runs:
            if op == "I":
                if begin < p < end:
                    out.append(np.array([(p - 1) * 8 + 6]))
                j += n
                continue
            at = np.arange(p, p + n, dtype=np.int64)
            if op == "D":
                cols = np.full(n, 5, np.int64)
            else:
                cols = CLASS[seq[j: j + n]]
                if qual is not None:
                    keep = qual[j: j + n] >= min_base_quality
                    at, cols = at[keep], cols[keep]
                j += n
            out.append(at * 8 + cols)
            if reverse:
                out.append(at * 8 + 7)
            p += n
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def lines_of(sam) -> list:
    text = sam.text.tobytes()
    return [text[sam.offsets[i]: sam.offsets[i + 1]] for i in range(sam.flag.size)]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "pileup.txt"))
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

    import bgsa_amd as B
    import pileup_reference as PR
    from bgsa_amd import reference as ref_module
    assert torch.cuda.is_available(), "no GPU visible: nothing here can be measured without one"
    ref, reads, _, _ = make_job(args)
    W, stride, n, ns, P = args.window, args.stride, args.read_len, args.reads, args.block_payload
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    mapper = B.ReferenceMapper(ref, W, stride)
    a, L = mapper.aligner, B.lib()
    lens = np.full(ns, n, dtype=np.int32)
    pileup = mapper.pileup()
    sites_at = dict(min_cover=2, min_alt=2, min_percent=20)      # the job's depth is 1.5: thresholds at which it has sites

    # ---- the pileup agrees with the model before any time is taken ---------------------------------------------------------------------
    few = max(args.sample, 256)
    call = dict(k_best=2, max_distance=args.bound, seed_len=args.seed_len, cigar_cap=args.cigar_cap)
    sample = mapper.map_reads_sam(reads[:few], None, quals[:few], RNAME, pileup=pileup, **call)
    sample_lines = lines_of(sample)
    want, want_stats = PR.pileup_of_sam(sample_lines, args.ref_len, pileup.min_mapq, pileup.min_base_quality, pileup.exclude_flags)
    got = pileup.counts_host()
    assert np.array_equal(got, want) and list(pileup.stats().values()) == want_stats, "the pileup of the sample is not the model's"
    flat = indices_of_sam(sample_lines, pileup.min_base_quality, pileup.exclude_flags)
    assert np.array_equal(np.bincount(flat, minlength=want.size), want.reshape(-1)), "the yardstick's indices are not the model's additions"
    codes = mapper.d_reference.cpu().numpy()
    found, model_sites = pileup.sites(**sites_at), PR.sites_of_fast(want, codes, **sites_at)
    assert all(np.array_equal(getattr(found, key), model_sites[key]) for key in model_sites), "the sites of the sample are not the model's"
    sample_stats, sample_sites = dict(pileup.stats()), int(found.pos.size)
    del got, want

    rname, flat_names, name_offsets, qual_rows = B.check_bam_call("measure_pileup", lens, None, quals, RNAME, P)
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def stage(fmt="bam", **form):
        sink = ref_module.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_pileup", sink, reads, lens, qual_rows, flat_names, name_offsets, rname, fmt=fmt, block_payload=P, **form)

    # ---- device events around the three kernels, taken inside the calls that launch them -------------------------------------------------
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
    L.bgsa_hip_pileup_dev = timed("counts", L.bgsa_hip_pileup_dev)
    L.bgsa_hip_pileup_sites_count_dev = timed("sites_count", L.bgsa_hip_pileup_sites_count_dev)
    L.bgsa_hip_pileup_sites_emit_dev = timed("sites_emit", L.bgsa_hip_pileup_sites_emit_dev)

    def piled():
        pileup.reset()
        return stage(pileup=pileup)
    calls = {"without pileup=": lambda: stage(), "with pileup=": piled}
    first = {name: fn() for name, fn in calls.items()}
    stats = dict(pileup.stats())
    assert first["with pileup="].blocks.tobytes() == first["without pileup="].blocks.tobytes(), "pileup= changed the blocks"
    flat = indices_of_sam(lines_of(stage(fmt="sam")), pileup.min_base_quality, pileup.exclude_flags)      # the same records as SAM lines
    full = pileup.counts.reshape(-1)
    assert np.array_equal(np.bincount(flat, minlength=full.numel()).astype(np.int32), full.cpu().numpy()), "the full job's counts are not the indices' histogram"
    additions = int(flat.size)
    torch.cuda.synchronize()
    for events in pending.values():
        events.clear()                                        # the warm-up calls are not counted
    wall, results = alternate(calls)
    job_sites = None
    for _ in range(REPS):
        job_sites = pileup.sites(**sites_at)
    torch.cuda.synchronize()
    events = {name: summary([e0.elapsed_time(e1) for e0, e1 in pairs]) for name, pairs in pending.items()}
    n_events = {name: len(pairs) for name, pairs in pending.items()}
    for name in calls:
        assert results[name].blocks.tobytes() == first[name].blocks.tobytes(), f"{name}: a repeated call gives other bytes"
    assert dict(pileup.stats()) == stats, "a repeated call gives other counters"

    # ---- the yardsticks: the same box, the same run -----------------------------------------------------------------------------------------
    d_flat = torch.from_numpy(flat).to(a.device)
    ones = torch.ones(additions, dtype=torch.int32, device=a.device)
    target, copy_to = torch.zeros_like(full), torch.empty_like(pileup.counts)

    def by_index_add():
        target.zero_()
        target.index_add_(0, d_flat, ones)
    yard = alternate_events(torch, {"zero": lambda: target.zero_(), "zero + index_add_": by_index_add, "copy_": lambda: copy_to.copy_(pileup.counts)})
    assert torch.equal(target, full), "index_add_ over the model's indices is not the kernel's matrix"
    a.check_faults()

    counts_ms = events["counts"]["median"]
    add_ms = yard["zero + index_add_"]["median"] - yard["zero"]["median"]
    lines = ["The pileup of a call's records on the device, beside three yardsticks (scripts/measure_pileup.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap {cap}, "
             f"QUAL uniform over 94 values, min_base_quality {pileup.min_base_quality}, exclude_flags {pileup.exclude_flags:#x}; count matrix "
             f"{pileup.counts.numel() * 4:,} bytes; box {box_tag()}; one run on one box",
             f"{few} reads through map_reads_sam(pileup=): rows, counters ({', '.join(f'{k} {v:,}' for k, v in sample_stats.items())}) and "
             f"{sample_sites} sites equal the host model's reading of the call's SAM lines; the full job's matrix is the histogram of the "
             f"model's indices, and the blocks with pileup= are the blocks without",
             "counters of the full job: " + ", ".join(f"{key} {value:,}" for key, value in stats.items()),
             f"additions of the full job (bases counted + their reverse-strand column + D and I runs): {additions:,}; "
             f"sites at {sites_at}: {job_sites.pos.size:,}",
             "device events inside the calls, median (min .. max):"]
    for name, what in STEPS:
        m = events[name]
        lines.append(f"  {what:<104s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  of {n_events[name]}")
    lines.append(f"  counts kernel: {stats['bases_counted'] / counts_ms / 1e6:.2f} G bases counted per second, {additions / counts_ms / 1e6:.2f} G atomic additions per second")
    lines.append(f"yardsticks by device events, alternating, median (min .. max) of {REPS}:")
    for name, m in yard.items():
        lines.append(f"  {name:<24s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})")
    lines.append(f"  index_add_ alone (the difference of the medians): {add_ms:.3f} ms, {additions / add_ms / 1e6:.2f} G additions per second; "
                 f"counts kernel / index_add_: {counts_ms / add_ms:.2f}")
    both = events["sites_count"]["median"] + events["sites_emit"]["median"]
    lines.append(f"  the two site passes together {both:.3f} ms, {both / yard['copy_']['median']:.2f} x the copy_ of the matrix "
                 f"({2 * pileup.counts.numel() * 4 / both / 1e6:.0f} GB/s read over both)")
    lines.append(f"wall clock of the BAM record stage, the two calls alternating, median (min .. max) of {REPS}, one process:")
    for name in calls:
        m = wall[name]
        lines.append(f"  {name:<20s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append(f"  with / without: {wall['with pileup=']['median'] / wall['without pileup=']['median']:.3f} (the second call also zeroes the matrix)")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

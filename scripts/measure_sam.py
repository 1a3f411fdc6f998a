#!/usr/bin/env python3
"""What the SAM stage costs, beside the path that exists without it, on the same hits, on the same box in the same run
(profiles/sam_records.txt).

    python scripts/measure_sam.py [--out profiles/sam_records.txt] [--ref-len 10000000] [--reads 100000] [--pairs 100000]
                                  [--window 400] [--stride 239] [--read-len 150] [--bound 12] [--sample 256]

One process.  Single ends: the 100,000 reads of scripts/measure_seeded_map.py (150 bp, two substitutions, both strands) on its
10 Mbp reference, mapped once by the seeded pipeline with k_best = 2; the bucket's device tensors are kept, so both paths below
start from the same hits.  Pairs: the 100,000 pairs of scripts/measure_pair_map.py, its bounds and insert range.  Before any time
is printed a fixed sample of records is compared, byte for byte, with the host model (tests/sam_reference.py) fed with the public
entry point's result.  Wall clock, median of 5:

  SAM stage            the list MAPQ and the primaries gathered (bgsa_hip_sam_mapq_dev + torch), measure, scan, emit, the text and
                       the four columns copied to the host: ReferenceMapper.sam_single_records / sam_pair_records
  parent's path        the lists, n_ops and the runs copied to the host, decode_cigars, and the host model's formatting of every
                       record: what a SAM writer on top of ReferenceHits / PairedHits does without the feature
  of which decode      the copies and decode_cigars alone
(the parent's path: median of 3.)  The ratio parent's path / SAM stage is recorded, not claimed in advance.
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

from measure_pair_map import make_pairs  # noqa: E402
from measure_reference_map import REPS, box_tag, event_ms, make_job  # noqa: E402

RNAME = b"ref10M"


class Recorder:
    """A sink that keeps every bucket's device tensors, to be replayed into a PrimarySink any number of times."""

    def __init__(self):
        self.buckets = []

    def add(self, idx, arrays, n_ops, cigar) -> None:
        self.buckets.append((idx, arrays, n_ops, cigar))


def wall(fn, reps: int = REPS):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        result = fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return dict(median=statistics.median(out), min=min(out), max=max(out)), result


def lines_at(records, sample):
    text = records.text.tobytes()
    return [text[records.offsets[i]: records.offsets[i + 1]] for i in sample]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "sam_records.txt"))
    ap.add_argument("--ref-len", type=int, default=10_000_000)
    ap.add_argument("--reads", type=int, default=100_000)
    ap.add_argument("--pairs", type=int, default=100_000)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--stride", type=int, default=239)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--bound", type=int, default=12)
    ap.add_argument("--seed-len", type=int, default=11)
    ap.add_argument("--pair-bound", type=int, default=6)
    ap.add_argument("--rescue", type=int, default=12)
    ap.add_argument("--insert-min", type=int, default=200)
    ap.add_argument("--insert-max", type=int, default=600)
    ap.add_argument("--cigar-cap", type=int, default=32)
    ap.add_argument("--block-rows", type=int, default=1000)
    ap.add_argument("--sample", type=int, default=256, help="records compared with the host model")
    ap.add_argument("--seed", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bgsa_amd as B
    import sam_reference as S
    from bgsa_amd import reference as R
    ref, reads, _, _ = make_job(args)
    reference = ref.tobytes()
    W, stride, n, ns = args.window, args.stride, args.read_len, args.reads
    mapper = B.ReferenceMapper(ref, W, stride)
    a = mapper.aligner
    rng = np.random.default_rng(args.seed + 7)
    quals = rng.integers(33, 127, size=(max(ns, args.pairs), n), dtype=np.uint8)
    lines = ["SAM records formatted on the device, beside decode_cigars + host formatting of the same hits (scripts/measure_sam.py)", ""]

    def row(name, m, note=""):
        lines.append(f"  {name:<66s} {m['median']:10.1f} ms  ({m['min']:.1f} .. {m['max']:.1f})  {note}")

    # ---- single ends ----------------------------------------------------------------------------------------------------------
    kw = dict(k_best=2, max_distance=args.bound, seed_len=args.seed_len, cigar_cap=args.cigar_cap, block_rows=args.block_rows)
    hits = mapper.map_reads_seeded(reads, **kw)
    lens = np.full(ns, n, dtype=np.int32)
    rname, flat, name_offsets, qual_rows = B.check_sam_call("measure_sam", lens, None, quals[:ns], RNAME)
    names = S.default_names(ns)
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def sam_single():
        sink = R.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_sam", sink, reads, lens, qual_rows, flat, name_offsets, rname)

    def decode_single():
        cigars = [[None] * hits.keep.shape[1] for _ in range(ns)]
        for idx, arrays, n_ops, cigar in recorder.buckets:
            host = [x.cpu().numpy() for x in arrays]
            R.decode_cigars("measure_sam", host[4], n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32), cap, idx, cigars)
        return cigars

    def parent_single():
        decode_single()
        return S.single_records(hits, reads, names, quals[:ns], reference, RNAME, args.bound)
    records = sam_single()
    sample = np.arange(0, ns, max(1, ns // args.sample))[: args.sample]
    picked = B.ReferenceHits(*(x[sample] for x in hits[:5]), [hits.cigars[c] for c in sample], hits.windows[sample])
    want = S.single_records(picked, reads[sample], [names[c] for c in sample], quals[sample], reference, RNAME, args.bound)[0]
    assert lines_at(records, sample) == want, "the sample differs from the host model"
    m_sam, records = wall(sam_single)
    m_parent, host_lines = wall(parent_single, 3)
    m_decode, _ = wall(decode_single)
    assert records.text.tobytes() == b"".join(host_lines[0]), "the two paths do not give the same file"
    sink = R.PrimarySink(mapper, ns, cap, args.bound)
    m_mapq = event_ms(torch, lambda: [sink.add(*bucket) for bucket in recorder.buckets])
    mapped = int((records.flag != 4).sum())
    lines += [f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2 (k_sel = "
              f"{mapper.k_selected(2)}), cigar_cap {cap}, QUAL given; box {box_tag()}",
              f"{len(sample)} records agree with the host model byte for byte, and the whole text equals the host path's: {mapped:,} mapped, "
              f"{records.text.size:,} bytes ({records.text.size / ns:.0f} per record)",
              f"wall clock, median (min .. max) of {REPS} runs, one process:"]
    row("SAM stage: mapq + gather, measure, scan, emit, copy of the text", m_sam, f"{records.text.size / m_sam['median'] / 1e6:.2f} GB/s of text")
    row("  of which mapq + gather of the primaries (HIP events)", m_mapq)
    row("parent's path: copies, decode_cigars, host formatting", m_parent, f"parent's path / SAM stage: {m_parent['median'] / m_sam['median']:.1f}")
    row("  of which the copies and decode_cigars", m_decode)

    # ---- pairs ----------------------------------------------------------------------------------------------------------------
    args.reads = 1
    reads1, reads2, _, _, _ = make_pairs(ref, args)
    ends_reads, np_ = (reads1, reads2), args.pairs
    pkw = dict(k_best=1, max_distance=args.pair_bound, cigar_cap=args.cigar_cap, block_rows=args.block_rows)
    paired = mapper.map_pairs(reads1, reads2, args.insert_min, args.insert_max, rescue_distance=args.rescue, **pkw)
    call = R.check_pair_call(True, reads1.shape, reads2.shape, args.insert_min, args.insert_max, 1, args.pair_bound, args.rescue, True, None, None,
                             args.cigar_cap, W, stride, mapper.ref_len, mapper.n_ids)
    single = [mapper.map_reads_seeded(rows, **pkw) for rows in ends_reads]
    ends = [mapper._rescue_checked(e, ends_reads, single, call, args.insert_max, args.block_rows) for e in range(2)]
    chosen = mapper.pair_select(ends[0][0][:5], ends[1][0][:5], args.insert_min, args.insert_max, args.block_rows)
    pair_quals = (quals[:np_], quals[:np_][:, ::-1].copy())
    checked = [B.check_sam_call("measure_sam", np.full(np_, n), None, q, RNAME) for q in pair_quals]
    pair_names = S.default_names(np_)

    def sam_pairs():
        return mapper.sam_pair_records("measure_sam", ends_reads, ends, chosen, call, checked)

    def decode_pairs():
        for e, (final, n_ops, cigar, _) in enumerate(ends):
            cigars = [[None] * final[0].shape[1] for _ in range(np_)]
            host = [x.cpu().numpy() for x in final]
            R.decode_cigars("measure_sam", host[4], n_ops.cpu().numpy(), cigar.cpu().numpy().view(np.uint32), call["caps"][e], np.arange(np_), cigars)

    def parent_pairs():
        decode_pairs()
        return S.pair_records(paired, reads1, reads2, pair_names, *pair_quals, reference, RNAME, call["bounds"])
    records = sam_pairs()
    sample = np.arange(0, np_, max(1, np_ // args.sample))[: args.sample]

    def take(h):
        return B.ReferenceHits(*(x[sample] for x in h[:5]), [h.cigars[c] for c in sample], h.windows[sample])
    sub = B.PairedHits(take(paired.end1), take(paired.end2), *(x[sample] for x in paired[2:]))
    want = S.pair_records(sub, reads1[sample], reads2[sample], [pair_names[c] for c in sample], pair_quals[0][sample], pair_quals[1][sample],
                          reference, RNAME, call["bounds"])[0]
    assert lines_at(records, np.stack((2 * sample, 2 * sample + 1), axis=1).reshape(-1)) == want, "the sample of pairs differs from the host model"
    m_sam, records = wall(sam_pairs)
    m_parent, host_lines = wall(parent_pairs, 3)
    m_decode, _ = wall(decode_pairs)
    assert records.text.tobytes() == b"".join(host_lines[0]), "the two paths do not give the same file for the pairs"
    a.check_faults()
    lines += ["", f"{np_:,} pairs of 2 x {n} bp, insert {args.insert_min}..{args.insert_max}, max_distance {args.pair_bound}, rescue_distance "
              f"{args.rescue}, k_pair = {call['k_pair']}: {2 * np_:,} records, {int((records.flag & 2 != 0).sum()) // 2:,} proper pairs, "
              f"{records.text.size:,} bytes",
              f"{len(sample)} pairs agree with the host model byte for byte, and the whole text equals the host path's"]
    row("SAM stage: pair mapq + gather, measure, scan, emit, copy of the text", m_sam, f"{records.text.size / m_sam['median'] / 1e6:.2f} GB/s of text")
    row("parent's path: copies, decode_cigars, host formatting", m_parent, f"parent's path / SAM stage: {m_parent['median'] / m_sam['median']:.1f}")
    row("  of which the copies and decode_cigars", m_decode)
    text = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())

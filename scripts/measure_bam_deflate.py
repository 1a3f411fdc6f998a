#!/usr/bin/env python3
"""What deflating the BGZF blocks on the device costs or saves beside the stored blocks of the same records, on the same box in
the same run (profiles/bam_deflate.txt).

    python scripts/measure_bam_deflate.py [--out profiles/bam_deflate.txt] [--ref-len 10000000] [--reads 100000] [--window 400]
                                          [--stride 239] [--read-len 150] [--bound 12] [--sample 256] [--block-payload 65280]

One process.  The job of scripts/measure_bam.py: 100,000 reads of 150 bp on a 10 Mbp reference, mapped once by the seeded pipeline
with k_best = 2, QUAL uniform over '!'..'~'; the bucket's device tensors are kept, so both calls start from the same hits.  Before any
time is printed the compressed blocks are inflated by zlib, must equal the stored call's payload, and a fixed sample of records is
decoded by the host model (tests/bam_reference.py) and compared with the lines of the SAM text, byte for byte.  Then

  sizes       the payload, the stored blocks, the compressed blocks and the share of blocks that came out stored; zlib level 1 and
              level 6 on the same payload cut into the same blocks, on the host, with their time
  wall clock  the BAM stage with compress=False and with compress=True, alternating, median and min .. max of 5
  events      by device events, alternating: bgsa_hip_bgzf_deflate_dev alone with its payload bytes per second, bgsa_hip_bgzf_pack_dev,
              bgsa_hip_bgzf_frame_dev and a device-to-device copy of the payload
No time is a threshold: the figures are recorded, not claimed in advance.
"""
from __future__ import annotations

import argparse
import sys
import time
import zlib
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))
sys.path.insert(0, str(ROOT / "tests"))

from measure_bam import alternate, alternate_events  # noqa: E402
from measure_reference_map import REPS, box_tag, make_job  # noqa: E402
from measure_sam import RNAME, Recorder  # noqa: E402


def block_list(blocks: bytes) -> list:
    out, at = [], 0
    while at < len(blocks):
        size = int.from_bytes(blocks[at + 16: at + 18], "little") + 1
        out.append(blocks[at: at + size])
        at += size
    return out


def zlib_blocks(payload: bytes, P: int, level: int) -> tuple:
    """(bytes, seconds) of the payload cut into blocks of P, each a raw deflate stream of its own at `level`, framed as BGZF."""
    t0, total = time.perf_counter(), 0
    for at in range(0, len(payload), P):
        z = zlib.compressobj(level, zlib.DEFLATED, -15)
        total += len(z.compress(payload[at: at + P])) + len(z.flush()) + 26
    return total, time.perf_counter() - t0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "bam_deflate.txt"))
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
    a, L = mapper.aligner, B.lib()
    quals = np.random.default_rng(args.seed + 7).integers(33, 127, size=(ns, n), dtype=np.uint8)
    lens = np.full(ns, n, dtype=np.int32)
    rname, flat, name_offsets, qual_rows = B.check_bam_call("measure_bam_deflate", lens, None, quals, RNAME, P, True)
    recorder = mapper._map_to(lambda *_: Recorder(), reads, lens, False, 2, args.bound, True, args.seed_len, None, args.block_rows, args.cigar_cap)
    cap = recorder.buckets[0][3].shape[2]

    def stage(**form):
        sink = R.PrimarySink(mapper, ns, cap, args.bound)
        for bucket in recorder.buckets:
            sink.add(*bucket)
        return mapper.sam_single_records("measure_bam_deflate", sink, reads, lens, qual_rows, flat, name_offsets, rname, **form)

    # ---- the records agree before any time is taken ---------------------------------------------------------------------------
    sam, stored, packed = stage(), stage(fmt="bam", block_payload=P), stage(fmt="bam", block_payload=P, compress=True)
    payload = b"".join(M.walk_blocks(stored.blocks.tobytes()))
    assert payload and b"".join(M.walk_blocks(packed.blocks.tobytes(), stored=False)) == payload, "the compressed blocks inflate to other bytes"
    sample = np.arange(0, ns, max(1, ns // max(args.sample, 256)))[: max(args.sample, 256)]
    text = sam.text.tobytes()
    for i in sample:
        line = M.decode(payload[packed.offsets[i]: packed.offsets[i + 1]], [RNAME])["line"]
        assert line == text[sam.offsets[i]: sam.offsets[i + 1]], f"record {i} decodes to another line than the SAM stage wrote"
    for name in ("offsets", "flag", "pos", "mapq", "nm"):
        assert np.array_equal(getattr(stored, name), getattr(packed, name)), name
    blocks = block_list(packed.blocks.tobytes())
    n_blocks = -(-len(payload) // P)
    n_stored = sum(1 for b in blocks if b[18] & 7 == 1)
    assert len(blocks) == n_blocks
    level1, level6 = zlib_blocks(payload, P, 1), zlib_blocks(payload, P, 6)

    # ---- the two stages, alternating ------------------------------------------------------------------------------------------------
    wall, results = alternate({"stored": lambda: stage(fmt="bam", block_payload=P), "deflate": lambda: stage(fmt="bam", block_payload=P, compress=True)})
    assert results["deflate"].blocks.tobytes() == packed.blocks.tobytes() and results["stored"].blocks.tobytes() == stored.blocks.tobytes(), \
        "a repeated call gives other bytes"

    # ---- the kernels alone ------------------------------------------------------------------------------------------------------------
    dev = a.device
    d_payload = torch.from_numpy(np.frombuffer(payload, np.uint8).copy()).to(dev)
    framed = int(L.bgsa_hip_bgzf_framed_bytes(len(payload), P))
    d_framed, d_copy = torch.empty(framed, dtype=torch.uint8, device=dev), torch.empty(len(payload), dtype=torch.uint8, device=dev)
    d_slots = torch.empty(n_blocks * (P + 31), dtype=torch.uint8, device=dev)
    d_lengths = torch.empty(n_blocks, dtype=torch.int64, device=dev)
    room = int(L.bgsa_hip_bgzf_deflate_workspace_bytes(len(payload), P))
    d_workspace = torch.empty(room // 4 + 1, dtype=torch.int32, device=dev)
    d_refused = torch.zeros(1, dtype=torch.int32, device=dev)

    def deflate():
        B.check(L.bgsa_hip_bgzf_deflate_dev(d_payload.data_ptr(), len(payload), P, d_slots.data_ptr(), n_blocks * (P + 31), d_lengths.data_ptr(),
                                            d_workspace.data_ptr(), room, a._stream()), "bgzf_deflate_dev")
    deflate()
    d_offsets = torch.zeros(n_blocks + 1, dtype=torch.int64, device=dev)
    d_offsets[1:] = torch.cumsum(d_lengths, 0)
    out_bytes = int(d_offsets[-1].item())
    d_out = torch.empty(out_bytes, dtype=torch.uint8, device=dev)

    def pack():
        B.check(L.bgsa_hip_bgzf_pack_dev(d_slots.data_ptr(), P, n_blocks, d_offsets.data_ptr(), d_out.data_ptr(), out_bytes, d_refused.data_ptr(),
                                         a._stream()), "bgzf_pack_dev")

    def frame():
        B.check(L.bgsa_hip_bgzf_frame_dev(d_payload.data_ptr(), len(payload), P, d_framed.data_ptr(), framed, a._stream()), "bgzf_frame_dev")
    events = alternate_events(torch, {"deflate": deflate, "pack": pack, "frame": frame, "copy": lambda: d_copy.copy_(d_payload)})
    assert d_out.cpu().numpy().tobytes() == packed.blocks.tobytes() and int(d_refused.item()) == 0, "the kernels alone give other blocks than the stage"
    a.check_faults()

    lines = ["BGZF blocks deflated on the device, beside the stored blocks of the same records (scripts/measure_bam_deflate.py)", "",
             f"reference {args.ref_len:,} bp, W = {W}, S = {stride}; {ns:,} reads of {n} bp, max_distance {args.bound}, k_best 2, cigar_cap {cap}, "
             f"QUAL uniform over 94 values, block_payload {P:,}; box {box_tag()}; one run on one box",
             f"the compressed blocks inflate (zlib) to the stored call's payload; {len(sample)} records decoded on the host equal their SAM lines "
             f"byte for byte; the offsets and the four columns are equal",
             f"bytes: payload {len(payload):,} in {n_blocks:,} blocks; stored blocks {len(stored.blocks):,}; compressed blocks {len(packed.blocks):,} "
             f"({len(packed.blocks) / len(stored.blocks):.3f} of the stored); {n_stored:,} of {n_blocks:,} blocks came out stored",
             f"zlib on the host, the same payload cut into the same blocks: level 1 {level1[0]:,} bytes in {level1[1] * 1e3:.0f} ms "
             f"({level1[0] / len(stored.blocks):.3f}); level 6 {level6[0]:,} bytes in {level6[1] * 1e3:.0f} ms ({level6[0] / len(stored.blocks):.3f})",
             f"wall clock of the BAM stage, the calls alternating, median (min .. max) of {REPS}, one process:"]
    for name, what in (("stored", "compress=False: mapq + gather, measure, scan, emit, frame, copy of the blocks"),
                       ("deflate", "compress=True:  mapq + gather, measure, scan, emit, deflate, scan, pack, copy of the blocks")):
        m = wall[name]
        lines.append(f"  {what:<92s} {m['median']:9.2f} ms  ({m['min']:.2f} .. {m['max']:.2f})")
    lines.append(f"  compress=True / compress=False: {wall['deflate']['median'] / wall['stored']['median']:.2f}")
    lines.append(f"device events, alternating, median (min .. max) of {REPS}, on the {len(payload):,} payload bytes:")
    for name, what in (("deflate", "bgzf_deflate_kernel: match, parse, codes, bitstream, CRC-32, one workgroup per block"),
                       ("pack", "bgzf_pack_kernel: the blocks from their slots to their offsets"),
                       ("frame", "bgzf_frame_kernel: copy + CRC-32 + 31 bytes of framing per block"),
                       ("copy", "device-to-device copy of the payload")):
        m = events[name]
        lines.append(f"  {what:<92s} {m['median']:9.3f} ms  ({m['min']:.3f} .. {m['max']:.3f})  {len(payload) / m['median'] / 1e6:8.2f} GB/s of payload")
    out = "\n".join(lines) + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(out)
    print(out)
    return 0


if __name__ == "__main__":
    sys.exit(main())

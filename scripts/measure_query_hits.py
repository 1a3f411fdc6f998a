#!/usr/bin/env python3
"""What the hit lists per subject cost beside the row selection and the scoring of the same tile (profiles/query_hits.txt).

    python scripts/measure_query_hits.py [--out profiles/query_hits.txt] [--subjects 1000000] [--queries 10000]

Two GPU steps, each a child process of its own under `timeout` (a step that hangs or faults ends there and the next one
is not started):

  block   one 1,000 x 1M x 150 bp Myers block (a 2 GB int16 tile), HIP events around each piece, in one process:
          the scoring kernel; top_hits(10), the row selection of the same tile — the yardstick; top_queries for K = 1, 10, 64
          on the scores of random reads; the threshold lists at a cutoff that keeps about 0.1 % of the pairs; and
          top_queries(10) on a tile of the same shape whose scores improve with the row index, so that every element enters
          its column's list (the worst case).  Every piece carries the shader clock eight probe waves saw while it ran, the
          card's power and a tag of the box.
  job     wall time of the whole 10k x 1M job through DeviceAligner.top_queries(10), beside DeviceAligner.score() alone over
          the same blocks into the same reused tile.

The yardstick: top_queries(10) on random scores should stay within three times top_hits(10) on the same tile in the same run.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import socket
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from measure_hits import BLOCK, QLEN, reads  # noqa: E402

K_LIST = (1, 10, 64)
CAP = 64


def box_tag() -> str:
    """Which box a line was measured on, without naming it: runs on one box carry one tag."""
    return hashlib.sha1(socket.gethostname().encode()).hexdigest()[:6]


def stream_event_ms(torch, fn, reps: int, warmup: int) -> dict:
    """HIP events around fn, waiting on the CALLER's stream only: a device-wide synchronize would also wait for the probe
    waves, which sleep on a stream of their own until they are stopped or their time bound passes."""
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    stream.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "reps": reps}


def measured(torch, L, stream, fn, reps: int, warmup: int = 2) -> dict:
    """stream_event_ms of fn with the shader clock (probe waves), the card's power and the box it ran on."""
    import numpy as np

    from bench import PowerSampler
    probing = L.bgsa_hip_clock_probe_start(8, 20000, stream) == 0
    sampler = PowerSampler(0.02).start()
    try:
        out = stream_event_ms(torch, fn, reps, warmup)
    finally:
        power = sampler.stop() or {}
        if probing:      # stopped before anything synchronises the whole device
            mhz, xcc = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
            n, secs = ctypes.c_int(0), ctypes.c_double(0)
            probed = L.bgsa_hip_clock_probe_stop(mhz, xcc, 16, ctypes.byref(n), ctypes.byref(secs)) == 0 and n.value
    out["watts_mean"] = power.get("watts_mean")
    if probing and probed:
        out["mhz"] = round(float(np.mean([mhz[i] for i in range(n.value)])), 1)
    out["box"] = box_tag()
    return out


def step_block(args) -> dict:
    import torch

    import bgsa_amd as B
    L = B.lib()
    q, s = reads(BLOCK, args.subjects)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    tile = torch.empty((BLOCK, a.ns), dtype=torch.int16, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    row_work = torch.empty(int(L.bgsa_hip_hits_workspace_bytes(BLOCK, a.ns, 2, 64)), dtype=torch.uint8, device="cuda:0")
    work = torch.empty(int(L.bgsa_hip_query_hits_workspace_bytes(BLOCK, a.ns, 2, 64)), dtype=torch.uint8, device="cuda:0")
    a.score(0, BLOCK, out=tile)
    a.check_faults()
    sample = tile[:8, : a.ns_real].reshape(-1).to(torch.int32)
    cutoff = int(torch.sort(sample).values[int(sample.numel() * 0.999)].item())

    row_scores = torch.empty((BLOCK, 10), dtype=torch.int32, device="cuda:0")
    row_subjects = torch.empty((BLOCK, 10), dtype=torch.int64, device="cuda:0")

    def top_hits_10():
        B.check(L.bgsa_hip_top_hits_dev(tile.data_ptr(), 2, BLOCK, a.ns, a.ns_real, 0, 10, 0, 0, row_scores.data_ptr(), row_subjects.data_ptr(),
                                        row_work.data_ptr(), row_work.numel(), stream), "top_hits_dev")

    def top_queries(k):
        sc = torch.empty((a.ns_real, k), dtype=torch.int32, device="cuda:0")
        hq = torch.empty((a.ns_real, k), dtype=torch.int32, device="cuda:0")

        def run():
            B.check(L.bgsa_hip_top_queries_dev(tile.data_ptr(), 2, BLOCK, a.ns, a.ns_real, 0, k, 0, 0, sc.data_ptr(), hq.data_ptr(),
                                               work.data_ptr(), work.numel(), stream), "top_queries_dev")
        return run

    cnt = torch.empty((a.ns_real,), dtype=torch.int32, device="cuda:0")
    tsc = torch.empty((a.ns_real, CAP), dtype=torch.int32, device="cuda:0")
    thq = torch.empty((a.ns_real, CAP), dtype=torch.int32, device="cuda:0")

    def threshold():
        B.check(L.bgsa_hip_threshold_queries_dev(tile.data_ptr(), 2, BLOCK, a.ns, a.ns_real, 0, cutoff, 0, 0, CAP, cnt.data_ptr(),
                                                 tsc.data_ptr(), thq.data_ptr(), work.data_ptr(), work.numel(), stream), "threshold_queries_dev")

    def m(fn, reps=args.reps, warmup=2):
        return measured(torch, L, stream, fn, reps, warmup)

    out = {"shape": f"{BLOCK} x {a.ns_real} x {QLEN} bp Myers global, tile {tile.numel() * 2 / 1e9:.3f} GB int16 (row stride {a.ns})",
           "score_kernel": m(lambda: a.score(0, BLOCK, out=tile)),
           "top_hits_k10": m(top_hits_10)}
    for k in K_LIST:
        out[f"top_queries_k{k}"] = m(top_queries(k))
    out["threshold_queries"] = m(threshold)
    kept = int(cnt.to(torch.int64).sum().item())
    out.update(threshold_cutoff=cutoff, threshold_kept_fraction=round(kept / (BLOCK * a.ns_real), 6), threshold_cap=CAP,
               threshold_columns_over_cap=int((cnt > CAP).sum().item()), workspace_bytes=work.numel())
    # the worst case: scores that improve with the row index, the same in every column — every element enters its list
    ramp = (torch.arange(BLOCK, device="cuda:0", dtype=torch.int32) - BLOCK // 2).to(torch.int16)
    tile.copy_(ramp.unsqueeze(1).expand(BLOCK, a.ns))
    out["top_queries_k10_improving_rows"] = m(top_queries(10), min(args.reps, 3), 1)
    a.check_faults()
    return out


def step_job(args) -> dict:
    import torch

    import bgsa_amd as B
    q, s = reads(args.queries, args.subjects)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    tile = torch.empty((BLOCK, a.ns), dtype=torch.int16, device="cuda:0")

    def score_only():
        for lo in range(0, a.nq, BLOCK):
            a.score(lo, min(lo + BLOCK, a.nq), out=tile[: min(lo + BLOCK, a.nq) - lo])

    def wall(fn):
        fn()                          # warm-up: code objects, the tile, the workspace
        torch.cuda.synchronize()
        times = []
        for _ in range(args.job_reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        return {"median_s": round(statistics.median(times), 4), "min_s": round(min(times), 4), "reps": args.job_reps}

    into = a.top_queries(10, block_rows=BLOCK)       # the lists are allocated once, as a caller walking query sets would
    out = {"shape": f"{a.nq} x {a.ns_real} x {QLEN} bp Myers global in blocks of {BLOCK} queries", "box": box_tag(),
           "score_only": wall(score_only), "top_queries_10": wall(lambda: a.top_queries(10, block_rows=BLOCK))}
    a.check_faults()
    del into
    cells = a.nq * a.ns_real * QLEN * QLEN
    out["gcups_score_only"] = round(cells / out["score_only"]["median_s"] / 1e9)
    out["gcups_top_queries_10"] = round(cells / out["top_queries_10"]["median_s"] / 1e9)
    out["matrix_bytes_not_written"] = a.nq * a.ns * 2
    out["hit_list_bytes"] = a.ns_real * 10 * 8
    return out


def report(block: dict | None, job: dict | None, notes: list[str]) -> str:
    lines = ["hit lists per subject beside the row selection and the scoring of the same tile (scripts/measure_query_hits.py)", ""]
    if block:
        score = block["score_kernel"]["median_ms"]
        yard = block["top_hits_k10"]["median_ms"]
        lines += [f"block: {block['shape']}", "HIP events, median (min .. max) of %d runs; x = against top_hits(10) of the same tile:" % block["score_kernel"]["reps"]]
        names = [("score_kernel", "scoring kernel"), ("top_hits_k10", "top_hits(10): the K best subjects per query (rows), the yardstick")]
        names += [(f"top_queries_k{k}", f"top_queries({k}): the K best queries per subject (columns)") for k in K_LIST]
        names += [("threshold_queries", f"threshold_queries, cutoff {block['threshold_cutoff']} keeps {100 * block['threshold_kept_fraction']:.3f} % of the pairs"),
                  ("top_queries_k10_improving_rows", "worst case: top_queries(10), scores improve with the row")]
        for key, name in names:
            m = block[key]
            lines.append(f"  {name:<72s} {m['median_ms']:10.3f} ms  ({m['min_ms']:.3f} .. {m['max_ms']:.3f})  {m['median_ms'] / yard:8.2f} x  "
                         f"{m['median_ms'] / score:7.3f} x scoring   [{m.get('mhz', 'n/a')} MHz, {m.get('watts_mean', 'n/a')} W, box {m['box']}]")
        k10 = block["top_queries_k10"]["median_ms"]
        lines += [f"  threshold lists: cap {block['threshold_cap']} per subject, {block['threshold_columns_over_cap']} columns over it; "
                  f"workspace {block['workspace_bytes']} bytes",
                  "",
                  f"yardstick: top_queries(10) on random scores ({k10:.3f} ms) is {k10 / yard:.2f} x top_hits(10) of the same tile ({yard:.3f} ms): "
                  f"{'WITHIN' if k10 <= 3 * yard else 'BEYOND'} three times; worst case "
                  f"{block['top_queries_k10_improving_rows']['median_ms'] / yard:.1f} x; K = 10 is {100 * k10 / score:.2f} % of the scoring time", ""]
    if job:
        lines += [f"job: {job['shape']}   [box {job['box']}]",
                  f"  score() alone over the blocks         {job['score_only']['median_s']:8.4f} s wall (min {job['score_only']['min_s']:.4f}, {job['score_only']['reps']} runs)  = {job['gcups_score_only']:,} GCUPS",
                  f"  top_queries(10) over the same blocks  {job['top_queries_10']['median_s']:8.4f} s wall (min {job['top_queries_10']['min_s']:.4f})  = {job['gcups_top_queries_10']:,} GCUPS",
                  f"  result: {job['hit_list_bytes']:,} bytes of hit lists instead of {job['matrix_bytes_not_written']:,} bytes of scores", ""]
    lines += notes
    return "\n".join(lines).rstrip() + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "query_hits.txt"))
    ap.add_argument("--subjects", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--job-reps", type=int, default=3)
    ap.add_argument("--step", choices=["block", "job"], help="run one step in this process and print its JSON (used by the driver)")
    ap.add_argument("--step-timeout", type=int, default=400, help="seconds each GPU step may take")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step_block(args) if args.step == "block" else step_job(args)))
        return 0
    results, notes = {}, []
    for step in ("block", "job"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()), "--step", step,
               "--subjects", str(args.subjects), "--queries", str(args.queries), "--reps", str(args.reps), "--job-reps", str(args.job_reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        found = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not found:
            notes.append(f"step {step}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
            break
        results[step] = json.loads(found[-1][len("RESULT "):])
    text = report(results.get("block"), results.get("job"), notes)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 1 if notes else 0


if __name__ == "__main__":
    sys.exit(main())

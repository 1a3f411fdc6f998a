#!/usr/bin/env python3
"""What hit selection costs beside the scoring it follows and the copy it replaces (profiles/hits_select.txt).

    python scripts/measure_hits.py [--out profiles/hits_select.txt] [--subjects 1000000] [--queries 10000]

Two GPU steps, each a child process of its own under `timeout` (a step that hangs or faults ends there and the next one
is not started):

  block   one 1,000 x 1M x 150 bp Myers block, HIP events around each piece, in one process:
          the scoring kernel; top-K selection for K = 1, 10, 64; threshold selection at a cutoff that keeps about 0.1 %
          of the pairs; the copy of the same 2 GB tile to page-locked host memory; and top-K at K = 10 on an adversarial
          tile of the same shape whose scores rise with the column inside every segment, so that every element is
          inserted (the selection's worst case).  Eight probe waves (probe.hip) record the shader clock the step sustained.
  job     wall time of the whole 10k x 1M job through DeviceAligner.top_hits(10), beside DeviceAligner.score() alone over
          the same blocks into the same reused tile.

The criterion: selection at K = 10 must take less time than the device-to-host copy of the tile, in the same run.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

QLEN = 150
BLOCK = 1000


def reads(n_queries: int, n_subjects: int):
    import oracle
    return oracle.gen_reads(0xB65A0001, n_queries, QLEN), oracle.gen_reads(0xB65A1001, n_subjects, QLEN)


def event_ms(torch, fn, reps: int, warmup: int = 2):
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
    return {"median_ms": round(statistics.median(out), 4), "min_ms": round(min(out), 4), "max_ms": round(max(out), 4), "reps": reps}


def step_block(args) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    L = B.lib()
    q, s = reads(BLOCK, args.subjects)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    tile = torch.empty((BLOCK, a.ns), dtype=torch.int16, device="cuda:0")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    work = torch.empty(int(L.bgsa_hip_hits_workspace_bytes(BLOCK, a.ns, 2, 64)), dtype=torch.uint8, device="cuda:0")
    a.score(0, BLOCK, out=tile)
    a.check_faults()
    # a cutoff that keeps about 0.1 % of the pairs: the 99.9th percentile of a sample of rows
    sample = tile[:8, : a.ns_real].reshape(-1).to(torch.int32)
    cutoff = int(torch.sort(sample).values[int(sample.numel() * 0.999)].item())
    host = torch.empty((BLOCK, a.ns), dtype=torch.int16, pin_memory=True)

    def top(k):
        sc = torch.empty((BLOCK, k), dtype=torch.int32, device="cuda:0")
        sj = torch.empty((BLOCK, k), dtype=torch.int64, device="cuda:0")

        def run():
            B.check(L.bgsa_hip_top_hits_dev(tile.data_ptr(), 2, BLOCK, a.ns, a.ns_real, 0, k, 0, 0, sc.data_ptr(), sj.data_ptr(),
                                            work.data_ptr(), work.numel(), stream), "top_hits_dev")
        return run

    cap = max(64, int(a.ns_real * 0.004))
    cnt = torch.empty((BLOCK,), dtype=torch.int32, device="cuda:0")
    tsc = torch.empty((BLOCK, cap), dtype=torch.int32, device="cuda:0")
    tsj = torch.empty((BLOCK, cap), dtype=torch.int64, device="cuda:0")

    def threshold():
        B.check(L.bgsa_hip_threshold_hits_dev(tile.data_ptr(), 2, BLOCK, a.ns, a.ns_real, 0, cutoff, 0, 0, cap, cnt.data_ptr(),
                                              tsc.data_ptr(), tsj.data_ptr(), work.data_ptr(), work.numel(), stream), "threshold_hits_dev")

    probing = L.bgsa_hip_clock_probe_start(8, 120000, stream) == 0
    out = {"shape": f"{BLOCK} x {a.ns_real} x {QLEN} bp Myers global, tile {tile.numel() * 2 / 1e9:.3f} GB int16 (row stride {a.ns})",
           "score_kernel": event_ms(torch, lambda: a.score(0, BLOCK, out=tile), args.reps)}
    for k in (1, 10, 64):
        out[f"top_hits_k{k}"] = event_ms(torch, top(k), args.reps)
    out["threshold_hits"] = event_ms(torch, threshold, args.reps)
    out["copy_tile_to_pinned_host"] = event_ms(torch, lambda: host.copy_(tile, non_blocking=True), args.reps)
    # the worst case: scores that rise with the column (a sawtooth of period 32,768, longer than a segment of the row),
    # so inside a segment every element beats the wave's cutoff and is inserted
    ramp = (torch.arange(a.ns, device="cuda:0", dtype=torch.int32) % 32768 - 16384).to(torch.int16)
    tile.copy_(ramp.unsqueeze(0).expand(BLOCK, a.ns))
    out["top_hits_k10_rising_scores"] = event_ms(torch, top(10), min(args.reps, 3), warmup=1)
    torch.cuda.synchronize()
    if probing:
        mhz, xcc = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
        n, secs = ctypes.c_int(0), ctypes.c_double(0)
        if L.bgsa_hip_clock_probe_stop(mhz, xcc, 16, ctypes.byref(n), ctypes.byref(secs)) == 0 and n.value:
            out["sustained_mhz"] = round(float(np.mean([mhz[i] for i in range(n.value)])), 1)
    kept = int(cnt.to(torch.int64).sum().item())
    out["threshold_cutoff"] = cutoff
    out["threshold_kept_fraction"] = round(kept / (BLOCK * a.ns_real), 6)
    out["threshold_cap_per_query"] = cap
    out["threshold_rows_over_cap"] = int((cnt > cap).sum().item())
    out["workspace_bytes"] = work.numel()
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

    out = {"shape": f"{a.nq} x {a.ns_real} x {QLEN} bp Myers global in blocks of {BLOCK} queries",
           "score_only": wall(score_only), "top_hits_10": wall(lambda: a.top_hits(10, block_rows=BLOCK))}
    a.check_faults()
    cells = a.nq * a.ns_real * QLEN * QLEN
    out["gcups_score_only"] = round(cells / out["score_only"]["median_s"] / 1e9)
    out["gcups_top_hits_10"] = round(cells / out["top_hits_10"]["median_s"] / 1e9)
    out["matrix_bytes_not_written"] = a.nq * a.ns * 2
    out["hit_list_bytes"] = a.nq * 10 * 12
    return out


def report(block: dict | None, job: dict | None, notes: list[str]) -> str:
    lines = ["hit selection beside scoring and the copy it replaces (scripts/measure_hits.py)", ""]
    if block:
        score = block["score_kernel"]["median_ms"]
        copy = block["copy_tile_to_pinned_host"]["median_ms"]
        lines += [f"block: {block['shape']}",
                  f"sustained shader clock during the step: {block.get('sustained_mhz', 'not measured')} MHz",
                  "HIP events, median (min .. max) of %d runs:" % block["score_kernel"]["reps"]]
        names = [("score_kernel", "scoring kernel"), ("top_hits_k1", "top-K selection, K = 1"), ("top_hits_k10", "top-K selection, K = 10"),
                 ("top_hits_k64", "top-K selection, K = 64"),
                 ("threshold_hits", f"threshold selection, cutoff {block['threshold_cutoff']} keeps {100 * block['threshold_kept_fraction']:.3f} % of the pairs"),
                 ("copy_tile_to_pinned_host", "copy of the tile to page-locked host memory"),
                 ("top_hits_k10_rising_scores", "worst case: K = 10 on a tile whose scores rise with the column")]
        for key, name in names:
            m = block[key]
            lines.append(f"  {name:<72s} {m['median_ms']:10.3f} ms  ({m['min_ms']:.3f} .. {m['max_ms']:.3f})   {m['median_ms'] / score:7.3f} x scoring")
        k10 = block["top_hits_k10"]["median_ms"]
        verdict = "SMALLER than" if k10 < copy else "NOT smaller than"
        lines += [f"  threshold lists: cap {block['threshold_cap_per_query']} per query, {block['threshold_rows_over_cap']} rows over it; "
                  f"selection workspace {block['workspace_bytes']} bytes",
                  "",
                  f"criterion: selection at K = 10 ({k10:.3f} ms) is {verdict} the device-to-host copy of the tile ({copy:.3f} ms): "
                  f"{copy / k10:.1f} x; it is {100 * k10 / score:.2f} % of the scoring time", ""]
    if job:
        lines += [f"job: {job['shape']}",
                  f"  score() alone over the blocks      {job['score_only']['median_s']:8.4f} s wall (min {job['score_only']['min_s']:.4f}, {job['score_only']['reps']} runs)  = {job['gcups_score_only']:,} GCUPS",
                  f"  top_hits(10) over the same blocks  {job['top_hits_10']['median_s']:8.4f} s wall (min {job['top_hits_10']['min_s']:.4f})  = {job['gcups_top_hits_10']:,} GCUPS",
                  f"  result: {job['hit_list_bytes']:,} bytes of hit lists instead of {job['matrix_bytes_not_written']:,} bytes of scores", ""]
    lines += notes
    return "\n".join(lines).rstrip() + "\n"


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hits_select.txt"))
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

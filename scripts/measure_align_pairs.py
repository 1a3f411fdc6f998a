#!/usr/bin/env python3
"""What the edit scripts of the hit pairs cost beside the scoring and the selection they follow (profiles/align_pairs.txt).

    python scripts/measure_align_pairs.py [--out profiles/align_pairs.txt]

Two GPU steps, each a child process of its own under `timeout` (a step that hangs or faults ends there and the next one
is not started), HIP events around each piece, everything of a step in one process on one box:

  short   150 bp: 10,000 queries x one bucket of 1,000,000 subjects, K = 10.  score() alone over the blocks of 1,000
          queries; top_hits(10) over the same blocks; align_hits of the 100,000 hit pairs with the recommended workspace
          (one pass) and with the minimum workspace (one wave per chunk), to price the chunking.
  long    1,000 bp: 1,000 queries x one bucket of 100,000 subjects, K = 10, the same way (10,000 pairs).

Beside the times: the bytes of history the forward kernel writes and the rate that makes, the shader clock eight probe
waves saw and the card's power during the alignment runs (hwmon files, best effort).  The reads are random, as in
scripts/measure_hits.py: the ten best of a random bucket are distant, so their paths wander and their scripts are long.
No ratio is asserted anywhere.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import statistics
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BLOCK = 1000
K_BEST = 10
STEPS = {"short": dict(length=150, queries=10_000, subjects=1_000_000), "long": dict(length=1000, queries=1_000, subjects=100_000)}


def event_ms(torch, fn, reps: int, warmup: int = 1):
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


def run_step(name: str, args) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    import oracle
    from bench import PowerSampler
    L = B.lib()
    shape = STEPS[name]
    length, nq, ns = shape["length"], min(shape["queries"], args.queries or 1 << 30), min(shape["subjects"], args.subjects or 1 << 30)
    q, s = oracle.gen_reads(0xA116_0001, nq, length), oracle.gen_reads(0xA116_1001, ns, length)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    block = min(BLOCK, nq)
    tile = torch.empty((block, a.ns), dtype=torch.int16, device="cuda:0")

    def score_only():
        for lo in range(0, nq, block):
            a.score(lo, min(lo + block, nq), out=tile[: min(lo + block, nq) - lo])

    hits = a.top_hits(K_BEST, block_rows=block)
    a.check_faults()
    n_pairs = nq * K_BEST
    cap = 2 * length
    out3 = (torch.empty((nq, K_BEST), dtype=torch.int32, device="cuda:0"), torch.empty((nq, K_BEST), dtype=torch.int32, device="cuda:0"),
            torch.empty((nq, K_BEST, cap), dtype=torch.int32, device="cuda:0"))
    ws_min = int(L.bgsa_hip_align_pairs_min_workspace_bytes(length, length))
    ws_all = int(L.bgsa_hip_align_pairs_workspace_bytes(length, length, n_pairs))
    a.align_hits(hits[1], into=out3, workspace_bytes=ws_all)      # allocates the workspace before anything is timed
    a.check_faults()
    distance, n_ops, _ = (t.cpu().numpy() for t in out3)
    agree = bool((distance == -hits[0].cpu().numpy()).all())

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"shape": f"{nq} queries x {a.ns_real} subjects x {length} bp Myers global, K = {K_BEST}: {n_pairs} pairs",
           "score_only": event_ms(torch, score_only, args.job_reps),
           "top_hits": event_ms(torch, lambda: a.top_hits(K_BEST, block_rows=block, into=None), args.job_reps)}
    probing = L.bgsa_hip_clock_probe_start(8, 60000, stream) == 0
    sampler = PowerSampler(0.02).start()
    out["align_hits_one_pass"] = event_ms(torch, lambda: a.align_hits(hits[1], into=out3, workspace_bytes=ws_all), args.reps)
    out["align_hits_min_workspace"] = event_ms(torch, lambda: a.align_hits(hits[1], into=out3, workspace_bytes=ws_min), args.reps)
    torch.cuda.synchronize()
    out["power"] = sampler.stop()
    if probing:
        mhz, xcc = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
        n, secs = ctypes.c_int(0), ctypes.c_double(0)
        if L.bgsa_hip_clock_probe_stop(mhz, xcc, 16, ctypes.byref(n), ctypes.byref(secs)) == 0 and n.value:
            out["sustained_mhz"] = round(float(np.mean([mhz[i] for i in range(n.value)])), 1)
    a.check_faults()
    again = tuple(t.cpu().numpy() for t in out3)
    waves = (n_pairs + 63) // 64
    out.update(n_pairs=n_pairs, blocks=-(-nq // block), waves=waves, word_num=a.wn, history_bytes=n_pairs * length * 8 * a.wn, workspace_min=ws_min, workspace_one_pass=ws_all,
               chunks_one_pass=-(-waves // max(1, ws_all // ws_min)), chunks_min_workspace=waves,
               distance_equals_negated_score=agree, chunked_equals_one_pass=bool((again[0] == distance).all() and (again[1] == n_ops).all()),
               mean_distance=round(float(distance.mean()), 2), mean_runs=round(float(n_ops.mean()), 2), max_runs=int(n_ops.max()), cigar_cap=cap)
    return out


def describe(step: dict) -> list[str]:
    score, top = step["score_only"]["median_ms"], step["top_hits"]["median_ms"]
    per_block = score / step["blocks"]
    power = step.get("power") or {}
    lines = [step["shape"],
             f"  shader clock during the alignment runs: {step.get('sustained_mhz', 'not measured')} MHz (probe waves); "
             f"card power {power.get('watts_mean', 'not measured')} W mean, {power.get('watts_max', 'not measured')} W max ({power.get('samples', 0)} samples)",
             "  HIP events, median (min .. max):"]
    for key, label in (("score_only", "score() alone over the blocks"), ("top_hits", f"top_hits({K_BEST}) over the same blocks"),
                       ("align_hits_one_pass", f"align_hits, workspace {step['workspace_one_pass']:,} B, {step['chunks_one_pass']} chunk(s)"),
                       ("align_hits_min_workspace", f"align_hits, minimum workspace {step['workspace_min']:,} B, {step['chunks_min_workspace']} chunks")):
        m = step[key]
        lines.append(f"    {label:<66s} {m['median_ms']:10.3f} ms  ({m['min_ms']:.3f} .. {m['max_ms']:.3f}, {m['reps']} runs)   "
                     f"{m['median_ms'] / score:7.4f} x scoring, {m['median_ms'] / per_block:7.3f} x one block of it")
    one = step["align_hits_one_pass"]["median_ms"]
    lines += [f"  history: {step['history_bytes']:,} bytes written (8 x {step['word_num']} words per row and pair) = "
              f"{step['history_bytes'] / one / 1e6:,.0f} GB/s over the whole one-pass call; {one * 1e3 / step['n_pairs']:.3f} us per pair",
              f"  scripts: mean distance {step['mean_distance']}, mean {step['mean_runs']} runs, longest {step['max_runs']} (cap {step['cigar_cap']}); "
              f"distance == -score for every pair: {step['distance_equals_negated_score']}; chunked == one pass: {step['chunked_equals_one_pass']}",
              f"  aligning the {step['n_pairs']:,} hit pairs costs {'MORE' if one > per_block else 'less'} than scoring one block of {BLOCK} queries "
              f"({one:.3f} ms against {per_block:.3f} ms); top_hits adds {top - score:.3f} ms to the scoring", ""]
    return lines


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "align_pairs.txt"))
    ap.add_argument("--queries", type=int, default=0, help="fewer queries than the step's own count (a quick look)")
    ap.add_argument("--subjects", type=int, default=0, help="fewer subjects than the step's own count")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--job-reps", type=int, default=3)
    ap.add_argument("--step", choices=list(STEPS), help="run one step in this process and print its JSON (used by the driver)")
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds each GPU step may take")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(run_step(args.step, args)))
        return 0
    lines, notes = ["edit scripts of the hit pairs beside scoring and selection (scripts/measure_align_pairs.py)", ""], []
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(Path(__file__).resolve()), "--step", step,
               "--queries", str(args.queries), "--subjects", str(args.subjects), "--reps", str(args.reps), "--job-reps", str(args.job_reps)]
        p = subprocess.run(cmd, capture_output=True, text=True)
        found = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
        if p.returncode != 0 or not found:
            notes.append(f"step {step}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
            break
        lines += describe(json.loads(found[-1][len("RESULT "):]))
    text = "\n".join(lines + notes).rstrip() + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 1 if notes else 0


if __name__ == "__main__":
    sys.exit(main())

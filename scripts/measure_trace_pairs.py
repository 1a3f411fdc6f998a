#!/usr/bin/env python3
"""What score, span and edit script of the hit pairs cost for the aligners bgsa_hip_trace_pairs_dev adds, beside the scoring
and the selection they follow (profiles/trace_pairs.txt).

    python scripts/measure_trace_pairs.py [--out profiles/trace_pairs.txt]

The two jobs of scripts/measure_align_pairs.py —

  short   150 bp: 10,000 queries x one bucket of 1,000,000 subjects, K = 10: 100,000 hit pairs
  long    1,000 bp: 1,000 queries x one bucket of 100,000 subjects, K = 10: 10,000 hit pairs

— for BitPAl 2/-3/-5 global and for Myers semi-global, and for the Myers global aligner through both align_hits (the
bit-parallel forward) and trace_hits (the scalar forward), which prices the scalar DP.  Every GPU step is a child process
of its own under `timeout` (a step that hangs or faults ends there and nothing after it is started): one with HIP events
around score() alone over the blocks of 1,000 queries, top_hits(10) over the same blocks and the trace call (one pass and
minimum workspace), with the shader clock eight probe waves saw and the card's power during the trace runs; and one under
`rocprofv3 --kernel-trace --stats`, a run of its own, for the forward and traceback kernel times (it traces the hit list the
first child left in a temporary file).  What matters is the ratio of the trace call to the scoring of the same job with the
same aligner.  The reads are random: the ten best of a random bucket are distant, so their paths wander.  No ratio is
asserted anywhere.
"""
from __future__ import annotations

import argparse
import csv
import ctypes
import glob
import json
import shutil
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "scripts"))

from measure_align_pairs import BLOCK, K_BEST, STEPS, event_ms  # noqa: E402

ALIGNERS = {"bitpal_global": "BitPAl 2/-3/-5 global", "myers_semi": "Myers semi-global", "myers_global": "Myers global"}
KERNELS = ("trace_pairs_forward_kernel", "trace_pairs_traceback_kernel", "align_pairs_forward_kernel", "align_pairs_traceback_kernel")


def make_aligner(which: str, q, s):
    import bgsa_amd as B
    a = {"bitpal_global": lambda: B.DeviceAligner(B.ALGO_BITPAL, "cuda:0", scores=(2, -3, -5)),
         "myers_semi": lambda: B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True),
         "myers_global": lambda: B.DeviceAligner(B.ALGO_MYERS, "cuda:0")}[which]()
    a.set_queries(q)
    a.set_subjects(s)
    return a


def job(name: str, args):
    import oracle
    shape = STEPS[name]
    length, nq, ns = shape["length"], min(shape["queries"], args.queries or 1 << 30), min(shape["subjects"], args.subjects or 1 << 30)
    return length, nq, ns, oracle.gen_reads(0xA116_0001, nq, length), oracle.gen_reads(0xA116_1001, ns, length)


def trace_outputs(torch, nq, cap):
    def empty(*shape):
        return torch.empty(shape, dtype=torch.int32, device="cuda:0")
    return empty(nq, K_BEST), empty(nq, K_BEST, 4), empty(nq, K_BEST), empty(nq, K_BEST, cap)


def run_step(name: str, which: str, args) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    from bench import PowerSampler
    L = B.lib()
    length, nq, ns, q, s = job(name, args)
    a = make_aligner(which, q, s)
    block = min(BLOCK, nq)
    tile = torch.empty((block, a.ns), dtype=torch.int16, device="cuda:0")

    def score_only():
        for lo in range(0, nq, block):
            a.score(lo, min(lo + block, nq), out=tile[: min(lo + block, nq) - lo])

    hits = a.top_hits(K_BEST, block_rows=block)
    a.check_faults()
    if args.hits_file:
        np.save(args.hits_file, hits[1].cpu().numpy())
    n_pairs = nq * K_BEST
    cap = 2 * length
    out4 = trace_outputs(torch, nq, cap)
    ws_min = int(L.bgsa_hip_align_pairs_min_workspace_bytes(length, length))
    ws_all = int(L.bgsa_hip_align_pairs_workspace_bytes(length, length, n_pairs))
    a.trace_hits(hits[1], into=out4, workspace_bytes=ws_all)      # allocates the workspace before anything is timed
    a.check_faults()
    score, span, n_ops, _ = (t.cpu().numpy() for t in out4)
    agree = bool((score == hits[0].cpu().numpy()).all())

    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"shape": f"{nq} queries x {a.ns_real} subjects x {length} bp {ALIGNERS[which]}, K = {K_BEST}: {n_pairs} pairs", "aligner": which,
           "score_only": event_ms(torch, score_only, args.job_reps),
           "top_hits": event_ms(torch, lambda: a.top_hits(K_BEST, block_rows=block, into=None), args.job_reps)}
    probing = L.bgsa_hip_clock_probe_start(8, 60000, stream) == 0
    sampler = PowerSampler(0.02).start()
    out["trace_hits_one_pass"] = event_ms(torch, lambda: a.trace_hits(hits[1], into=out4, workspace_bytes=ws_all), args.reps)
    if which == "myers_global":
        out3 = (out4[0], out4[2], out4[3])
        out["align_hits_one_pass"] = event_ms(torch, lambda: a.align_hits(hits[1], into=out3, workspace_bytes=ws_all), args.reps)
        a.trace_hits(hits[1], into=out4, workspace_bytes=ws_all)
    else:
        out["trace_hits_min_workspace"] = event_ms(torch, lambda: a.trace_hits(hits[1], into=out4, workspace_bytes=ws_min), max(1, args.reps // 2))
    torch.cuda.synchronize()
    out["power"] = sampler.stop()
    if probing:
        mhz, xcc = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
        n, secs = ctypes.c_int(0), ctypes.c_double(0)
        if L.bgsa_hip_clock_probe_stop(mhz, xcc, 16, ctypes.byref(n), ctypes.byref(secs)) == 0 and n.value:
            out["sustained_mhz"] = round(float(np.mean([mhz[i] for i in range(n.value)])), 1)
    a.check_faults()
    again = tuple(t.cpu().numpy() for t in out4)
    waves = (n_pairs + 63) // 64
    aligned_q, aligned_s = span[:, :, 1] - span[:, :, 0], span[:, :, 3] - span[:, :, 2]
    out.update(n_pairs=n_pairs, blocks=-(-nq // block), waves=waves, word_num=a.wn, cells=n_pairs * length * length,
               history_bytes=n_pairs * length * 8 * a.wn, lds_row_bytes=(length + 1) * 128, workspace_min=ws_min, workspace_one_pass=ws_all,
               chunks_one_pass=-(-waves // max(1, ws_all // ws_min)), chunks_min_workspace=waves, score_equals_hit_score=agree,
               repeat_equals_first=bool((again[0] == score).all() and (again[1] == span).all() and (again[2] == n_ops).all()),
               mean_score=round(float(score.mean()), 2), mean_runs=round(float(n_ops.mean()), 2), max_runs=int(n_ops.max()), cigar_cap=cap,
               mean_aligned_query=round(float(aligned_q.mean()), 1), mean_aligned_subject=round(float(aligned_s.mean()), 1))
    return out


def run_kernels(name: str, which: str, args) -> dict:
    """Under rocprofv3 --kernel-trace: trace (and, Myers global, align) the saved hit list reps + 1 times; nothing else."""
    import numpy as np
    import torch

    import bgsa_amd as B
    L = B.lib()
    length, nq, ns, q, s = job(name, args)
    a = make_aligner(which, q, s)
    hit_subjects = torch.from_numpy(np.load(args.hits_file)).to("cuda:0")
    n_pairs = nq * K_BEST
    out4 = trace_outputs(torch, nq, 2 * length)
    ws_all = int(L.bgsa_hip_align_pairs_workspace_bytes(length, length, n_pairs))
    for _ in range(args.reps + 1):
        a.trace_hits(hit_subjects, into=out4, workspace_bytes=ws_all)
        if which == "myers_global":
            a.align_hits(hit_subjects, into=(out4[0], out4[2], out4[3]), workspace_bytes=ws_all)
    a.check_faults()
    return {"calls": args.reps + 1}


def kernel_times(directory: str, calls: int) -> dict:
    """ms per trace call of each pair kernel, from the run's *kernel_stats.csv (a call launches one pair of kernels per chunk)."""
    files = sorted(glob.glob(directory + "/**/*kernel_stats.csv", recursive=True))
    out = {}
    if not files:
        return out
    for r in csv.DictReader(open(files[-1])):
        for k in KERNELS:
            if k in r["Name"]:
                out[k] = out.get(k, 0.0) + float(r["TotalDurationNs"]) / 1e6 / calls
    return {k: round(v, 4) for k, v in out.items()}


def describe(step: dict) -> list[str]:
    score, top = step["score_only"]["median_ms"], step["top_hits"]["median_ms"]
    per_block = score / step["blocks"]
    power = step.get("power") or {}
    lines = [step["shape"],
             f"  shader clock during the trace runs: {step.get('sustained_mhz', 'not measured')} MHz (probe waves); "
             f"card power {power.get('watts_mean', 'not measured')} W mean, {power.get('watts_max', 'not measured')} W max ({power.get('samples', 0)} samples)",
             "  HIP events, median (min .. max):"]
    rows = [("score_only", "score() alone over the blocks"), ("top_hits", f"top_hits({K_BEST}) over the same blocks"),
            ("trace_hits_one_pass", f"trace_hits, workspace {step['workspace_one_pass']:,} B, {step['chunks_one_pass']} chunk(s)"),
            ("trace_hits_min_workspace", f"trace_hits, minimum workspace {step['workspace_min']:,} B, {step['chunks_min_workspace']} chunks"),
            ("align_hits_one_pass", f"align_hits (bit-parallel forward), same workspace, {step['chunks_one_pass']} chunk(s)")]
    for key, label in rows:
        if key not in step:
            continue
        m = step[key]
        lines.append(f"    {label:<66s} {m['median_ms']:10.3f} ms  ({m['min_ms']:.3f} .. {m['max_ms']:.3f}, {m['reps']} runs)   "
                     f"{m['median_ms'] / score:7.4f} x scoring, {m['median_ms'] / per_block:7.3f} x one block of it")
    one = step["trace_hits_one_pass"]["median_ms"]
    kern = step.get("kernels") or {}
    lines.append("  kernels per one-pass call (rocprofv3 --kernel-trace --stats, a run of its own): " +
                 (", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()) if kern else "not measured"))
    lines += [f"  forward: {step['cells']:,} cells = {step['cells'] / one / 1e6:,.1f} GCUPS over the whole one-pass call, DP row {step['lds_row_bytes']:,} B of LDS per wave; "
              f"history {step['history_bytes']:,} bytes; {one * 1e3 / step['n_pairs']:.3f} us per pair",
              f"  scripts: mean score {step['mean_score']}, mean {step['mean_runs']} runs, longest {step['max_runs']} (cap {step['cigar_cap']}); aligned "
              f"{step['mean_aligned_query']} query x {step['mean_aligned_subject']} subject characters on average; score == the hit list's for every "
              f"pair: {step['score_equals_hit_score']}; repeated and chunked calls equal the first: {step['repeat_equals_first']}",
              f"  tracing the {step['n_pairs']:,} hit pairs costs {'MORE' if one > per_block else 'less'} than scoring one block of {BLOCK} queries "
              f"({one:.3f} ms against {per_block:.3f} ms) and {one / top:.4f} x scoring and selecting the job ({top:.3f} ms)"]
    if "align_hits_one_pass" in step:
        lines.append(f"  scalar forward against bit-parallel forward on the same pairs: {one / step['align_hits_one_pass']['median_ms']:.1f} x the time of align_hits")
    return lines + [""]


def child(args, extra: list[str], limit: int, prefix: list[str] = ()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, str(Path(__file__).resolve()), *extra,
           "--queries", str(args.queries), "--subjects", str(args.subjects), "--reps", str(args.reps), "--job-reps", str(args.job_reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    found = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    return p, (json.loads(found[-1][len("RESULT "):]) if p.returncode == 0 and found else None)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trace_pairs.txt"))
    ap.add_argument("--queries", type=int, default=0, help="fewer queries than the step's own count (a quick look)")
    ap.add_argument("--subjects", type=int, default=0, help="fewer subjects than the step's own count")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--job-reps", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated aligner:step pairs instead of all six, e.g. bitpal_global:short")
    ap.add_argument("--step", help="aligner:step — run it in this process and print its JSON (used by the driver)")
    ap.add_argument("--kernels", help="aligner:step — the traced run (used by the driver, under rocprofv3)")
    ap.add_argument("--hits-file", default="", help="where --step leaves and --kernels finds the hit list")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--no-kernel-trace", action="store_true")
    args = ap.parse_args()
    if args.step or args.kernels:
        which, name = (args.step or args.kernels).split(":")
        print("RESULT " + json.dumps(run_step(name, which, args) if args.step else run_kernels(name, which, args)))
        return 0
    todo = [tuple(x.split(":")) for x in args.only.split(",") if x] or [(w, n) for n in STEPS for w in ALIGNERS]
    lines, notes = ["score, span and edit script of the hit pairs beside scoring and selection (scripts/measure_trace_pairs.py)", ""], []
    tmp = tempfile.mkdtemp(prefix="trace_pairs_")
    try:
        for which, name in todo:
            hits_file = f"{tmp}/{which}_{name}.npy"
            p, step = child(args, ["--step", f"{which}:{name}", "--hits-file", hits_file], args.step_timeout)
            if step is None:
                notes.append(f"step {which}:{name}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
                break
            if not args.no_kernel_trace and shutil.which("rocprofv3"):
                prof = f"{tmp}/prof_{which}_{name}"
                p, traced = child(args, ["--kernels", f"{which}:{name}", "--hits-file", hits_file], args.step_timeout,
                                  ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--"])
                if traced is None:
                    lines += describe(step)
                    notes.append(f"kernel trace of {which}:{name}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
                    break
                step["kernels"] = kernel_times(prof, traced["calls"])
            lines += describe(step)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines + notes).rstrip() + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 1 if notes else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the band-limited edit scripts cost (profiles/align_pairs_banded.txt).

    python scripts/measure_align_pairs_banded.py [--out profiles/align_pairs_banded.txt]

Pair p = (query p, subject p), the subject a copy of the query with about 1 % random edits, so every pair lies within
its bound:

  1000     10,000 pairs of 1,000 bp at B = 64, beside align_pairs on the same pairs (the only baseline that exists)
  4000     2,048 pairs of 4,000 bp at B = 80 (2 %) and B = 200 (5 %)
  10000    1,024 pairs of 10,000 bp at B = 200 (2 %) and B = 500 (5 %)

For each: HIP events around the call (one pass of the default workspace), the workspace, the chunks, score() of the
same queries against the same bucket, and — from a run of its own under `rocprofv3 --kernel-trace --stats` — the forward
and traceback kernel times.  Every GPU step is a child process of its own under `timeout`; after a step that fails
nothing more is started.  No ratio is asserted anywhere: what is measured is recorded.
"""
from __future__ import annotations

import argparse
import csv
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

from measure_align_pairs import event_ms  # noqa: E402

STEPS = {"1000": dict(length=1000, pairs=10_000, bounds=(64,), edits=10),
         "4000": dict(length=4000, pairs=2_048, bounds=(80, 200), edits=40),
         "10000": dict(length=10_000, pairs=1_024, bounds=(200, 500), edits=100)}
KERNELS = ("align_pairs_banded_forward_kernel", "align_pairs_banded_traceback_kernel", "align_pairs_forward_kernel",
           "align_pairs_traceback_kernel")
BLOCK = 1000


def make_aligner(name: str, args):
    import numpy as np

    import bgsa_amd as B
    import oracle
    step = STEPS[name]
    length, pairs = step["length"], min(step["pairs"], args.pairs or 1 << 30)
    q = oracle.gen_reads(0xBA4D_0000 + length, pairs, length)
    s = oracle.mutate(q, np.full(pairs, step["edits"]), 0xBA4D_1000 + length)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    return a, length, pairs


def outputs(torch, pairs, cap):
    return tuple(torch.empty(shape, dtype=torch.int32, device="cuda:0") for shape in ((pairs,), (pairs,), (pairs, cap)))


def run_step(name: str, args) -> dict:
    import torch

    import bgsa_amd as B
    L = B.lib()
    a, length, pairs = make_aligner(name, args)
    idx = torch.arange(pairs, device="cuda:0")
    cap = 4 * STEPS[name]["edits"] + 16
    out3 = outputs(torch, pairs, cap)
    block = min(BLOCK, pairs)
    tile = torch.empty((block, a.ns), dtype=torch.int16, device="cuda:0")

    def score_only():
        for lo in range(0, pairs, block):
            a.score(lo, min(lo + block, pairs), out=tile[: min(lo + block, pairs) - lo])

    waves = (pairs + 63) // 64
    out = {"shape": f"{pairs} pairs of {length} bp ({pairs} queries x {a.ns_real} subjects resident, word_num {a.wn})", "pairs": pairs,
           "length": length, "score_only": event_ms(torch, score_only, args.job_reps), "bounds": {}}
    for bound in STEPS[name]["bounds"]:
        ws_min = int(L.bgsa_hip_align_pairs_banded_min_workspace_bytes(length, length, bound))
        ws_all = int(L.bgsa_hip_align_pairs_banded_workspace_bytes(length, length, bound, pairs))
        a.align_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out3, workspace_bytes=ws_all)      # allocates the workspace before anything is timed
        a.check_faults()
        d, k = out3[0].cpu().numpy(), out3[1].cpu().numpy()
        out["bounds"][str(bound)] = {
            "call": event_ms(torch, lambda: a.align_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out3, workspace_bytes=ws_all), args.reps),
            "band_words": int(L.bgsa_hip_align_pairs_band_words(length, length, bound)), "workspace_min": ws_min, "workspace": ws_all,
            "chunks": -(-waves // max(1, ws_all // ws_min)), "beyond": int((d < 0).sum()), "mean_distance": round(float(d[d >= 0].mean()), 2),
            "mean_runs": round(float(k[d >= 0].mean()), 2), "max_runs": int(k.max()), "cigar_cap": cap}
    if a.wn <= 32:
        full = outputs(torch, pairs, cap)
        ws = int(L.bgsa_hip_align_pairs_workspace_bytes(length, length, pairs))
        a.align_pairs(idx, idx, cigar_cap=cap, into=full, workspace_bytes=ws)
        a.check_faults()
        out["align_pairs"] = {"call": event_ms(torch, lambda: a.align_pairs(idx, idx, cigar_cap=cap, into=full, workspace_bytes=ws), args.reps), "workspace": ws,
                              "workspace_min": int(L.bgsa_hip_align_pairs_min_workspace_bytes(length, length)),
                              "equal": bool(all((x == y).all() for x, y in zip((t.cpu().numpy() for t in full[:2]), (d, k))))}
        out["align_pairs"]["chunks"] = -(-waves // max(1, ws // out["align_pairs"]["workspace_min"]))
    a.check_faults()
    return out


def run_kernels(name: str, args) -> dict:
    """Under rocprofv3 --kernel-trace: every bound's call (and align_pairs where it applies) reps + 1 times; nothing else."""
    import torch

    import bgsa_amd as B
    L = B.lib()
    a, length, pairs = make_aligner(name, args)
    idx = torch.arange(pairs, device="cuda:0")
    cap = 4 * STEPS[name]["edits"] + 16
    out3 = outputs(torch, pairs, cap)
    bound = int(args.bound)
    for _ in range(args.reps + 1):
        if bound >= 0:
            a.align_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out3)
        else:
            a.align_pairs(idx, idx, cigar_cap=cap, into=out3, workspace_bytes=int(L.bgsa_hip_align_pairs_workspace_bytes(length, length, pairs)))
    a.check_faults()
    return {"calls": args.reps + 1}


def kernel_times(directory: str, calls: int) -> dict:
    files = sorted(glob.glob(directory + "/**/*kernel_stats.csv", recursive=True))
    out = {}
    if not files:
        return out
    for r in csv.DictReader(open(files[-1])):
        for k in KERNELS:                       # no name is a substring of another
            if k in r["Name"]:
                out[k] = out.get(k, 0.0) + float(r["TotalDurationNs"]) / 1e6 / calls
    return {k: round(v, 4) for k, v in out.items()}


def describe(step: dict) -> list[str]:
    score = step["score_only"]["median_ms"]
    lines = [step["shape"], f"  score() of the same queries against the same bucket: {score:.3f} ms ({step['score_only']['min_ms']:.3f} .. "
                            f"{step['score_only']['max_ms']:.3f}, {step['score_only']['reps']} runs)"]
    for bound, b in step["bounds"].items():
        c = b["call"]
        kern = b.get("kernels") or {}
        lines += [f"  B = {bound}: window {b['band_words']} of the subject's words; workspace {b['workspace']:,} B (one wave {b['workspace_min']:,} B), "
                  f"{b['chunks']} chunk(s)",
                  f"    align_pairs_banded  {c['median_ms']:10.3f} ms  ({c['min_ms']:.3f} .. {c['max_ms']:.3f}, {c['reps']} runs)   "
                  f"{c['median_ms'] / score:7.4f} x scoring   {c['median_ms'] * 1e3 / step['pairs']:.2f} us per pair",
                  "    kernels per call (rocprofv3 --kernel-trace --stats, a run of its own): " +
                  (", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()) if kern else "not measured"),
                  f"    {b['beyond']} pairs beyond the bound; mean distance {b['mean_distance']}, mean {b['mean_runs']} runs, longest {b['max_runs']} "
                  f"(cap {b['cigar_cap']})"]
    if "align_pairs" in step:
        f = step["align_pairs"]
        c = f["call"]
        kern = f.get("kernels") or {}
        first = next(iter(step["bounds"].values()))["call"]["median_ms"]
        lines += [f"  align_pairs on the same pairs: workspace {f['workspace']:,} B (one wave {f['workspace_min']:,} B), {f['chunks']} chunk(s)",
                  f"    align_pairs         {c['median_ms']:10.3f} ms  ({c['min_ms']:.3f} .. {c['max_ms']:.3f}, {c['reps']} runs)   "
                  f"the banded call takes {first / c['median_ms']:.2f} x its time; distances and run counts equal: {f['equal']}",
                  "    kernels per call: " + (", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()) if kern else "not measured")]
    return lines + [""]


def child(args, extra: list[str], limit: int, prefix: list[str] = ()):
    cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, str(Path(__file__).resolve()), *extra,
           "--pairs", str(args.pairs), "--reps", str(args.reps), "--job-reps", str(args.job_reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    found = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    return p, (json.loads(found[-1][len("RESULT "):]) if p.returncode == 0 and found else None)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "align_pairs_banded.txt"))
    ap.add_argument("--pairs", type=int, default=0, help="fewer pairs than the step's own count (a quick look)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--job-reps", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated steps instead of all three, e.g. 1000,4000")
    ap.add_argument("--step", help="run this step in this process and print its JSON (used by the driver)")
    ap.add_argument("--kernels", help="the traced run of this step (used by the driver, under rocprofv3)")
    ap.add_argument("--bound", default="-1", help="with --kernels: the bound to trace, -1 = align_pairs")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--no-kernel-trace", action="store_true")
    args = ap.parse_args()
    if args.step or args.kernels:
        print("RESULT " + json.dumps(run_step(args.step, args) if args.step else run_kernels(args.kernels, args)))
        return 0
    todo = [x for x in args.only.split(",") if x] or list(STEPS)
    lines, notes = ["band-limited edit scripts of selected pairs beside scoring and align_pairs (scripts/measure_align_pairs_banded.py)", ""], []
    tmp = tempfile.mkdtemp(prefix="align_pairs_banded_")
    try:
        for name in todo:
            p, step = child(args, ["--step", name], args.step_timeout)
            if step is None:
                notes.append(f"step {name}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
                break
            failed = False
            if not args.no_kernel_trace and shutil.which("rocprofv3"):
                targets = [(b, step["bounds"][b]) for b in step["bounds"]] + ([("-1", step["align_pairs"])] if "align_pairs" in step else [])
                for bound, slot in targets:
                    prof = f"{tmp}/prof_{name}_{bound}"
                    p, traced = child(args, ["--kernels", name, "--bound", bound], args.step_timeout,
                                      ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "--"])
                    if traced is None:
                        notes.append(f"kernel trace of {name} (bound {bound}): FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
                        failed = True
                        break
                    slot["kernels"] = kernel_times(prof, traced["calls"])
            lines += describe(step)
            if failed:
                break
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = "\n".join(lines + notes).rstrip() + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 1 if notes else 0


if __name__ == "__main__":
    sys.exit(main())

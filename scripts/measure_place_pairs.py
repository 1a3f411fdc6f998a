#!/usr/bin/env python3
"""What the band-limited semi-global placement costs (profiles/place_pairs_banded.txt).

    python scripts/measure_place_pairs.py [--out profiles/place_pairs_banded.txt]

Pair p = (window p, read p), Myers semi-global: the read is a piece of the window from a random position with about 1 % random
edits, so every pair lies within its bound:

  150      100,000 pairs of 150 bp reads in 400 bp windows at B = 12, beside trace_pairs on the same pairs and aligner
  1000     10,000 pairs of 1,000 bp reads in 1,300 bp windows at B = 64, beside trace_pairs likewise
  4000     2,048 pairs of 4,000 bp reads in 5,000 bp windows at B = 80 and B = 200
  10000    1,024 pairs of 10,000 bp reads in 12,000 bp windows at B = 200

For each: HIP events around the call (median of 5, one pass of the default workspace), the workspace, the chunks, score() of the
same windows against the same bucket, the shader clock eight probe waves saw and the card's power during the placement runs
(hwmon files, best effort), and — from a run of its own under `rocprofv3 --kernel-trace --stats` — the locate, forward and
traceback kernel times.  Where trace_pairs applies its scores, spans and run counts are compared with the placement's.  Every
GPU step is a child process of its own under `timeout`; after a step that fails nothing more is started.  No ratio is asserted
anywhere: what is measured is recorded.
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

from measure_align_pairs import event_ms  # noqa: E402

STEPS = {"150": dict(window=400, length=150, pairs=100_000, bounds=(12,), edits=2),
         "1000": dict(window=1300, length=1000, pairs=10_000, bounds=(64,), edits=10),
         "4000": dict(window=5000, length=4000, pairs=2_048, bounds=(80, 200), edits=40),
         "10000": dict(window=12_000, length=10_000, pairs=1_024, bounds=(200,), edits=100)}
KERNELS = ("place_pairs_locate_kernel", "place_pairs_forward_kernel", "place_pairs_traceback_kernel", "trace_pairs_forward_kernel",
           "trace_pairs_traceback_kernel")
BLOCK = 1000


def make_aligner(name: str, args):
    import numpy as np

    import bgsa_amd as B
    import oracle
    step = STEPS[name]
    window, length, pairs = step["window"], step["length"], min(step["pairs"], args.pairs or 1 << 30)
    q = oracle.gen_reads(0x91AC_0000 + length, pairs, window)
    at = np.random.default_rng(length).integers(0, window - length + 1, size=pairs)
    piece = np.stack([q[p, at[p]: at[p] + length] for p in range(pairs)])
    s = oracle.mutate(piece, np.full(pairs, step["edits"]), 0x91AC_1000 + length)
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True)
    a.set_queries(q)
    a.set_subjects(s)
    return a, window, length, pairs


def outputs(torch, pairs, cap):
    return tuple(torch.empty(shape, dtype=torch.int32, device="cuda:0") for shape in ((pairs,), (pairs, 4), (pairs,), (pairs, cap)))


def run_step(name: str, args) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    from bench import PowerSampler
    L = B.lib()
    a, window, length, pairs = make_aligner(name, args)
    idx = torch.arange(pairs, device="cuda:0")
    cap = 4 * STEPS[name]["edits"] + 16
    out4 = outputs(torch, pairs, cap)
    block = min(BLOCK, pairs)
    tile = torch.empty((block, a.ns), dtype=torch.int16, device="cuda:0")

    def score_only():
        for lo in range(0, pairs, block):
            a.score(lo, min(lo + block, pairs), out=tile[: min(lo + block, pairs) - lo])

    waves = (pairs + 63) // 64
    out = {"shape": f"{pairs} pairs of {length} bp reads in {window} bp windows ({pairs} queries x {a.ns_real} subjects resident, word_num {a.wn})",
           "pairs": pairs, "length": length, "score_only": event_ms(torch, score_only, args.job_reps), "bounds": {}}
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    probing = L.bgsa_hip_clock_probe_start(8, 60000, stream) == 0
    sampler = PowerSampler(0.02).start()
    for bound in STEPS[name]["bounds"]:
        ws_min = int(L.bgsa_hip_place_pairs_banded_min_workspace_bytes(window, length, bound))
        ws_all = int(L.bgsa_hip_place_pairs_banded_workspace_bytes(window, length, bound, pairs))
        a.place_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out4, workspace_bytes=ws_all)      # allocates the workspace before anything is timed
        a.check_faults()
        d, sp, k = out4[0].cpu().numpy(), out4[1].cpu().numpy(), out4[2].cpu().numpy()
        inside = d <= bound
        out["bounds"][str(bound)] = {
            "call": event_ms(torch, lambda: a.place_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out4, workspace_bytes=ws_all), args.reps),
            "band_words": int(L.bgsa_hip_place_pairs_band_words(length, bound)), "workspace_min": ws_min, "workspace": ws_all,
            "chunks": -(-waves // max(1, ws_all // ws_min)), "beyond": int((~inside).sum()), "mean_distance": round(float(d.mean()), 2),
            "mean_runs": round(float(k[inside].mean()), 2) if inside.any() else 0.0, "max_runs": int(k.max()), "cigar_cap": cap}
    torch.cuda.synchronize()
    out["power"] = sampler.stop()
    if probing:
        mhz, xcc = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
        n, secs = ctypes.c_int(0), ctypes.c_double(0)
        if L.bgsa_hip_clock_probe_stop(mhz, xcc, 16, ctypes.byref(n), ctypes.byref(secs)) == 0 and n.value:
            out["sustained_mhz"] = round(float(np.mean([mhz[i] for i in range(n.value)])), 1)
    if a.wn <= 32:
        full = outputs(torch, pairs, cap)
        ws = int(L.bgsa_hip_align_pairs_workspace_bytes(window, length, pairs))
        a.trace_pairs(idx, idx, cigar_cap=cap, into=full, workspace_bytes=ws)
        a.check_faults()
        t_score, t_span, t_ops = (t.cpu().numpy() for t in full[:3])
        out["trace_pairs"] = {"call": event_ms(torch, lambda: a.trace_pairs(idx, idx, cigar_cap=cap, into=full, workspace_bytes=ws), args.reps),
                              "workspace": ws, "workspace_min": int(L.bgsa_hip_align_pairs_min_workspace_bytes(window, length)),
                              "equal": bool((t_score == -d).all() and (t_span[inside] == sp[inside]).all() and (t_ops[inside] == k[inside]).all())}
        out["trace_pairs"]["chunks"] = -(-waves // max(1, ws // out["trace_pairs"]["workspace_min"]))
    a.check_faults()
    return out


def run_kernels(name: str, args) -> dict:
    """Under rocprofv3 --kernel-trace: one bound's call (or trace_pairs, bound -1) reps + 1 times; nothing else."""
    import torch

    import bgsa_amd as B
    L = B.lib()
    a, window, length, pairs = make_aligner(name, args)
    idx = torch.arange(pairs, device="cuda:0")
    cap = 4 * STEPS[name]["edits"] + 16
    out4 = outputs(torch, pairs, cap)
    bound = int(args.bound)
    for _ in range(args.reps + 1):
        if bound >= 0:
            a.place_pairs_banded(idx, idx, bound, cigar_cap=cap, into=out4)
        else:
            a.trace_pairs(idx, idx, cigar_cap=cap, into=out4, workspace_bytes=int(L.bgsa_hip_align_pairs_workspace_bytes(window, length, pairs)))
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
    power = step.get("power") or {}
    lines = [step["shape"], f"  score() of the same windows against the same bucket: {score:.3f} ms ({step['score_only']['min_ms']:.3f} .. "
                            f"{step['score_only']['max_ms']:.3f}, {step['score_only']['reps']} runs)",
             f"  shader clock during the placement runs: {step.get('sustained_mhz', 'not measured')} MHz (probe waves); "
             f"card power {power.get('watts_mean', 'not measured')} W mean, {power.get('watts_max', 'not measured')} W max ({power.get('samples', 0)} samples)"]
    for bound, b in step["bounds"].items():
        c = b["call"]
        kern = b.get("kernels") or {}
        lines += [f"  B = {bound}: window {b['band_words']} of the read's words; workspace {b['workspace']:,} B (one wave {b['workspace_min']:,} B), "
                  f"{b['chunks']} chunk(s)",
                  f"    place_pairs_banded  {c['median_ms']:10.3f} ms  ({c['min_ms']:.3f} .. {c['max_ms']:.3f}, {c['reps']} runs)   "
                  f"{c['median_ms'] / score:7.4f} x scoring   {c['median_ms'] * 1e3 / step['pairs']:.2f} us per pair",
                  "    kernels per call (rocprofv3 --kernel-trace --stats, a run of its own): " +
                  (", ".join(f"{k} {v:.3f} ms" for k, v in kern.items()) if kern else "not measured"),
                  f"    {b['beyond']} pairs beyond the bound; mean distance {b['mean_distance']}, mean {b['mean_runs']} runs, longest {b['max_runs']} "
                  f"(cap {b['cigar_cap']})"]
    if "trace_pairs" in step:
        f = step["trace_pairs"]
        c = f["call"]
        kern = f.get("kernels") or {}
        first = next(iter(step["bounds"].values()))["call"]["median_ms"]
        lines += [f"  trace_pairs on the same pairs and aligner: workspace {f['workspace']:,} B (one wave {f['workspace_min']:,} B), {f['chunks']} chunk(s)",
                  f"    trace_pairs         {c['median_ms']:10.3f} ms  ({c['min_ms']:.3f} .. {c['max_ms']:.3f}, {c['reps']} runs)   "
                  f"the placement takes {first / c['median_ms']:.2f} x its time; scores, spans and run counts equal: {f['equal']}",
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
    ap.add_argument("--out", default=str(ROOT / "profiles" / "place_pairs_banded.txt"))
    ap.add_argument("--pairs", type=int, default=0, help="fewer pairs than the step's own count (a quick look)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--job-reps", type=int, default=2)
    ap.add_argument("--only", default="", help="comma-separated steps instead of all four, e.g. 150,4000")
    ap.add_argument("--step", help="run this step in this process and print its JSON (used by the driver)")
    ap.add_argument("--kernels", help="the traced run of this step (used by the driver, under rocprofv3)")
    ap.add_argument("--bound", default="-1", help="with --kernels: the bound to trace, -1 = trace_pairs")
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--no-kernel-trace", action="store_true")
    args = ap.parse_args()
    if args.step or args.kernels:
        print("RESULT " + json.dumps(run_step(args.step, args) if args.step else run_kernels(args.kernels, args)))
        return 0
    todo = [x for x in args.only.split(",") if x] or list(STEPS)
    lines, notes = ["band-limited semi-global placement beside scoring and trace_pairs (scripts/measure_place_pairs.py)", ""], []
    tmp = tempfile.mkdtemp(prefix="place_pairs_")
    try:
        for name in todo:
            p, step = child(args, ["--step", name], args.step_timeout)
            if step is None:
                notes.append(f"step {name}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")
                break
            failed = False
            if not args.no_kernel_trace and shutil.which("rocprofv3"):
                targets = [(b, step["bounds"][b]) for b in step["bounds"]] + ([("-1", step["trace_pairs"])] if "trace_pairs" in step else [])
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

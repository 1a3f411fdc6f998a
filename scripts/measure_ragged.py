#!/usr/bin/env python3
"""What subject buckets of mixed read lengths cost (profiles/ragged_lengths.txt).

    python scripts/measure_ragged.py [--parent-lib bgsa_amd/_prev/libbgsa_hip_prev.so] [--out profiles/ragged_lengths.txt]

Four measurements, every GPU step a child process of its own under `timeout` (a step that hangs or faults ends there and
nothing after it is started):

  bench      `python bench.py` (Myers 10k x 1M x 150 bp, the equal-length path) twice on the parent's library and twice on this
             one, alternating, on the same box: ms_per_step with the clock each run measured.  The parent's library is a build
             of the parent commit (git archive <commit> bgsa_amd/csrc include | tar -x -C <dir>; make -C <dir>/bgsa_amd/csrc)
             loaded through BGSA_HIP_LIB; without --parent-lib only this library is timed.
  epilogue   10k x 1M x 150 bp Myers with lengths drawn uniformly from 120..150 (the per-lane epilogue, full rows) against the
             same bucket at uniform 150 bp with BGSA_MYERS_BAND=0 (full rows too): GCUPS on padded and on real cells.
  band       the uniform bucket with the band on: what the certified band is worth where a mixed bucket cannot use it.
  binned     align_top_hits_ragged (K = 10) over 1M subjects of lengths 50..300 against ONE padded bucket at 300 bp
             (set_subjects_ragged + top_hits), 1,000 queries of 150 bp.

Nothing is asserted here; the criteria are in the text the script writes.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

BLOCK = 1000


def event_ms(torch, fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1], "reps": reps}


def subjects_with_lengths(ns, width, lens):
    import numpy as np

    import oracle
    rows = oracle.gen_reads(0xA66D_1001, ns, width)
    rows[np.arange(width)[None, :] >= lens[:, None]] = ord("N")
    return rows


def run_scoring(args, mixed: bool) -> dict:
    """score() over blocks of 1,000 queries; mixed: lengths 120..150 through d_lens, else every subject 150 bp."""
    import numpy as np
    import torch

    import bgsa_amd as B
    import oracle
    nq, ns, width = args.queries, args.subjects, 150
    q = oracle.gen_reads(0xA66D_0001, nq, width)
    lens = np.random.default_rng(7).integers(120, 151, ns).astype(np.int32) if mixed else np.full(ns, width, dtype=np.int32)
    lens[0] = width
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    rows = subjects_with_lengths(ns, width, lens)
    padded, extra = B.pad_rows(rows)
    a.ns_real, a.extra = ns, extra
    d_lens = torch.from_numpy(np.concatenate([lens, np.full(extra, width, dtype=np.int32)])).to("cuda:0") if mixed else None
    a.set_subject_rows_device(torch.from_numpy(B.rows_to_buffer(padded)).to("cuda:0"), padded.shape[0], width, None, d_lens=d_lens)
    block = min(BLOCK, nq)
    tile = torch.empty((block, a.ns), dtype=torch.int16, device="cuda:0")

    def score_all():
        for lo in range(0, nq, block):
            a.score(lo, min(lo + block, nq), out=tile[: min(lo + block, nq) - lo])
    t = event_ms(torch, score_all, args.reps)
    a.check_faults()
    stats = (__import__("ctypes").c_ulonglong * 2)()
    B.lib().bgsa_hip_myers_band_stats(stats, 0)
    t.update(padded_cells=nq * ns * width * width, real_cells=int(nq * width * lens.astype(np.int64).sum()), mean_len=float(lens.mean()),
             band_env=os.environ.get("BGSA_MYERS_BAND", ""), banded_queries=int(stats[1]), shape=f"{nq} x {ns} x {width} bp")
    return t


def run_binned(args, binned: bool) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    import oracle
    nq, ns = min(args.queries, 1000), args.subjects
    q = oracle.gen_reads(0xA66D_0002, nq, 150)
    lens = np.random.default_rng(11).integers(50, 301, ns).astype(np.int32)
    rows = oracle.gen_reads(0xA66D_2001, ns, 300)
    subjects = [rows[i, : lens[i]] for i in range(ns)]
    t0 = time.perf_counter()
    if binned:
        scores, ids = B.align_top_hits_ragged(q, subjects, 10, device="cuda:0", block_rows=BLOCK)
    else:
        a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
        a.set_queries(q)
        a.set_subjects_ragged(subjects)
        s, i = a.top_hits(10, block_rows=BLOCK)
        a.check_faults()
        scores, ids = s.cpu().numpy(), i.cpu().numpy()
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    # the device part alone, buckets resident: one more pass over the same bins
    bins = B.bin_by_words(lens) if binned else [np.arange(ns)]
    aligners = []
    for idx in bins:
        a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
        a.set_queries(q)
        a.set_subjects_ragged([subjects[j] for j in idx])
        aligners.append(a)

    def walk():
        into, base = None, 0
        for a in aligners:
            into = a.top_hits(10, block_rows=BLOCK, subject_base=base, into=into)
            base += a.ns_real
    t = event_ms(torch, walk, args.reps)
    for a in aligners:
        a.check_faults()
    t.update(wall_s_with_host_padding_and_upload=wall, bins=len(bins), widths=[int(a.wn) for a in aligners],
             real_cells=int(nq * 150 * lens.astype(np.int64).sum()), checksum=int(scores.astype(np.int64).sum()),
             shape=f"{nq} queries x {ns} subjects of 50..300 bp, K = 10")
    return t


def child(args, extra, limit, env=None):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, str(Path(__file__).resolve()), *extra,
           "--queries", str(args.queries), "--subjects", str(args.subjects), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True, env={**os.environ, **(env or {})})
    found = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    return p, (json.loads(found[-1][len("RESULT "):]) if p.returncode == 0 and found else None)


def bench_once(args, lib):
    env = {**os.environ, **({"BGSA_HIP_LIB": str(lib)} if lib else {})}
    p = subprocess.run(["timeout", "-k", "10", str(args.step_timeout), sys.executable, str(ROOT / "bench.py"), "--gpus", "1",
                        "--steps", str(args.bench_steps), "--warmup", "1"], capture_output=True, text=True, env=env)
    for line in reversed(p.stdout.splitlines()):
        if line.startswith("{"):
            return p, json.loads(line)
    return p, None


def gcups(cells, ms):
    return cells / ms / 1e6


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "ragged_lengths.txt"))
    ap.add_argument("--parent-lib", default="", help="libbgsa_hip.so built from the parent commit (the bench A/B)")
    ap.add_argument("--queries", type=int, default=10000)
    ap.add_argument("--subjects", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds each GPU step may take")
    ap.add_argument("--skip", default="", help="comma-separated: bench, epilogue, band, binned")
    ap.add_argument("--step", help="mixed | uniform | binned | padded — run it in this process and print its JSON (used by the driver)")
    args = ap.parse_args()
    if args.step:
        out = run_scoring(args, args.step == "mixed") if args.step in ("mixed", "uniform") else run_binned(args, args.step == "binned")
        print("RESULT " + json.dumps(out))
        return 0
    skip = set(x for x in args.skip.split(",") if x)
    lines, notes = ["subject buckets of mixed read lengths (scripts/measure_ragged.py)", ""], []

    def failed(what, p):
        notes.append(f"{what}: FAILED with exit status {p.returncode}; nothing after it was run\n{p.stderr[-2000:]}")

    def finish():
        text = "\n".join(lines + notes).rstrip() + "\n"
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
        print(text)
        return 1 if notes else 0

    if "bench" not in skip:
        lines.append("1. the equal-length path: python bench.py --steps %d (Myers 10k x 1M x 150 bp), runs alternating on one box" % args.bench_steps)
        runs = {"parent": [], "this": []}
        order = ["parent", "this", "parent", "this"] if args.parent_lib else ["this", "this"]
        for who in order:
            p, r = bench_once(args, args.parent_lib if who == "parent" else "")
            if r is None:
                failed(f"bench.py ({who})", p)
                return finish()
            clock = r.get("clock") or {}
            runs[who].append(r["ms_per_step"])
            lines.append(f"   {who:<7s} ms_per_step {r['ms_per_step']:.2f}   clock {json.dumps(clock)[:160]}")
        if runs["parent"]:
            spread = max(runs["parent"]) - min(runs["parent"])
            bound = max(runs["parent"]) + max(spread, 0.005 * min(runs["parent"]))
            lines.append(f"   criterion: this <= max(parent) + max(spread of the parent's two runs, 0.5 %) = {bound:.2f} ms; this branch's runs: "
                         f"{', '.join('%.2f' % x for x in runs['this'])} -> {'met' if max(runs['this']) <= bound else 'NOT met'}")
        lines.append("")
    mixed = uniform = None
    if "epilogue" not in skip:
        p, mixed = child(args, ["--step", "mixed"], args.step_timeout)
        if mixed is None:
            failed("mixed lengths", p)
            return finish()
        p, uniform = child(args, ["--step", "uniform"], args.step_timeout, {"BGSA_MYERS_BAND": "0"})
        if uniform is None:
            failed("uniform, full rows", p)
            return finish()
        m, u = mixed["median_ms"], uniform["median_ms"]
        lines += [f"2. the per-lane epilogue: {mixed['shape']} Myers, score() over blocks of {BLOCK} queries, HIP events, median (min .. max) of {mixed['reps']}",
                  f"   lengths uniform in 120..150 (mean {mixed['mean_len']:.2f}), full rows, lens  {m:9.2f} ms ({mixed['min_ms']:.2f} .. {mixed['max_ms']:.2f})   "
                  f"{gcups(mixed['padded_cells'], m):,.0f} GCUPS on padded cells, {gcups(mixed['real_cells'], m):,.0f} on real cells",
                  f"   every subject 150 bp, BGSA_MYERS_BAND=0 (full rows)      {u:9.2f} ms ({uniform['min_ms']:.2f} .. {uniform['max_ms']:.2f})   "
                  f"{gcups(uniform['padded_cells'], u):,.0f} GCUPS",
                  f"   difference {100 * (m - u) / u:+.2f} % of the full-row time (expected of the order of the epilogue's share of a wave-row; above 2 %: see LABNOTES)",
                  ""]
    if "band" not in skip:
        p, banded = child(args, ["--step", "uniform"], args.step_timeout)
        if banded is None:
            failed("uniform, band on", p)
            return finish()
        b = banded["median_ms"]
        lines += [f"3. what the band is worth here (recorded only): every subject 150 bp, band on ({banded['banded_queries']:,} banded wave-queries counted)",
                  f"   {b:9.2f} ms ({banded['min_ms']:.2f} .. {banded['max_ms']:.2f})   {gcups(banded['padded_cells'], b):,.0f} GCUPS"
                  + (f"   = {b / uniform['median_ms']:.3f} x the full-row time; the mixed bucket runs at {mixed['median_ms'] / b:.3f} x this" if uniform and mixed else ""),
                  ""]
    if "binned" not in skip:
        p, binned = child(args, ["--step", "binned"], args.step_timeout)
        if binned is None:
            failed("binned driver", p)
            return finish()
        p, padded = child(args, ["--step", "padded"], args.step_timeout)
        if padded is None:
            failed("one padded bucket", p)
            return finish()
        lines += [f"4. the binned driver: {binned['shape']}, top_hits over resident buckets, HIP events, median of {binned['reps']}",
                  f"   align_top_hits_ragged's bins ({binned['bins']} buckets of {binned['widths']} words)  {binned['median_ms']:9.2f} ms   "
                  f"{gcups(binned['real_cells'], binned['median_ms']):,.0f} GCUPS on real cells   (whole call with host padding and upload: {binned['wall_s_with_host_padding_and_upload']:.1f} s)",
                  f"   one bucket padded to 300 bp ({padded['widths']} words)                      {padded['median_ms']:9.2f} ms   "
                  f"{gcups(padded['real_cells'], padded['median_ms']):,.0f} GCUPS on real cells   (whole call: {padded['wall_s_with_host_padding_and_upload']:.1f} s)",
                  f"   binned / padded = {binned['median_ms'] / padded['median_ms']:.3f}; the hit scores of the two sum to {binned['checksum']} and {padded['checksum']}",
                  ""]
    return finish()


if __name__ == "__main__":
    sys.exit(main())

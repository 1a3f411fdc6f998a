#!/usr/bin/env python3
"""What read buckets of mixed lengths cost in the Myers semi-global mode (profiles/place_lens.txt).

    python scripts/measure_place_lens.py [--out profiles/place_lens.txt] [--queries 1000] [--reads 1000000] [--reps 5]

1,000 queries of 400 bp against 1,000,000 reads of up to 150 bp, score() into one resident tile, HIP events, the median of
--reps repetitions; the runs are taken in turns (a, b, c, d, e, a, b, ...) inside ONE child process under `timeout`, so that they
share the box, its clock and its neighbours:

  a   the equal-length score(): every read 150 bp, myers_semi_asm_kernel<5>                              (the yardstick)
  b   bgsa_hip_myers_place_score_lens_dev with every length equal to 150: myers_semi_asm_kernel<5, true>
  c   the same with lengths uniform in 129..150 (one word count, 22 lengths)
  d   lengths uniform in 33..150 in ONE bucket (5 words wide, 2..5 words used)
  e   the reads of d binned by bin_by_words: four buckets of 2, 3, 4 and 5 words, one launch each

The row loop of a and b is the same code, so b is expected to sit at a; the yardstick's own spread over the repetitions is
printed beside it.  The tiles of a and b are compared bit for bit.  Nothing is asserted; the card's power and shader clock over the
timed region (hwmon files, read on the host) are recorded with the numbers.
"""
from __future__ import annotations

import argparse
import json
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

QLEN, WIDTH = 400, 150
RUNS = ("a", "b", "c", "d", "e")


def bucket(B, torch, q, rows, lens, mark):
    """One resident bucket of `rows` cut to its longest length; lens None: the equal-length path."""
    import numpy as np
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True)
    a.set_queries(q)
    width = rows.shape[1] if lens is None else int(lens.max())
    padded, extra = B.pad_rows(rows[:, :width])
    a.ns_real, a.extra = rows.shape[0], extra
    d_lens = None
    if lens is not None:
        d_lens = torch.from_numpy(np.concatenate([lens, np.full(extra, width, dtype=np.int32)]).astype(np.int32)).to("cuda:0")
    a.set_subject_rows_device(torch.from_numpy(B.rows_to_buffer(padded)).to("cuda:0"), padded.shape[0], width, None, d_lens=d_lens)
    if mark:
        a.mark_reads_ragged()
    return a


def measure(args) -> dict:
    import numpy as np
    import torch

    import bgsa_amd as B
    import oracle
    from bench import PowerSampler
    nq, ns = args.queries, args.reads
    q = oracle.gen_reads(0x91F0_0001, nq, QLEN)
    rows = oracle.gen_reads(0x91F0_1001, ns, WIDTH)
    rng = np.random.default_rng(0x91F0)
    lens_c = rng.integers(129, 151, ns).astype(np.int32)
    lens_d = rng.integers(33, 151, ns).astype(np.int32)
    lens_c[0] = lens_d[0] = WIDTH
    bins = B.bin_by_words(lens_d)
    buckets = {"a": [bucket(B, torch, q, rows, None, False)],
               "b": [bucket(B, torch, q, rows, np.full(ns, WIDTH, dtype=np.int32), True)],
               "c": [bucket(B, torch, q, rows, lens_c, True)],
               "d": [bucket(B, torch, q, rows, lens_d, True)],
               "e": [bucket(B, torch, q, rows[idx], lens_d[idx], True) for idx in bins]}
    widest = max(a.ns for group in buckets.values() for a in group)
    tile = torch.empty((nq, widest), dtype=torch.int16, device="cuda:0")

    def run(name):
        for a in buckets[name]:
            a.score(0, nq, out=tile.view(-1)[: nq * a.ns].view(nq, a.ns))

    for name in RUNS:      # warm-up of every shape, and the bit-for-bit check of b against a
        run(name)
        if name == "a":
            kept = tile.view(-1)[: nq * buckets["a"][0].ns].clone()
        if name == "b":
            same = bool(torch.equal(kept, tile.view(-1)[: nq * buckets["b"][0].ns]))
            del kept
    torch.cuda.synchronize()
    times = {name: [] for name in RUNS}
    sampler = PowerSampler(0.05).start()
    for _ in range(args.reps):
        for name in RUNS:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run(name)
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1))
    power = sampler.stop()
    for group in buckets.values():
        for a in group:
            a.check_faults()
    return {"times_ms": times, "b_equals_a": same, "power": power, "queries": nq, "reads": ns,
            "kernel_a": buckets["a"][0].kernel_name(), "words": {name: [int(a.wn) for a in buckets[name]] for name in RUNS},
            "reads_per_bin": [int(idx.size) for idx in bins],
            "real_cells": {"a": nq * QLEN * ns * WIDTH, "b": nq * QLEN * ns * WIDTH, "c": int(nq * QLEN * lens_c.astype(np.int64).sum()),
                           "d": int(nq * QLEN * lens_d.astype(np.int64).sum()), "e": int(nq * QLEN * lens_d.astype(np.int64).sum())}}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "place_lens.txt"))
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reads", type=int, default=1000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=420, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true", help="measure in this process and print the JSON (used by the driver)")
    args = ap.parse_args()
    if args.child:
        print("RESULT " + json.dumps(measure(args)))
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, str(Path(__file__).resolve()), "--child", "--queries", str(args.queries),
           "--reads", str(args.reads), "--reps", str(args.reps)]
    p = subprocess.run(cmd, capture_output=True, text=True)
    found = [line for line in p.stdout.splitlines() if line.startswith("RESULT ")]
    lines = ["read buckets of mixed lengths, Myers semi-global (scripts/measure_place_lens.py)", ""]
    if p.returncode != 0 or not found:
        lines.append(f"FAILED with exit status {p.returncode}; nothing was measured\n{p.stderr[-2000:]}")
    else:
        r = json.loads(found[-1][len("RESULT "):])
        t = {k: sorted(v) for k, v in r["times_ms"].items()}
        med = {k: v[len(v) // 2] for k, v in t.items()}
        spread = t["a"][-1] - t["a"][0]
        what = {"a": "equal-length score(), every read 150 bp", "b": "per-lane lengths, every length 150",
                "c": "per-lane lengths, uniform in 129..150", "d": "per-lane lengths, uniform in 33..150, ONE bucket",
                "e": "the reads of d binned by words, one bucket per bin"}
        lines.append(f"{r['queries']} queries x {QLEN} bp against {r['reads']} reads, score() into a resident tile, HIP events, "
                     f"median (min .. max) of {len(t['a'])}, runs in turns; kernel of a: {r['kernel_a']}")
        for k in RUNS:
            lines.append(f"  {k}  {what[k]:<52s} {med[k]:9.2f} ms ({t[k][0]:.2f} .. {t[k][-1]:.2f})   words {r['words'][k]}   "
                         f"{r['real_cells'][k] / med[k] / 1e6:,.0f} GCUPS on real cells   {100 * (med[k] - med['a']) / med['a']:+.2f} % of a")
        lines += [f"  the yardstick's own spread (max - min of a): {spread:.2f} ms = {100 * spread / med['a']:.2f} % of its median",
                  f"  b - a = {med['b'] - med['a']:+.2f} ms, c - a = {med['c'] - med['a']:+.2f} ms: "
                  f"{'within' if max(med['b'], med['c']) - med['a'] <= spread else 'ABOVE'} that spread",
                  f"  e / d = {med['e'] / med['d']:.3f} (reads per bin {r['reads_per_bin']})",
                  f"  the tile of b equals the tile of a bit for bit: {r['b_equals_a']}",
                  f"  power / clock over the timed region: {json.dumps(r['power'])}"]
    text = "\n".join(lines).rstrip() + "\n"
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)
    print(text)
    return 0 if found and p.returncode == 0 else 1


if __name__ == "__main__":
    sys.exit(main())

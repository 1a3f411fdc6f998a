"""The banded census on the MI355X: every threshold k = 1 .. 31 of the banded filter at the lengths and inputs of
tests/banded_census.py, under its four configurations — the static grid, the task counter, no survivor queue (every score from the
row loop's own band walk) and the queue taking survivors at the first test that finds at most 32 alive (every score it can from
the dense pass) —, against the plain band DP of the census and against oracle.banded64.  tests/test_banded_census_cpu.py proves on
the host that those lengths reach every placement of a stream event, that the two references and the row simulator agree on every
input, and which route every (wave, query) takes.

One child process per (configuration, block of four thresholds): the knobs are read once per process.  Per shape the child makes
one set_queries, one set_subjects and one score, then check_faults; the int8 result must equal both references exactly, and the
query row whose mapped bytes were overwritten with bytes above 4 must equal its twin.  The flush launches of the census (16 queries
at k = 16 .. 24: the survivor list exactly full in the middle of a tile under the default knobs) run in every configuration too.
The child reports per k the kernel the library names after the launch, which must be the form that k selects (a run under another
kernel cannot pass), the query tile of every launch, which must be the one the host model of the routes assumes, and the shape
count, the launch count and the lengths seen, which must be the census's.  After the first fault word or HIP error the child launches nothing more and says where it
stopped.

Whether a launch took the task counter cannot be observed from outside the library: the `counter` configuration rests on its knob
(BGSA_DYNAMIC_MIN_TASKS=1: launch_rows plans the counter for every launch of at least one task).  The subprocess timeout is a hang
guard, not a measurement."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import banded_census as C  # noqa: E402

pytestmark = pytest.mark.gpu

_CHILD = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
          "import test_banded_census_gpu as T\n"
          "T.run_block(int(sys.argv[2]))\n")


def run_block(block):
    """In the child: every launch of the block; prints one RESULT line."""
    import torch

    B, O = C.B, C.O
    L = B.lib()
    out = {"shapes": 0, "launches": 0, "lengths": {}, "flush": [], "names": {}, "tiles": [], "failures": [], "stopped": None}
    t0 = time.perf_counter()
    for k, length, q, s, foreign, kind in C.cases(block):
        want = C.band_dp(q, s, k)
        if not np.array_equal(want, O.banded64(q, s, k)):
            out["failures"].append([k, length, "the references differ"])
            continue
        try:
            a = B.DeviceAligner(B.ALGO_BANDED, k=k)
            a.set_queries(q)
            if foreign:
                at = torch.tensor([2 * (length + 1) + p for p, _ in foreign], dtype=torch.long, device=a.d_content.device)
                a.d_content[at] = torch.tensor([b for _, b in foreign], dtype=torch.uint8, device=a.d_content.device)
            a.set_subjects(s)
            got = a.score().cpu().numpy()
            a.check_faults()
            out["launches"] += 1
        except Exception as e:      # a fault word or a HIP error: nothing more is launched
            out["stopped"] = [k, length, repr(e)[:300]]
            break
        name = L.bgsa_hip_kernel_name(B.ALGO_BANDED, a.wn).decode()
        if out["names"].setdefault(str(k), name) != name:
            out["failures"].append([k, length, "kernel", name])
        if int(L.bgsa_hip_last_query_tile()) != C.query_tile(length, k, q.shape[0]):
            out["tiles"].append([k, length, int(L.bgsa_hip_last_query_tile()), C.query_tile(length, k, q.shape[0])])
        if got.dtype != np.int8 or got.shape != want.shape:
            out["failures"].append([k, length, "result", str(got.dtype), list(got.shape)])
        elif not np.array_equal(got, want):
            row, lane = (int(x) for x in np.argwhere(got != want)[0])
            out["failures"].append([k, length, row, lane, int(got[row, lane]), int(want[row, lane]), int((got != want).sum())])
        elif kind == "census" and not np.array_equal(got[2], got[1]):
            out["failures"].append([k, length, "the foreign-byte row differs from its twin"])
        out["shapes"] += 1
        if kind == "census":
            out["lengths"].setdefault(str(k), []).append(length)
        else:
            out["flush"].append([k, length, int(L.bgsa_hip_last_query_tile())])
    out["seconds"] = round(time.perf_counter() - t0, 2)
    if out["stopped"] is None:
        out["stream_faults"] = int(L.bgsa_hip_stream_faults(1))
    print("RESULT " + json.dumps(out))


@pytest.mark.parametrize("config,block", [(c, b) for c in C.CONFIGS for b in C.blocks()], ids=lambda x: str(x))
def test_banded_census(config, block):
    shapes = C.shapes(block) + C.flush_shapes(block)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(C.ROOT), str(block)], capture_output=True, text=True,
                       timeout=60 + len(shapes) // 2, env=C.child_env(config, os.environ), cwd=str(C.ROOT))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
    print(f"banded census {config}, thresholds {C.block_thresholds(block)}: {r['shapes']} shapes, {r['launches']} launches, "
          f"{r['seconds']} s in the loop")
    assert r["stopped"] is None, r["stopped"]
    assert not r["failures"], (f"{len(r['failures'])} differences, the first: (k, length, query, lane, got, want, pairs that differ) = "
                               f"{r['failures'][:5]}")
    assert r["stream_faults"] == 0
    assert not r["tiles"], f"(k, length, the launch's query tile, the model's) = {r['tiles'][:5]}"
    assert r["shapes"] == r["launches"] == len(shapes)
    assert r["lengths"] == {str(k): list(C.lengths(k)) for k in C.block_thresholds(block)}
    assert r["flush"] == [[k, n, C.FLUSH_NQ] for k, n in C.flush_shapes(block)]      # a query tile of 16: the list can fill inside it
    assert r["names"] == {str(k): C.kernel_name(k) for k in C.block_thresholds(block)}

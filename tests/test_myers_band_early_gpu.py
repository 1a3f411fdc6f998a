"""GPU parity of the early leave of the certified Myers band (myers_band.h, LABNOTES §37): the RESCUE
instantiations myers_global_asm_kernel<NW, 2, *, true, false, *, true> on the schedule with the cuts applied, every lane certified
against its own limit min(B, M), and myers_band_rescue_kernel<NW> on the lanes above it.

Every run is a child process that pins BGSA_MYERS_BAND_GROUPS=2, BGSA_MYERS_BAND_RESCUE=1 and BGSA_MYERS_BAND_EARLY=1 (the
knobs are read once).  192 subjects — three groups, the second wave has one live group — at 150 x 150, 100 x 100 and 68 x 68 (the
shortest four- and three-word lengths with cuts), from tests/band_early_family.py: random reads, copies with 0 .. 5 edits, the
band-edge ladders and the rotations, no group with more than eight lanes above their limit.  Every score must equal
oracle.dp_edit; `lanes rescued` must equal the host model's count of D' > limit EXACTLY (tests/test_myers_band_early_cpu.py is
what makes the model right), and nothing may be redone — except in the bucket whose third group holds nine such lanes for
query 0.  The same on the static grid and on the counter, with prefix sharing off (6 queries) and forced on with depths 2,3
(24 queries).  BGSA_MYERS_BAND_EARLY=0 gives the same scores and the parent's counts, the pairs with D > B; one capture in a
graph replayed twice gives the same scores and counts.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
LENGTHS = (150, 100, 68)

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import ctypes, numpy as np
import band_early_family as F
import bgsa_amd as B
nq = int(sys.argv[2])
L = B.lib()
def pair(fn):
    st = (ctypes.c_ulonglong * 2)(); assert fn(st, 1) == 0
    return [int(st[0]), int(st[1])]
def run(a, first, last):
    pair(L.bgsa_hip_myers_band_stats); pair(L.bgsa_hip_myers_band_rescue_stats)
    got = -a.score(first, last).cpu().numpy().astype(np.int64)      # scores are negated distances
    a.check_faults()
    return got, pair(L.bgsa_hip_myers_band_stats), pair(L.bgsa_hip_myers_band_rescue_stats)
out = {}
for n in F.LENGTHS:
    d = F.build(n)
    q, bp = d["q"][:nq], 2 * d["h"] + 1
    pick = np.arange(nq) % F.N_DISTINCT
    r = {"bp": bp, "cuts": [list(c) for c in d["cuts"]]}
    for name in ("base", "nine"):
        over = d[name + "_over"][pick].reshape(nq, 3, 64).sum(axis=2)           # the model: lanes with D' > limit, [query, group]
        above = (d[name + "_want"][pick] > bp).reshape(nq, 3, 64).sum(axis=2)   # the parent's: pairs with D > B
        r[name + "_over"], r[name + "_above"] = over.tolist(), above.tolist()
    rows = (ctypes.c_int * 2)()
    r["early"] = [int(rows[j]) for j in range(L.bgsa_hip_myers_band_early(n, n, nq, 192, rows))]
    r["groups"] = int(L.bgsa_hip_myers_band_groups((n + 31) // 32, 192, n, n, 0))
    r["rescue_half"] = int(L.bgsa_hip_myers_band_rescue(n, n, nq, 192))
    dd = (ctypes.c_int * 8)()
    r["depths"] = [int(dd[j]) for j in range(L.bgsa_hip_myers_prefix_depths((n + 31) // 32, 192, n, n, nq, 0, dd, 8))]
    a = B.DeviceAligner(B.ALGO_MYERS)
    a.set_queries(q)
    a.set_subjects(d["base"])
    got, bs, rs = run(a, 0, nq)
    r["base"] = [bool(np.array_equal(got, d["base_want"][pick])), bs, rs]
    a.set_subjects(d["nine"])
    got, bs, rs = run(a, 0, 1)
    r["nine"] = [bool(np.array_equal(got, d["nine_want"][:1])), bs, rs]
    out[str(n)] = r
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""

GRAPH_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import ctypes, numpy as np, torch
import band_early_family as F
import bgsa_amd as B
L = B.lib()
d = F.build(150)
q, s, want = d["q"][:6], d["base"], -d["base_want"]
a = B.DeviceAligner(B.ALGO_MYERS)
a.set_queries(q); a.set_subjects(s)
out = torch.zeros(want.shape, dtype=torch.int16, device="cuda:0")
a.score(out=out)                                   # warm-up allocates the workspace outside the capture
a.check_faults()
st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_rescue_stats(st, 1)
first = [int(st[0]), int(st[1])]
side = torch.cuda.Stream()
graph = torch.cuda.CUDAGraph()
with torch.cuda.stream(side):
    with torch.cuda.graph(graph, stream=side):
        a.score(out=out)
torch.cuda.synchronize()
L.bgsa_hip_myers_band_rescue_stats(st, 1)
replays = []
for _ in range(2):
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    a.check_faults()
    L.bgsa_hip_myers_band_rescue_stats(st, 1)
    replays.append([bool(np.array_equal(out.cpu().numpy(), want)), int(st[0]), int(st[1])])
rows = (ctypes.c_int * 2)()
print("RESULT " + json.dumps({"first": first, "replays": replays, "model": int(d["base_over"].sum()),
                              "early": [int(rows[j]) for j in range(L.bgsa_hip_myers_band_early(150, 150, 6, 192, rows))]}))
"""

PIN = {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_MYERS_BAND_RESCUE": "1", "BGSA_MYERS_BAND_EARLY": "1"}
TILE = {"BGSA_TASK_TARGET": "1", "BGSA_DYNAMIC_TASK_TARGET": "1"}      # the largest tile: sharing needs 16 queries per task
GRIDS = {"static": {"BGSA_DYNAMIC_TASKS": "0"}, "counter": {"BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"}}
_runs = {}


def _child(script, env_extra, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BGSA_MYERS_BAND")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", script, str(ROOT)] + [str(x) for x in args], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def _run(grid, share):
    """Every length in one child: all queries on the base bucket, then query 0 on the bucket with nine lanes in one group."""
    key = (grid, share)
    if key not in _runs:
        env = dict(PIN, **GRIDS[grid], **TILE, BGSA_MYERS_PREFIX_SHARE="2,3" if share else "0")
        _runs[key] = _child(CHILD, env, 24 if share else 6)
    return _runs[key]


def _sum(table, groups=(0, 1, 2)):
    return sum(row[g] for row in table for g in groups)


@pytest.mark.parametrize("share", [False, True], ids=["no sharing", "sharing 2,3"])
@pytest.mark.parametrize("grid", ["static", "counter"])
@pytest.mark.parametrize("length", LENGTHS)
def test_scores_exact_and_rescued_lanes_are_the_models(length, grid, share):
    r = _run(grid, share)[str(length)]
    nq = 24 if share else 6
    # the input conditions: lanes above their limit that B certifies, never more than eight of a group
    assert _sum(r["base_over"]) > _sum(r["base_above"]) > 0 and max(max(row) for row in r["base_over"]) <= 8, r
    assert r["groups"] == 2 and r["rescue_half"] == (r["bp"] - 1) // 2 and r["depths"] == ([2, 3] if share else []), r
    assert r["early"] == [c[0] for c in r["cuts"]] and r["early"], r
    exact, (redone, banded), (rescued, forced) = r["base"]
    assert exact, r
    assert rescued == _sum(r["base_over"]), r           # EXACTLY the model's lanes with D' > limit
    assert (redone, banded, forced) == (0, 3 * nq, 0), r


@pytest.mark.parametrize("share", [False, True], ids=["no sharing", "sharing 2,3"])
@pytest.mark.parametrize("grid", ["static", "counter"])
@pytest.mark.parametrize("length", LENGTHS)
def test_nine_lanes_of_a_group_take_the_redo(length, grid, share):
    """Query 0: the second wave's one live group holds nine lanes above their limit.  That wave runs the query again with full rows
    and is counted in the second statistic; the first wave's lanes are rescued as without it."""
    r = _run(grid, share)[str(length)]
    assert r["nine_over"][0][2] == 9 and max(r["nine_over"][0][:2]) <= 8, r
    assert r["nine"] == [True, [1, 3], [_sum(r["nine_over"][:1], (0, 1)), 1]], r


def test_early_leave_forced_off_gives_the_same_scores_and_the_parents_counts():
    env = dict(PIN, **GRIDS["static"], BGSA_MYERS_PREFIX_SHARE="0", BGSA_MYERS_BAND_EARLY="0")
    for name, r in _child(CHILD, env, 6).items():
        assert r["early"] == [] and r["groups"] == 2 and r["rescue_half"] == (r["bp"] - 1) // 2, (name, r)
        assert r["base"] == [True, [0, 18], [_sum(r["base_above"]), 0]], (name, r)      # the pairs with D > B
        assert max(r["nine_above"][0]) <= 8 and r["nine"] == [True, [0, 3], [_sum(r["nine_above"][:1]), 0]], (name, r)


def test_graph_capture_replays_the_early_leave():
    r = _child(GRAPH_CHILD, dict(PIN, **GRIDS["static"]))
    assert r["early"] == [106, 130] and r["first"] == [r["model"], 0] and r["model"] > 0, r
    for exact, rescued, forced in r["replays"]:
        assert exact and [rescued, forced] == r["first"], r

"""GPU parity of the rescue of the certified Myers band (myers_band.h): myers_global_asm_kernel<NW, 2, *, true, false,
*, true> on a band three narrower than the default, and myers_band_rescue_kernel<NW> on the lanes it did not certify.

The launcher rescues on large buckets only, so every run is a child process that pins BGSA_MYERS_BAND_GROUPS=2 and
BGSA_MYERS_BAND_RESCUE=1 (the knobs are read once).  192 subjects — three groups, the second wave has one live group — at
150 x 150, 100 x 97 and 65 x 65, taken from the ladders of oracle/band_edge.py: distances B' - 1, B', B' + 1, B' + 2, B' + 3 and
one above the default B (B' = 2 x rescue half-width + 1), the uncertified ones at lanes 0, 31, 32 and 63 of either group of
the first wave (and at 31, 32 of the second wave's one group), among copies of the
query with up to 20 edits.  Every score must equal oracle.dp_edit; `lanes rescued` must equal the number of pairs with
D > B' EXACTLY (tests/test_myers_band_rescue_cpu.py is what makes that the right count), and no query may be redone.  The
same on the static grid and on the counter, with prefix sharing off (6 queries) and forced on (24 queries that share their
first rows: sharing needs a tile of 16).  One query then goes through the variants: a group with nine lanes above B' (the
redo), a pool of two entries for five uncertified pairs, and rescue forced off.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
SHAPES = [(150, 150), (100, 97), (65, 65)]

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/bgsa_amd/csrc")
import ctypes, numpy as np
import oracle as O
from oracle import band_edge as E
import rows_ir as R
mode, shapes, nq = sys.argv[2], json.loads(sys.argv[3]), int(sys.argv[4])

def dist(q, s):
    return -O.dp_edit(q, s).astype(np.int64)

def build(m, n):
    # -> queries [24, m], and per variant the 192 subjects
    h = R.myers_band_rescue_half(max(m, n))
    bp, bd = 2 * h + 1, 2 * R.myers_band_half(max(m, n)) + 1
    q0 = E.three_run_query(m)
    rungs, _ = E.band_edge_pairs(q0, n, h, near=8)
    d = dist(q0[None], rungs)[0]
    def rung(want, k=0):
        at = np.flatnonzero(d == want)
        assert len(at), (m, n, want, sorted(set(d.tolist())))
        return rungs[at[k % len(at)]]
    far = int(d[d > bd].min())                       # the nearest rung above the default B
    k = min(m, n)
    fill = O.gen_reads(900 + m, 192, n)
    fill[:, :k] = O.mutate(np.repeat(q0[None, :k], 192, axis=0), np.arange(192) % 21, 31 + m)
    assert (dist(q0[None], fill)[0] <= 20 + abs(n - m)).all()
    def bucket(lanes):
        s = fill.copy()
        for (g, lane), want in lanes.items():
            s[64 * g + lane] = rung(want, g)
        return np.ascontiguousarray(s)
    near = {(0, 1): bp, (0, 2): bp - 1, (1, 5): bp, (2, 7): bp - 1}
    sets = {
        "base": bucket({(0, 0): bp + 1, (0, 31): bp + 3, (0, 32): far, (0, 63): bp + 2,
                        (1, 0): bp + 1, (1, 31): bp + 2, (1, 32): bp + 3, (1, 63): far,      # the second group's ranks start behind the first's
                        (2, 31): bp + 3, (2, 32): bp + 1, **near}),
        "nine": bucket({(0, 0): bp + 1, (0, 31): bp + 3, (0, 32): far, (0, 63): bp + 2,
                        (1, 0): bp + 1, (1, 31): bp + 2, (1, 32): bp + 3, (1, 63): far,
                        **{(2, 3 * j): bp + 1 + j % 3 for j in range(9)}, **near}),
        "five": bucket({(0, 0): bp + 1, (0, 63): bp + 2, (1, 31): bp + 3, (2, 32): bp + 1, (2, 33): far, **near}),
    }
    # the queries: q0, then q0 with i % 6 substitutions behind its first rows (sorted neighbours share at least 10 rows)
    q = np.repeat(q0[None], 24, axis=0)
    for i in range(24):
        for j in range(i % 6):
            at = 12 + ((7 * i + 11 * j) % (m - 14))
            q[i, at] = {ord("A"): ord("C"), ord("C"): ord("T"), ord("T"): ord("A")}[int(q[i, at])]
    return np.ascontiguousarray(q), sets, bp, bd

out = {}
if mode != "build":
    import bgsa_amd as B
    L = B.lib()
def band_stats():
    st = (ctypes.c_ulonglong * 2)(); assert L.bgsa_hip_myers_band_stats(st, 1) == 0
    return [int(st[0]), int(st[1])]
def rescue_stats():
    st = (ctypes.c_ulonglong * 2)(); assert L.bgsa_hip_myers_band_rescue_stats(st, 1) == 0
    return [int(st[0]), int(st[1])]
def run(a, first, last):
    band_stats(); rescue_stats()
    got = -a.score(first, last).cpu().numpy().astype(np.int64)      # scores are negated distances
    a.check_faults()
    return got, band_stats(), rescue_stats()

for m, n in shapes:
    q, sets, bp, bd = build(m, n)
    q = q[:nq]
    want = {k: dist(q, s) for k, s in sets.items()}
    over = {k: (w > bp).reshape(nq, 3, 64).sum(axis=2) for k, w in want.items()}      # [query, group]
    r = {"bp": bp, "bd": bd, "over_base_max": int(over["base"].max()), "over_base": int(over["base"].sum()),
         "over_nine": over["nine"][0].tolist(), "over_five": over["five"][0].tolist(),
         "seen": sorted(set((want["base"][0] - bp).tolist()) & set(range(-1, 12)))}
    if mode != "build":
        nw = (n + 31) // 32
        r["groups"] = int(L.bgsa_hip_myers_band_groups(nw, 192, m, n, 0))
        r["rescue_half"] = int(L.bgsa_hip_myers_band_rescue(m, n, nq, 192))
        d = (ctypes.c_int * 8)()
        r["depths"] = [int(d[j]) for j in range(L.bgsa_hip_myers_prefix_depths(nw, 192, m, n, nq, 0, d, 8))]
        a = B.DeviceAligner(B.ALGO_MYERS)
        a.set_queries(q)
        if mode == "all":
            a.set_subjects(sets["base"])
            got, bs, rs = run(a, 0, nq)
            r["base"] = [bool(np.array_equal(got, want["base"])), bs, rs]
        a.set_subjects(sets["base"])
        got, bs, rs = run(a, 0, 1)
        r["one"] = [bool(np.array_equal(got, want["base"][:1])), bs, rs]
        a.set_subjects(sets["nine"])
        got, bs, rs = run(a, 0, 1)
        r["nine"] = [bool(np.array_equal(got, want["nine"][:1])), bs, rs]
        a.set_subjects(sets["five"])
        got, bs, rs = run(a, 0, 1)
        r["five"] = [bool(np.array_equal(got, want["five"][:1])), bs, rs]
    out["%dx%d" % (m, n)] = r
if mode != "build":
    assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""

GRAPH_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np, torch
import bgsa_amd as B, oracle as O
L = B.lib()
q = O.gen_reads(71, 6, 150)
s = O.gen_reads(72, 192, 150)                      # random pairs: a few lanes per group lie above the B of the knob
s[:60] = O.mutate(q[np.arange(60) % 6], np.arange(60) % 25, 5)
want = O.dp_edit(q, s)
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
print("RESULT " + json.dumps({"first": first, "replays": replays, "rescue_half": int(L.bgsa_hip_myers_band_rescue(150, 150, 6, 192))}))
"""

PIN = {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_MYERS_BAND_RESCUE": "1"}
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
    """Every shape in one child: all queries on the base bucket, then query 0 through the variants."""
    key = (grid, share)
    if key not in _runs:
        env = dict(PIN, **GRIDS[grid], **TILE, BGSA_MYERS_PREFIX_SHARE="2,3" if share else "0")
        _runs[key] = _child(CHILD, env, "all", json.dumps(SHAPES), 24 if share else 6)
    return _runs[key]


@pytest.mark.parametrize("share", [False, True], ids=["no sharing", "sharing 2,3"])
@pytest.mark.parametrize("grid", ["static", "counter"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_rescued_lanes_exact_scores_and_counts(shape, grid, share):
    r = _run(grid, share)["%dx%d" % shape]
    nq = 24 if share else 6
    # the input conditions: distances B' - 1 .. B' + 3 and one above the default B; never more than eight lanes of a group above B'
    assert set(range(-1, 4)) <= set(r["seen"]) and max(r["seen"]) > r["bd"] - r["bp"] and 0 < r["over_base_max"] <= 8, r
    assert r["groups"] == 2 and r["rescue_half"] == (r["bp"] - 1) // 2 and r["depths"] == ([2, 3] if share else []), r
    exact, (redone, banded), (rescued, forced) = r["base"]
    assert exact, r
    assert rescued == r["over_base"], r                 # EXACTLY the pairs with D > B'
    assert (redone, banded, forced) == (0, 3 * nq, 0), r


@pytest.mark.parametrize("share", [False, True], ids=["no sharing", "sharing 2,3"])
@pytest.mark.parametrize("grid", ["static", "counter"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_nine_lanes_of_a_group_take_the_redo(shape, grid, share):
    """Query 0: the second wave's one live group holds nine lanes above B'.  That wave runs the query again with full rows and is
    counted in the second statistic; the first wave's eight lanes are rescued as without it."""
    r = _run(grid, share)["%dx%d" % shape]
    assert r["over_nine"] == [4, 4, 9] and r["one"] == [True, [0, 3], [10, 0]], r
    assert r["nine"] == [True, [1, 3], [8, 1]], r


def test_a_full_pool_sends_the_rest_through_the_redo():
    """A pool of two entries, five uncertified pairs: wave 0 claims three — they do not fit, it runs the query again with full rows,
    two group-queries — and wave 1 claims two, which fit if it comes first.  Either way the scores are exact."""
    env = dict(PIN, **GRIDS["static"], BGSA_MYERS_PREFIX_SHARE="0", BGSA_MYERS_BAND_RESCUE_POOL="2")
    for name, r in _child(CHILD, env, "variants", json.dumps(SHAPES), 6).items():
        assert r["over_five"] == [2, 1, 2], r
        exact, (redone, banded), (rescued, forced) = r["five"]
        assert exact and banded == 3, (name, r)
        assert (rescued, redone, forced) in ((2, 2, 2), (0, 3, 3)), (name, r)


def test_rescue_forced_off_gives_the_same_scores():
    env = dict(PIN, **GRIDS["static"], BGSA_MYERS_PREFIX_SHARE="0", BGSA_MYERS_BAND_RESCUE="0")
    for name, r in _child(CHILD, env, "all", json.dumps(SHAPES), 6).items():
        assert r["rescue_half"] == 0 and r["groups"] == 2, (name, r)
        for key in ("base", "one", "nine", "five"):
            assert r[key][0] and r[key][2] == [0, 0], (name, key, r)


def test_graph_capture_replays_the_rescue():
    """BGSA_MYERS_BAND=43 (B = 87 at 150 bp): about three random pairs in a hundred lie above it, a few per group — the capture
    holds the scoring kernel, the rescue kernel and the statistics, and nothing is read back between them."""
    r = _child(GRAPH_CHILD, dict(PIN, **GRIDS["static"], BGSA_MYERS_BAND="43"))
    assert r["rescue_half"] == 43 and r["first"][0] > 0, r
    for exact, rescued, forced in r["replays"]:
        assert exact and [rescued, forced] == r["first"], r

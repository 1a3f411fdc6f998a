"""GPU parity of prefix sharing in the certified band's kernels: myers_global_asm_kernel<NW, G, *, true> walking
its tile in sorted order and resuming every query behind the rows it shares with its predecessor.

Sharing must not change a score or a count.  Every case runs in a child process with its knobs pinned (they are read once):
one and two subject groups per wave, static grid and counter grid, the depths 5,6,7 and 2,3, and sharing off as the
reference.  About 300 queries of the family of tests/prefix_family.py in shuffled order against 192 subjects — three groups,
so the last wave of the two-group kernel has a dead second group.  Each child asserts through bgsa_hip_myers_prefix_depths
that its launches share (or, for the reference, do not), so no case can pass with the feature silently off.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import ctypes, numpy as np
import bgsa_amd as B, oracle as O
from prefix_family import family
L = B.lib()
want_depths = json.loads(sys.argv[2])
def stats():
    st = (ctypes.c_ulonglong * 2)(); assert L.bgsa_hip_myers_band_stats(st, 1) == 0
    return [int(st[0]), int(st[1])]
def depths(nq, ns):
    d = (ctypes.c_int * 8)()
    n = L.bgsa_hip_myers_prefix_depths(5, ns, 150, 150, nq, 0, d, 8)
    return list(d[:n])
rng = np.random.default_rng(11)
q = np.concatenate([family(150, seed) for seed in range(5)])
q = np.ascontiguousarray(q[rng.permutation(len(q))])
nq = len(q)
s = O.gen_reads(77, 192, 150)
s[:96] = O.mutate(q[np.arange(96) * 3 % nq], np.arange(96) % 30, 5)
out = {"nq": nq, "depths": depths(nq, 192), "sub_depths": depths(100, 192)}
assert out["depths"] == want_depths and out["sub_depths"] == want_depths, out
a = B.DeviceAligner(B.ALGO_MYERS)
a.set_queries(q)
a.set_subjects(s)
stats()
got = a.score().cpu().numpy()
out["stats"] = stats()
# what the launch left behind its streams: the sorted order, and every query's start segment — the device really resumes
if want_depths:
    import torch
    from prefix_family import CODE, sorted_order
    off = (ctypes.c_int * 8)(); dd = (ctypes.c_int * len(want_depths))(*want_depths)
    stride = L.bgsa_hip_myers_band_segments(CODE[q[0]].ctypes.data_as(ctypes.c_void_p), 150, 150, dd, len(want_depths), None, 0, off)
    at = (stride * nq + 255) // 256 * 256 + 512          # myers_band.h: prefix_entries behind task_counter_in
    e = a.d_work[at:at + 8 * nq].view(torch.int32).cpu().numpy().reshape(nq, 2)
    tile = int(L.bgsa_hip_last_query_tile())
    order, lcp = sorted_order(q, want_depths, tile)
    seg = [sum(1 for d in want_depths if d <= x) for x in lcp]
    out["tile"] = tile
    out["entries"] = bool(np.array_equal(e[:, 0], order) and np.array_equal(e[:, 1] & 0xffff, lcp) and np.array_equal(e[:, 1] >> 16, seg))
    out["resumed"] = int((e[:, 1] >> 16 > 0).sum())
want = O.dp_edit(q, s)
out["exact"] = bool(np.array_equal(got, want))
out["scores"] = got.astype(np.int64).tolist()
# a sub-range, and two adjacent sub-ranges: the same rows
out["window"] = bool(np.array_equal(a.score(37, 137).cpu().numpy(), want[37:137]))
out["windows"] = bool(np.array_equal(np.concatenate([a.score(0, 100).cpu().numpy(), a.score(100, nq).cpu().numpy()]), want))
# the same queries given in another order
perm = rng.permutation(nq)
a.set_queries(np.ascontiguousarray(q[perm]))
out["reordered"] = bool(np.array_equal(a.score().cpu().numpy(), want[perm]))
# redo: lane 6 of group 1 holds a poly-G read, distance 150 - (G's of the query) > B: that wave runs every query twice.  21 queries,
# neighbours in sorted order: 63 group-queries, too few for the guard to stop the banding, so the counts are exact
by_text = sorted(range(nq), key=lambda i: q[i].tobytes())
share = [int(np.argmin(np.append(q[i] == q[j], False))) >= want_depths[0] if want_depths else True for i, j in zip(by_text, by_text[1:])]
at = max(range(nq - 21), key=lambda k: sum(share[k:k + 20]))
q2 = np.ascontiguousarray(q[[by_text[k] for k in rng.permutation(21) + at]])
out["redo_sharing_neighbours"] = int(sum(share[at:at + 20]))
s2 = s.copy(); s2[70] = ord("G")
want2 = O.myers64(q2, s2)
assert (-want2[:, 70].astype(np.int64) > 97).all()
assert depths(21, 192) == want_depths
a.set_queries(q2); a.set_subjects(s2)
stats()
out["redo_exact"] = bool(np.array_equal(a.score().cpu().numpy(), want2))
out["redo_stats"] = stats()
over = (-want2.astype(np.int64) > 97).reshape(21, 3, 64).any(axis=2)
out["redo_want"] = [int(over.sum()), 3 * 21]
a.set_queries(q)
# guard off: every subject far from every query, the waves stop banding mid-launch
s3 = np.full((192, 150), ord("N"), dtype=np.uint8)
a.set_subjects(s3)
stats()
out["far_exact"] = bool(np.array_equal(a.score().cpu().numpy(), O.myers64(q, s3)))
out["far_stats"] = stats()
a.check_faults()
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""

TILE = {"BGSA_TASK_TARGET": "1", "BGSA_DYNAMIC_TASK_TARGET": "1"}      # the largest tile: 32 queries on the static grid, 128 on the counter
GRIDS = {"static": {"BGSA_DYNAMIC_TASKS": "0"}, "counter": {"BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"}}
_results = {}


def _child(groups, grid, share):
    key = (groups, grid, share)
    if key not in _results:
        env = dict(os.environ, BGSA_MYERS_BAND_GROUPS=str(groups), BGSA_MYERS_PREFIX_SHARE=share, **TILE, **GRIDS[grid])
        want = [] if share == "0" else [int(x) for x in share.split(",")]
        p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), json.dumps(want)], capture_output=True, text=True, timeout=300, env=env)
        assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
        _results[key] = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
    return _results[key]


@pytest.mark.parametrize("grid", ["static", "counter"])
@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("share", ["5,6,7", "2,3"])
def test_sharing_keeps_every_score_and_count(groups, grid, share):
    r = _child(groups, grid, share)
    assert r["nq"] == 300 and r["depths"] == [int(x) for x in share.split(",")]
    # the entries on the device are the sorted order, and a good part of the queries start behind a snapshot
    assert r["entries"] and r["tile"] >= 16 and r["resumed"] >= r["nq"] // 4, (r["tile"], r["resumed"])
    assert r["exact"] and r["window"] and r["windows"] and r["reordered"], {k: v for k, v in r.items() if k != "scores"}
    # the redo wave: exact scores, and exactly the (64-subject group, query) pairs above B redone, every pair banded once
    assert r["redo_exact"] and r["redo_stats"] == r["redo_want"] and r["redo_want"][0] >= 21, (r["redo_stats"], r["redo_want"])
    assert r["redo_sharing_neighbours"] >= 5
    # far pairs: exact scores; the guard stopped the banding, so fewer group-queries were tried than there are
    assert r["far_exact"] and r["far_stats"][0] == r["far_stats"][1] and 64 <= r["far_stats"][1] < 3 * r["nq"], r["far_stats"]
    off = _child(groups, grid, "0")
    assert off["depths"] == [] and off["exact"]
    assert r["scores"] == off["scores"]
    assert r["stats"] == off["stats"] and r["redo_stats"] == off["redo_stats"]

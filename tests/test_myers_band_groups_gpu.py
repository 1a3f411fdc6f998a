"""GPU parity of the certified band with TWO subject groups per wave: myers_global_asm_kernel<NW, 2, *, true>, 3..5 words
(DESIGN.md §4.2).

The launcher picks that kernel for large buckets only, so every run here is a child process with BGSA_MYERS_BAND_GROUPS=2
(the knob is read once), which forces it for any bucket of at least two groups.  The data are the F10 band-edge fixtures
(tests/golden/f10_myers_band_edge_*: whole waves within B with a pair at exactly B, waves with one lane at B + 1), one shape
per width and both signs of n - m where a fixture of that width has them.  Scores must equal the fixture, and the counts of
bgsa_hip_myers_band_stats — which stay in units of (64-subject group, query) whichever kernel ran — must equal (groups with a
lane above B, group-queries) exactly: on the dynamic grid and on the static one, on an odd group count (192 subjects: the
second wave's second group is dead — not stored, not tested, not counted), on four groups, and in a query window.  A forced
one-group run of the same launches gives the same scores and the same counts.  Far pairs: the guard reads the same pair.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# 3 words; 4 words, n - m = +1 and 0; 5 words, n - m = +10 and 0 (no fixture of 3..5 words has n < m)
FIXTURES = ["f10_myers_band_edge_70x70", "f10_myers_band_edge_96x97", "f10_myers_band_edge_128x128",
            "f10_myers_band_edge_140x150", "f10_myers_band_edge_150x150"]
FIRST_GROUP = 1   # the 3- and 4-group buckets start here: in every fixture they hold certified groups and groups with a lane above B

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np
import bgsa_amd as B
L = B.lib()
def stats():
    st = (ctypes.c_ulonglong * 2)(); assert L.bgsa_hip_myers_band_stats(st, 1) == 0
    return [int(st[0]), int(st[1])]
out = {}
for name in json.loads(sys.argv[2]):
    z = np.load(sys.argv[1] + "/tests/golden/" + name + ".npz")
    q, s, want = z["queries"], z["subjects"], z["scores"]
    r = {"groups": int(L.bgsa_hip_myers_band_groups((s.shape[1] + 31) // 32, s.shape[0], q.shape[1], s.shape[1], 0))}
    a = B.DeviceAligner(B.ALGO_MYERS)
    a.set_queries(q)
    lo = 64 * int(sys.argv[3])
    for key, sl in (("all", slice(0, s.shape[0])), ("three", slice(lo, lo + 192)), ("four", slice(lo, lo + 256))):
        a.set_subjects(np.ascontiguousarray(s[sl]))
        stats()
        got = a.score().cpu().numpy()
        a.check_faults()
        r[key] = [bool(np.array_equal(got, want[:, sl])), stats()]
    a.set_subjects(s)
    stats()
    got = a.score(1, 2).cpu().numpy()
    a.check_faults()
    r["window"] = [bool(np.array_equal(got[0], want[1])), stats()]
    out[name] = r
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""

FAR_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np
import bgsa_amd as B, oracle as O
L = B.lib()
q = np.full((2048, 150), ord("A"), dtype=np.uint8); s = O.gen_reads(44, 64 * 6, 150)
got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
assert L.bgsa_hip_stream_faults(1) == 0
ok = bool(np.array_equal(got, O.dp_edit(q[:1], s)[0][None, :].repeat(q.shape[0], 0)))
print("RESULT " + json.dumps({"far": [ok, int(st[0]), int(st[1])], "groups": int(L.bgsa_hip_myers_band_groups(5, 64 * 6, 150, 150, 0))}))
"""


def _child(script, env_extra, *args):
    env = dict(os.environ, **env_extra)
    p = subprocess.run([sys.executable, "-c", script, str(ROOT)] + [str(x) for x in args], capture_output=True, text=True,
                       timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


ENVS = {
    # (small launches take the static grid unless the floor is lowered)
    "dynamic": {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"},
    "static": {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_DYNAMIC_TASKS": "0"},
    "one group": {"BGSA_MYERS_BAND_GROUPS": "1", "BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"},
}
_runs = {}


def _run(env):
    if env not in _runs:
        _runs[env] = _child(CHILD, ENVS[env], json.dumps(FIXTURES), FIRST_GROUP)
    return _runs[env]


def _over(name):
    """over[q, g]: group g holds a lane above B for query q."""
    g = load_golden(name)
    nq, qlen = g["queries"].shape
    ns, slen = g["subjects"].shape
    sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
    import rows_ir as R
    limit = 2 * R.myers_band_half(max(qlen, slen)) + 1
    over = (-g["scores"].astype(np.int64) > limit).reshape(nq, ns // 64, 64).any(axis=2)
    assert nq * (ns // 64) < 64          # too few banded group-queries per launch for the guard to stop banding
    return over


@pytest.mark.parametrize("env", ["dynamic", "static"])
@pytest.mark.parametrize("name", FIXTURES)
def test_two_groups_per_wave_exact_scores_and_counts(env, name):
    r = _run(env)[name]
    over = _over(name)
    assert r["groups"] == 2
    assert over.shape[1] % 2 == 0 and over.any() and not over.all()
    assert r["all"] == [True, [int(over.sum()), over.size]], r


@pytest.mark.parametrize("env", ["dynamic", "static"])
@pytest.mark.parametrize("name", FIXTURES)
def test_odd_group_count_and_four_groups(env, name):
    """192 subjects: waves (g, g + 1) and (g + 2, dead).  The dead group is all zero masks — far above B if it were tested."""
    r = _run(env)[name]
    over = _over(name)
    three, four = over[:, FIRST_GROUP:FIRST_GROUP + 3], over[:, FIRST_GROUP:FIRST_GROUP + 4]
    assert three.any() and not three.all()
    assert r["three"] == [True, [int(three.sum()), three.size]], r
    assert r["four"] == [True, [int(four.sum()), four.size]], r


@pytest.mark.parametrize("env", ["dynamic", "static"])
@pytest.mark.parametrize("name", FIXTURES)
def test_query_window(env, name):
    """score(1, 2): the streams are packed from ref_start, and only query 1's group-queries are counted."""
    r = _run(env)[name]
    over = _over(name)
    assert r["window"] == [True, [int(over[1].sum()), over.shape[1]]], r


def test_forced_one_group_run_is_identical():
    one, two = _run("one group"), _run("dynamic")
    for name in FIXTURES:
        assert one[name]["groups"] == 1 and two[name]["groups"] == 2
        assert {k: v for k, v in one[name].items() if k != "groups"} == {k: v for k, v in two[name].items() if k != "groups"}, name


def test_guard_stops_banding_for_far_pairs():
    """Poly-A queries against 6 groups of random subjects: no group is ever certified.  Static grid, 32 queries per task
    (BGSA_TASK_TARGET=1 keeps the tile at its maximum): 3 waves x 64 tiles = 192 tasks of one wave each.  Every fallback adds
    two group-queries to the launch's pair, so at most 31 fallbacks see it below 64; every other fallback sees >= 64 banded,
    all of them redone, and is its wave's last.  At most (31 + 192) x 2 of the 2048 x 6 group-queries run twice."""
    r = _child(FAR_CHILD, {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_DYNAMIC_TASKS": "0", "BGSA_TASK_TARGET": "1"})
    ok, redone, banded = r["far"]
    assert r["groups"] == 2 and ok
    assert redone == banded and 0 < banded <= (31 + 192) * 2, r

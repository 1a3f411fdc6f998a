"""GPU parity of the certified diagonal band: myers_global_asm_kernel<NW, 1, *, true> for 3..8 words.

The band must not change a score: certified waves keep the banded result, every other wave runs the query again with full
rows.  Covered: every width with the band on and off (BGSA_MYERS_BAND=0, a child process: the knob is read once), a wave
where exactly one lane fails the certificate, all-'N' padding groups, and poly-A queries against random subjects, where
the guard must stop banding.

Those inputs never come near the band's outer diagonals or near B = 2h + 1.  The F10 fixtures do (tests/golden/
f10_myers_band_edge_*, minted from the reference; oracle/band_edge.py): whole waves of band-edge pairs that are all within B
of their query — one of them at exactly B — and waves with a single lane at B + 1.  On them the counts of
bgsa_hip_myers_band_stats are asserted EXACTLY: one redo too many means a certifiable pair came out above B on the band's
edge, one too few means a pair above B was let through.  Static and dynamic grid, query windows, the narrow band and graph
replay run on the same pairs.
"""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B
from conftest import golden_names, load_golden

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

# (query length, subject length): 3, 4, 5, 5, 6, 7, 8, 8 words; equal and unequal lengths, not multiples of 32
SHAPES = [(70, 70), (100, 97), (150, 150), (140, 150), (170, 181), (200, 210), (240, 230), (256, 256)]


def _stats(clear=1):
    out = (ctypes.c_ulonglong * 2)()
    assert B.lib().bgsa_hip_myers_band_stats(out, clear) == 0
    return int(out[0]), int(out[1])


def _inputs(oracle, seed, nq, ns, qlen, slen, n_lane=True):
    q = oracle.gen_reads(seed, nq, qlen)
    s = oracle.gen_reads(seed + 1, ns, slen)
    m = min(qlen, slen)
    k = ns // 4
    s[:k, :m] = oracle.mutate(q[np.arange(k) % nq][:, :m], np.arange(k) % 20, seed)
    if n_lane:
        s[k, : slen // 3] = ord("N")      # a third 'N': usually too far for the certificate
    return q, s


@pytest.mark.parametrize("qlen,slen", SHAPES)
def test_band_scores_equal_the_oracle(oracle, qlen, slen):
    L = B.lib()
    assert L.bgsa_hip_myers_band_half(qlen, slen) > 0
    q, s = _inputs(oracle, 3100 + qlen + slen, 24, 256, qlen, slen)
    _stats()
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    assert np.array_equal(got, oracle.myers64(q, s))
    assert L.bgsa_hip_stream_faults(1) == 0
    redone, banded = _stats()
    # a (query, wave) pair falls back iff one of its lanes is above B — unless the guard has stopped banding by then
    B_ = 2 * L.bgsa_hip_myers_band_half(qlen, slen) + 1
    over = (-oracle.myers64(q, s).astype(np.int64) > B_).reshape(24, 4, 64).any(axis=2)
    assert 0 < banded <= 24 * 4 and redone <= int(over.sum()) and redone <= banded
    if not over.any():
        assert (redone, banded) == (0, 24 * 4)


def test_one_lane_fails_the_certificate(oracle):
    """Lane 17 of group 0 holds a poly-T subject: its distance to every random query is above B, so group 0's wave runs every
    query twice; group 1's wave is certified.  Scores equal the oracle either way."""
    q, s = _inputs(oracle, 3300, 16, 128, 150, 150, n_lane=False)
    s[17] = ord("T")
    _stats()
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    want = oracle.myers64(q, s)
    assert np.array_equal(got, want)
    assert (-want[:, 17] > 97).all() and (-np.delete(want, 17, axis=1) <= 97).all()
    assert _stats() == (16, 32)       # 32 banded queries: too few for the guard to stop banding


def test_all_n_padding_groups(oracle):
    """100 subjects are padded to 128 with all-'N' reads; subjects 64..99 are all 'N' too: that wave is never certified."""
    q, s = _inputs(oracle, 3500, 10, 100, 150, 150, n_lane=False)
    s[64:] = ord("N")
    _stats()
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    assert np.array_equal(got, oracle.myers64(q, s))
    redone, banded = _stats()
    assert banded == 20 and redone == 10


CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np
import bgsa_amd as B, oracle as O
out = {}
L = B.lib()
for qlen, slen in json.loads(sys.argv[2]):
    q = O.gen_reads(41 + qlen, 12, qlen); s = O.gen_reads(42 + slen, 192, slen)
    s[:20, :min(qlen, slen)] = O.mutate(q[np.arange(20) % 12][:, :min(qlen, slen)], np.arange(20) % 9, 43)
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
    out[f"{qlen},{slen}"] = [bool(np.array_equal(got, O.myers64(q, s))), int(st[0]), int(st[1])]
if len(sys.argv) > 3 and int(sys.argv[3]):   # far pairs: poly-A queries against random subjects, enough queries per wave for the guard
    q = np.full((int(sys.argv[3]), 150), ord("A"), dtype=np.uint8); s = O.gen_reads(44, 64 * 16, 150)
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
    out["far"] = [bool(np.array_equal(got, O.dp_edit(q[:1], s)[0][None, :].repeat(q.shape[0], 0))), int(st[0]), int(st[1])]
if len(sys.argv) > 4:   # band-edge ladders at half-width h (oracle/band_edge.py): whole waves within B, one lane at B + 1, waves above B
    from oracle import band_edge as E
    h = int(sys.argv[4]); limit = 2 * h + 1
    for qlen, slen in json.loads(sys.argv[5]):
        q = O.gen_reads(77 + qlen, 1, qlen).copy(); q[q == E.FILLER] = ord("T")
        s, _ = E.band_edge_pairs(q[0], slen, h)
        d = -O.dp_edit(q, s).astype(np.int64)[0]
        inside, above = s[d <= limit], s[d > limit]
        cyc = lambda rows: rows[np.arange(-(-len(rows) // 64) * 64) % len(rows)]
        one = np.insert(cyc(inside)[:63], 32, s[d == limit + 1][0], axis=0)
        s = np.ascontiguousarray(np.concatenate([cyc(inside), one, cyc(above)]))
        want = O.myers64(q, s)
        over = (-want.astype(np.int64) > limit).reshape(-1, 64).any(axis=1)
        got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
        st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
        out[f"edge {qlen},{slen}"] = {"half": int(L.bgsa_hip_myers_band_half(qlen, slen)),
                                      "exact": bool(np.array_equal(got, want) and np.array_equal(want, O.dp_edit(q, s))),
                                      "stats": [int(st[0]), int(st[1])], "want": [int(over.sum()), int(len(over))],
                                      "at_limit": bool((d[d <= limit] == limit).any()), "certified_waves": int((~over).sum())}
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""

NARROW_EDGE_SHAPES = [(150, 150), (100, 97), (240, 256)]


def _child(env_extra, shapes, far=0, edge_half=0, edge_shapes=(), script=None):
    env = dict(os.environ, **env_extra)
    args = [sys.executable, "-c", script or CHILD, str(ROOT), json.dumps(shapes)] + ([str(far)] if far or edge_half else [])
    if edge_half:
        args += [str(edge_half), json.dumps(list(edge_shapes))]
    p = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def test_band_off_and_narrow_band_in_a_child_process():
    off = _child({"BGSA_MYERS_BAND": "0"}, SHAPES)
    assert all(v == [True, 0, 0] for v in off.values()), off
    narrow = _child({"BGSA_MYERS_BAND": "12"}, SHAPES, edge_half=12, edge_shapes=NARROW_EDGE_SHAPES)
    edge = {k: narrow.pop(k) for k in [f"edge {m},{n}" for m, n in NARROW_EDGE_SHAPES]}
    assert all(v[0] for v in narrow.values()), narrow          # random pairs fail a band this narrow: every wave falls back
    assert all(v[1] > 0 and v[1] <= v[2] for k, v in narrow.items() if k != "70,70"), narrow
    # ladders made for h = 12: the waves within B = 25 are certified, every other wave is redone — exactly
    for k, v in edge.items():
        assert v["half"] == 12 and v["exact"] and v["at_limit"] and v["certified_waves"] > 0, (k, v)
        assert v["want"][1] < 64 and v["stats"] == v["want"], (k, v)


def test_guard_stops_banding_for_far_pairs():
    """Poly-A queries: no wave is ever certified.  Once the launch has reported 64 banded queries with more than one in eight
    redone, every wave that falls back runs full rows only from then on, so far fewer than all wave-queries run twice."""
    r = _child({"BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"}, [], far=2048)
    ok, redone, banded = r["far"]
    assert ok
    assert redone == banded and 0 < banded < 2048 * 16 * 3 // 4, r


# ---- band-edge pairs: the F10 fixtures ------------------------------------------------------------------------------------

EDGE = golden_names("f10_myers_band_edge_")


def _edge(name):
    """The fixture, B of its shape, and over[q, w]: wave w holds a lane above B for query q."""
    g = load_golden(name)
    nq, qlen = g["queries"].shape
    ns, slen = g["subjects"].shape
    half = B.lib().bgsa_hip_myers_band_half(qlen, slen)
    assert half > 0 and ns % 64 == 0
    limit = 2 * half + 1
    dist = -g["scores"].astype(np.int64)
    over = (dist > limit).reshape(nq, ns // 64, 64).any(axis=2)
    assert nq * (ns // 64) < 64          # too few banded queries per launch for the guard to stop banding
    return g, limit, dist, over


def _one_lane_waves(dist, over, limit, i):
    """Query i owns the i-th share of the waves (make_golden.py: band_edge_fixture): first the waves in which every lane is
    within B — one lane at exactly B —, then four waves with one lane at B + 1, lanes 0, 31, 32 and 63, and one at B.  Checks
    that and returns [(wave, lane)] of the four."""
    nq, waves = over.shape
    per = waves // nq
    assert per * nq == waves and per > 4
    d = dist[i].reshape(waves, 64)
    certified = d[i * per:(i + 1) * per - 4]
    assert (certified <= limit).all() and (certified == limit).any()
    ones = list(zip(range((i + 1) * per - 4, (i + 1) * per), (0, 31, 32, 63)))
    for w, lane in ones:
        assert d[w, lane] == limit + 1 and (np.delete(d[w], lane) <= limit).all() and (d[w] == limit).any()
    return ones


def test_band_edge_fixtures_are_all_here():
    assert len(EDGE) >= 13
    widths = [(load_golden(n)["subjects"].shape[1] + 31) // 32 for n in EDGE]
    assert all(widths.count(nw) >= 2 for nw in range(3, 9))


@pytest.mark.parametrize("name", EDGE)
def test_band_edge_pairs_exact_scores_and_counts(oracle, name):
    """Equality of the counts in both directions: a redo too many is a pair at D = B that came out above B on the band's edge, a
    redo too few is a pair at D = B + 1 that was let through."""
    g, limit, dist, over = _edge(name)
    q, s = g["queries"], g["subjects"]
    assert np.array_equal(oracle.myers64(q, s), g["scores"])
    for i in range(q.shape[0]):          # the inputs: a fully certified wave with a pair at exactly B; four waves with one lane at B + 1
        _one_lane_waves(dist, over, limit, i)
    _stats()
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    assert np.array_equal(got, g["scores"])
    assert B.lib().bgsa_hip_stream_faults(1) == 0
    assert _stats() == (int(over.sum()), over.size)


@pytest.mark.parametrize("name", EDGE)
def test_one_lane_above_the_limit_at_lanes_0_31_32_63(name):
    """Each such wave alone under its own query alone: the wave is redone — (1, 1) — and every score equals the fixture."""
    g, limit, dist, over = _edge(name)
    a = B.DeviceAligner(B.ALGO_MYERS)
    a.set_queries(g["queries"])
    for i in range(g["queries"].shape[0]):
        for w, lane in _one_lane_waves(dist, over, limit, i):
            a.set_subjects(g["subjects"][64 * w:64 * w + 64])
            _stats()
            out = a.score(i, i + 1)
            a.check_faults()
            assert np.array_equal(out.cpu().numpy()[0], g["scores"][i, 64 * w:64 * w + 64]), (i, w, lane)
            assert _stats() == (1, 1), (i, w, lane)


@pytest.mark.parametrize("name", EDGE)
def test_query_window_counts_only_its_own_waves(name):
    """score(1, 2): the band streams are packed from ref_start — row 1 of the fixture, and only query 1's waves are counted."""
    g, limit, dist, over = _edge(name)
    a = B.DeviceAligner(B.ALGO_MYERS)
    a.set_queries(g["queries"])
    a.set_subjects(g["subjects"])
    _stats()
    out = a.score(1, 2)
    a.check_faults()
    assert np.array_equal(out.cpu().numpy()[0], g["scores"][1])
    assert _stats() == (int(over[1].sum()), over.shape[1])


EDGE_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np
import bgsa_amd as B
out = {}
L = B.lib()
for name in json.loads(sys.argv[2]):
    z = np.load(sys.argv[1] + "/tests/golden/" + name + ".npz")
    got = B.align_all_pairs(z["queries"], z["subjects"], algo=B.ALGO_MYERS, device="cuda:0")
    st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
    out[name] = [bool(np.array_equal(got, z["scores"])), int(st[0]), int(st[1])]
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("env", [{"BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"}, {"BGSA_DYNAMIC_TASKS": "0"}],
                         ids=["dynamic", "static"])
def test_band_edge_pairs_on_both_grids(env):
    """The dynamic-handout instantiation (myers_global_asm_kernel<NW, 1, true, true>; small launches take the static grid unless
    the floor is lowered) and the static one, each in a child process: the knobs are read once.  Same scores, same counts.
    (bgsa_hip_kernel_name does not tell the two instantiations apart.)"""
    r = _child(env, EDGE, script=EDGE_CHILD)
    assert sorted(r) == EDGE
    for name in EDGE:
        g, limit, dist, over = _edge(name)
        assert r[name] == [True, int(over.sum()), over.size], (name, r[name])


def test_band_edge_graph_replay():
    """One captured launch with redone waves, replayed three times: the packer zeroes the launch's guard pair inside the graph,
    so every replay adds the same pair to the counts and writes the same scores."""
    import torch
    g, limit, dist, over = _edge("f10_myers_band_edge_150x150")
    assert over.any() and not over.all()
    a = B.DeviceAligner(B.ALGO_MYERS)
    a.set_queries(g["queries"])
    a.set_subjects(g["subjects"])
    out = torch.zeros(g["scores"].shape, dtype=torch.int16, device="cuda:0")
    a.score(out=out)  # warm-up allocates the workspace outside the capture
    a.check_faults()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            a.score(out=out)
    torch.cuda.synchronize()
    _stats()
    for k in range(1, 4):
        out.zero_()
        graph.replay()
        a.check_faults()
        assert np.array_equal(out.cpu().numpy(), g["scores"])
        assert _stats(clear=0) == (k * int(over.sum()), k * over.size)
    _stats()

"""Rescue of the certified Myers band (myers_band.h), on the CPU: a launch with two subject groups per wave on a
large bucket runs a band three narrower than the default and scores its few uncertified lanes again one by one.

Checked here, without a GPU: the rescue half-width against its restatement, the word-rows it saves at 150 bp, the selection
(bgsa_hip_myers_band_rescue) on both sides of each of its conditions, what the pool adds to the workspace, and — through the
rows_ir interpreter on the band-edge pairs of oracle/band_edge.py — that the narrower band is exact both ways: D <= B' implies
D' = D, and D > B' implies D' > B'.  The second half is what makes "pairs with D > B'" the exact number of lanes a launch
rescues (tests/test_myers_band_rescue_gpu.py).
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B
from oracle import band_edge as E

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import gen_rows_asm as G  # noqa: E402

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v

KNOBS = ("BGSA_MYERS_BAND", "BGSA_MYERS_BAND_GROUPS", "BGSA_MYERS_BAND_RESCUE", "BGSA_MYERS_BAND_RESCUE_POOL")

CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import bgsa_amd as B
L = B.lib()
print("RESULT " + json.dumps([int(L.bgsa_hip_myers_band_rescue(*case)) for case in json.loads(sys.argv[2])]))
"""


def _rescue(cases, **env_extra):
    """bgsa_hip_myers_band_rescue(ref_len, read_len, n_queries, read_count) per case, in a process of its own: the knobs are read once."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), json.dumps(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def test_rescue_half_width_equals_its_restatement():
    L = B.lib()
    for length in range(65, 161):
        assert L.bgsa_hip_myers_band_rescue_half(length) == R.myers_band_rescue_half(length) == R.myers_band_half(length) - 3
    assert R.myers_band_rescue_half(150) == 45


STREAM_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import ctypes, numpy as np
import bgsa_amd as B
L = B.lib()
row = np.zeros(150, dtype=np.uint8)
n = L.bgsa_hip_myers_band_stream(row.ctypes.data, 150, 150, None, 0)
buf = (ctypes.c_ubyte * n)()
assert L.bgsa_hip_myers_band_stream(row.ctypes.data, 150, 150, buf, n) == n
print("RESULT " + json.dumps(list(buf)))
"""


def _library_word_rows(h):
    """Word-rows of a 150 x 150 query as band_schedule (myers_band.h) lays them out at half-width h: the library's band stream
    under BGSA_MYERS_BAND=h, walked as the row loop walks it — every row code on the words of the window its last SETWIN named."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env["BGSA_MYERS_BAND"] = str(h)
    p = subprocess.run([sys.executable, "-c", STREAM_CHILD, str(ROOT)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    stream = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
    windows = [(a, b) for a in range(5) for b in range(a, 5)]          # slot groups in band_window_index's order
    pos, rows, words, width = 0, 0, 0, None
    while stream[pos] != 5:
        c = stream[pos]
        if c == 6:
            pos = (pos | 7) + 1
        elif c == 7:
            a, b = windows[stream[pos + 1]]
            width = b - a + 1
            pos += 2
        else:
            rows, words, pos = rows + 1, words + width, pos + 1
    assert rows == 150
    return words


def test_word_rows_of_the_rescue_band_at_150():
    """band_schedule(150, 150, 45, 5) sums to 474 word-rows of 750, and to 492 at h = 48: from the library's own schedule, and
    from the restatement the interpreter tests below run on."""
    assert _library_word_rows(45) == 474
    assert _library_word_rows(48) == 492
    assert sum(b - a + 1 for a, b in R.myers_band_windows(150, 150, 45, 5)) == 474
    assert sum(b - a + 1 for a, b in R.myers_band_windows(150, 150, 48, 5)) == 492


def test_selection_on_both_sides_of_its_conditions():
    cases = [
        # the bucket's size: two groups per wave by default from 125,000 subjects on
        (150, 150, 2000, 64 * 1953), (150, 150, 2000, 64 * 1954),
        # the queries: the rescue kernel's floor outweighs the gain of a short launch
        (150, 150, 999, 200000), (150, 150, 1000, 200000),
        # the pool: 2e-3 x queries x subjects <= half of 4,096 entries per query — subjects <= 1,024,000 ...
        (150, 150, 10000, 1000000), (150, 150, 10000, 64 * 16000), (150, 150, 10000, 64 * 16001),
        # ... and of the capped pool (2^26 entries from 16,384 queries on): 20,000 queries, subjects <= 838,860
        (150, 150, 20000, 64 * 13107), (150, 150, 20000, 64 * 13108),
        # the lengths: default_half loses less than a quarter (150, 100 bp) or more (66, 80, 72 bp); |n - m| <= 3; 3..5 words
        (100, 100, 2000, 200000), (66, 66, 2000, 200000), (80, 80, 2000, 200000), (72, 72, 2000, 200000),
        (100, 97, 2000, 200000), (100, 96, 2000, 200000), (160, 160, 2000, 200000), (161, 161, 2000, 200000), (64, 64, 2000, 200000),
    ]
    assert 64 * 1953 < 125000 <= 64 * 1954
    got = _rescue(cases)
    assert got == [0, 45,
                   0, 45,
                   45, 45, 0,
                   45, 0,
                   31, 0, 0, 0,
                   31, 0, 48, 0, 0], got


def test_selection_knobs():
    cases = [(150, 150, 100, 200000), (66, 66, 100, 128), (150, 150, 100, 64), (300, 300, 100, 200000)]
    assert _rescue(cases, BGSA_MYERS_BAND_RESCUE="0") == [0, 0, 0, 0]
    # forced on: every banded launch with two groups per wave (a small bucket has them with BGSA_MYERS_BAND_GROUPS=2 only)
    assert _rescue(cases, BGSA_MYERS_BAND_RESCUE="1") == [45, 0, 0, 0]
    assert _rescue(cases, BGSA_MYERS_BAND_RESCUE="1", BGSA_MYERS_BAND_GROUPS="2") == [45, 21, 0, 0]
    assert _rescue(cases, BGSA_MYERS_BAND_RESCUE="1", BGSA_MYERS_BAND_GROUPS="2", BGSA_MYERS_BAND="20") == [20, 20, 0, 0]
    assert _rescue(cases, BGSA_MYERS_BAND_RESCUE="1", BGSA_MYERS_BAND_GROUPS="2", BGSA_MYERS_BAND_RESCUE_POOL="0") == [0, 0, 0, 0]


def test_workspace_grows_by_the_pool_only_where_a_launch_may_rescue():
    L = B.lib()
    ws = L.bgsa_hip_workspace_bytes
    for nq in (1, 100, 10000):
        pool = min(32768 * nq, 512 << 20)
        # (the streams follow ref_len; read_len decides the pool alone)
        assert ws(B.ALGO_MYERS, 150, 65, nq) - ws(B.ALGO_MYERS, 150, 64, nq) == pool
        assert ws(B.ALGO_MYERS, 150, 160, nq) - ws(B.ALGO_MYERS, 150, 161, nq) == pool
        assert ws(B.ALGO_MYERS, 150, 150, nq) == ws(B.ALGO_MYERS, 150, 65, nq)
        for read_len in (64, 150, 161):                                    # uniform over the plain plans
            assert ws(B.ALGO_BITPAL, 150, read_len, nq) == ws(B.ALGO_MYERS, 150, read_len, nq)
        assert ws(B.ALGO_BANDED, 150, 150, nq) == ws(B.ALGO_BANDED, 150, 64, nq)
    assert ws(B.ALGO_MYERS, 150, 150, 16384) - ws(B.ALGO_MYERS, 150, 64, 16384) == 512 << 20
    assert ws(B.ALGO_MYERS, 150, 150, 50000) - ws(B.ALGO_MYERS, 150, 64, 50000) == 512 << 20      # capped


# ---- the rescue band is exact both ways on the band-edge pairs ------------------------------------------------------------

def _band_scores(q, s, h):
    qlen, slen = len(q), s.shape[1]
    nw = (slen + 31) // 32
    stream = R.myers_band_stream(CODE[q], qlen, slen, h, nw)
    assert stream is not None
    st = R.myers_init_state(nw, 1, s.shape[0])
    rows = R.run_band_stream(nw, st, R.build_peq32(s, nw), stream, band=True, schedule=G.ilp)   # the bodies as the generator emits them
    return -R.myers_score(st, nw, qlen, slen).astype(np.int64), rows


@pytest.mark.parametrize("qlen,slen", [(150, 150), (100, 97), (65, 65)])
def test_rescue_band_is_exact_both_ways(oracle, qlen, slen):
    h = R.myers_band_rescue_half(max(qlen, slen))
    limit = 2 * h + 1
    assert (qlen, slen, h) in ((150, 150, 45), (100, 97, 31), (65, 65, 21))
    assert R.myers_band_windows(qlen, slen, h, (slen + 31) // 32) is not None
    seen = set()
    for q in (E.three_run_query(qlen), E.seeded_runs_query(qlen, 1)):
        s, _ = E.band_edge_pairs(q, slen, h)
        want = -oracle.dp_edit(q[None], s).astype(np.int64)[0]
        got, rows = _band_scores(q, s, h)
        assert rows < qlen * ((slen + 31) // 32)
        assert (got >= want).all()
        inside = want <= limit
        assert np.array_equal(got[inside], want[inside])           # D <= B': the optimal path lies inside the band
        assert (got[~inside] > limit).all()                        # D > B': nothing is let through
        seen |= set((want - limit).tolist())
    # the input condition: paths on both sides of the certificate, one exactly at B' and one at B' + 1
    assert set(range(-2, 4)) <= seen, sorted(seen)

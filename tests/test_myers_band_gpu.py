"""GPU parity of the certified diagonal band: myers_global_asm_kernel<NW, 1, *, true> for 3..8 words.

The band must not change a score: certified waves keep the banded result, every other wave runs the query again with full
rows.  Covered: every width with the band on and off (BGSA_MYERS_BAND=0, a child process: the knob is read once), a wave
where exactly one lane fails the certificate, all-'N' padding groups, and poly-A queries against random subjects, where
the guard must stop banding.
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
if len(sys.argv) > 3:   # far pairs: poly-A queries against random subjects, enough queries per wave for the guard
    q = np.full((int(sys.argv[3]), 150), ord("A"), dtype=np.uint8); s = O.gen_reads(44, 64 * 16, 150)
    got = B.align_all_pairs(q, s, algo=B.ALGO_MYERS, device="cuda:0")
    st = (ctypes.c_ulonglong * 2)(); L.bgsa_hip_myers_band_stats(st, 1)
    out["far"] = [bool(np.array_equal(got, O.dp_edit(q[:1], s)[0][None, :].repeat(q.shape[0], 0))), int(st[0]), int(st[1])]
assert L.bgsa_hip_stream_faults(1) == 0
print("RESULT " + json.dumps(out))
"""


def _child(env_extra, shapes, far=0):
    env = dict(os.environ, **env_extra)
    args = [sys.executable, "-c", CHILD, str(ROOT), json.dumps(shapes)] + ([str(far)] if far else [])
    p = subprocess.run(args, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def test_band_off_and_narrow_band_in_a_child_process():
    off = _child({"BGSA_MYERS_BAND": "0"}, SHAPES)
    assert all(v == [True, 0, 0] for v in off.values()), off
    narrow = _child({"BGSA_MYERS_BAND": "12"}, SHAPES)        # random pairs fail a band this narrow: every wave falls back
    assert all(v[0] for v in narrow.values()), narrow
    assert all(v[1] > 0 and v[1] <= v[2] for k, v in narrow.items() if k != "70,70"), narrow


def test_guard_stops_banding_for_far_pairs():
    """Poly-A queries: no wave is ever certified.  Once the launch has reported 64 banded queries with more than one in eight
    redone, every wave that falls back runs full rows only from then on, so far fewer than all wave-queries run twice."""
    r = _child({"BGSA_DYNAMIC_MIN_TASKS": "1", "BGSA_DYNAMIC_TASK_WORDS": "1"}, [], far=2048)
    ok, redone, banded = r["far"]
    assert ok
    assert redone == banded and 0 < banded < 2048 * 16 * 3 // 4, r

"""Two subject groups per wave in the certified band's row loops, on the CPU.

rows_ir.myers_window_body(nw, a, b, groups = 2) is the window body of TWO groups behind one dispatch; for every window of
3, 4 and 5 words, as the generator schedules it, it must compute what the one-group body computes on each group's state and
masks, in twice the instructions.  run_band_stream(groups = 2) walks a band stream with those bodies: on band-edge pairs
(oracle/band_edge.py) it equals two one-group runs.  The launcher's choice between the two kernels is a host-side rule
(bgsa_hip_myers_band_groups): one group below the threshold, for 6..8 words, mixed lengths and with the band off.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from oracle import band_edge as E

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import gen_rows_asm as G  # noqa: E402

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v

WINDOWS = [(nw, a, b) for nw in (3, 4, 5) for a in range(nw) for b in range(a, nw)]
LANES = 96


def _two_group_schedule(body):
    """The pass gen_band_function(nw, 2) applies to its bodies."""
    return R.schedule_ilp(body, G.MYERS_ILP[0], G.MYERS_BAND_PAIR_WINDOW, *G.MYERS_ILP[2:3])


def _random_state(rng, words):
    """(VP, VN) per word with VP & VN = 0, and a match mask per word."""
    st, eq = [], []
    for _ in range(words):
        vp = rng.integers(0, 2 ** 32, LANES, dtype=np.uint64).astype(np.uint32)
        vn = rng.integers(0, 2 ** 32, LANES, dtype=np.uint64).astype(np.uint32) & ~vp
        st += [vp, vn]
        eq.append(rng.integers(0, 2 ** 32, LANES, dtype=np.uint64).astype(np.uint32))
    return st, eq


@pytest.mark.parametrize("nw,a,b", WINDOWS)
def test_two_group_body_equals_the_one_group_body_on_each_group(nw, a, b):
    rng = np.random.default_rng(1000 * nw + 10 * a + b)
    one = G.ilp(R.myers_window_body(nw, a, b))
    two = _two_group_schedule(R.myers_window_body(nw, a, b, groups=2))
    assert two.valu_count() == 2 * one.valu_count()
    for _ in range(4):
        st, eq = _random_state(rng, 2 * nw)
        want = []
        for g in range(2):
            s1 = [x.copy() for x in st[2 * g * nw:2 * (g + 1) * nw]]
            one.simulate(s1, eq[g * nw:(g + 1) * nw])
            want += s1
        got = [x.copy() for x in st]
        two.simulate(got, eq)
        for i, (x, y) in enumerate(zip(got, want)):
            assert np.array_equal(x, y), (nw, a, b, i)
        for w in list(range(a)) + list(range(b + 1, nw)):       # words outside the window keep their state, in both groups
            for g in range(2):
                i = 2 * (g * nw + w)
                assert np.array_equal(got[i], st[i]) and np.array_equal(got[i + 1], st[i + 1])


@pytest.mark.parametrize("nw", [3, 4, 5])
def test_two_group_bodies_fit_the_one_group_temporaries_plus_one(nw):
    """The register ledger of myers_global_asm_kernel<NW, 2, *, true> counts on it: at most one temporary more than one group."""
    _, n_one = G.ilp(R.myers_body(nw, 1)).allocate_temps()
    for a in range(nw):
        for b in range(a, nw):
            _, n_two = _two_group_schedule(R.myers_window_body(nw, a, b, groups=2)).allocate_temps()
            assert n_two <= n_one + 1, (nw, a, b, n_two, n_one)


@pytest.mark.parametrize("qlen,slen", [(65, 65), (100, 97), (150, 150)])
def test_band_stream_with_two_groups_equals_two_one_group_runs(oracle, qlen, slen):
    nw = (slen + 31) // 32
    h = R.myers_band_half(max(qlen, slen))
    q = oracle.gen_reads(500 + qlen, 1, qlen)[0].copy()
    q[q == E.FILLER] = ord("T")
    s, _ = E.band_edge_pairs(q, slen, h)
    n = len(s) // 2
    assert n >= 8
    groups = [np.ascontiguousarray(s[:n]), np.ascontiguousarray(s[n:2 * n])]
    stream = R.myers_band_stream(CODE[q], qlen, slen, h, nw)
    assert stream is not None
    for band in (True, False):
        want, rows_one = [], None
        for sg in groups:
            st = R.myers_init_state(nw, 1, n)
            rows_one = R.run_band_stream(nw, st, R.build_peq32(sg, nw), stream, band=band, schedule=G.ilp)
            want += st
        st2 = R.myers_init_state(nw, 2, n)
        peq2 = np.concatenate([R.build_peq32(sg, nw) for sg in groups], axis=1)
        rows_two = R.run_band_stream(nw, st2, peq2, stream, band=band, schedule=_two_group_schedule, groups=2)
        assert rows_two == rows_one
        assert len(st2) == len(want) and all(np.array_equal(x, y) for x, y in zip(st2, want))
        if not band:      # full rows: the DP's distances, per group
            for g, sg in enumerate(groups):
                assert np.array_equal(R.myers_score(st2, nw, qlen, slen, group=g).astype(np.int64), oracle.dp_edit(q[None, :], sg)[0].astype(np.int64))


# ---- the launcher's choice (host only) ---------------------------------------------------------------------------------------

SELECT_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
import bgsa_amd as B
L = B.lib()
print("RESULT " + json.dumps([int(L.bgsa_hip_myers_band_groups(*case)) for case in json.loads(sys.argv[2])]))
"""


def _select(cases, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("BGSA_MYERS_BAND_GROUPS", "BGSA_MYERS_BAND")}
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", SELECT_CHILD, str(ROOT), json.dumps(cases)], capture_output=True, text=True,
                       timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


THRESHOLD = 125000   # myers_global.hip: kBandPairMinReads — the smallest bucket measured, two groups ahead at every size from there up


def test_two_groups_from_the_threshold_up_and_only_where_the_band_applies():
    # (word_num, read_count, ref_len, read_len, mixed_lengths)
    cases = [(5, THRESHOLD - 1, 150, 150, 0), (5, THRESHOLD, 150, 150, 0), (5, 1000000, 150, 150, 0),
             (3, THRESHOLD - 1, 70, 70, 0), (3, THRESHOLD, 70, 70, 0), (4, THRESHOLD, 100, 97, 0), (5, THRESHOLD, 140, 150, 0),
             (5, 128, 150, 150, 0),                                                            # the bucket bgsa_hip_kernel_name names
             (6, 1000000, 170, 181, 0), (7, 1000000, 200, 210, 0), (8, 1000000, 256, 256, 0),  # 6..8 words: no two-group loop
             (2, 1000000, 64, 64, 0), (10, 1000000, 300, 300, 0),                              # no band at these widths
             (5, 1000000, 150, 150, 1),                                                        # mixed lengths run full rows
             (5, 1000000, 40, 150, 0)]                                                         # |n - m| > B: band off
    want = [1, 2, 2, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1]
    assert _select(cases) == want
    assert _select(cases, BGSA_MYERS_BAND="0") == [1] * len(cases)
    # the knob forces either kernel for every banded bucket of at least two groups — and nothing else
    forced = [2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1]
    assert _select(cases + [(5, 127, 150, 150, 0)], BGSA_MYERS_BAND_GROUPS="2") == forced + [1]
    assert _select(cases, BGSA_MYERS_BAND_GROUPS="1") == [1] * len(cases)


def test_kernel_name_is_the_small_bucket_answer():
    import bgsa_amd as B
    assert B.lib().bgsa_hip_kernel_name(B.ALGO_MYERS, 5).decode() == "myers_global_asm_kernel<5, 1>"

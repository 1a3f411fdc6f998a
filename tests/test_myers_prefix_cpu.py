"""Prefix sharing of the certified band's kernels, on the CPU.

A wave walks its tile of queries in sorted order and keeps the state after a few fixed depths of the current query's
prefix; a query that begins like its predecessor resumes behind the deepest depth they share.  Here the interpreter of the
generated bodies (rows_ir.run_band_stream) walks a sorted family of queries the way myers_global_asm_kernel<NW, G, *, true>
does — segment by segment, fixed-depth slots of words 0..1 per group, a full-row redo from row 0 in the middle of a run of
sharing queries — and each query alone over its unsegmented band stream: the states must be equal, and the scores the DP's.
The segmented stream the packer writes (bgsa_hip_myers_band_segments) must be the restatement's (rows_ir.myers_band_segments).
"""
import ctypes
import os
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402

from prefix_family import CODE, KEY_CHARS, family, sorted_order  # noqa: E402

SHAPES = [(150, 150), (97, 97), (65, 70)]
LANES = 12
TILE = 32           # the family is two tiles: position 32 shares nothing whatever its prefix


def test_the_family_holds_the_cases_it_is_there_for():
    q = family(150)
    assert 55 <= len(q) <= 64
    order, lcp = sorted_order(q, (5, 6, 7, 8, 9, 10), len(q))
    assert set(range(0, 11)) <= set(lcp)                                    # every shared length 0..10 between sorted neighbours
    assert any(a > b > 0 for a, b in zip(lcp, lcp[1:]))                     # a predecessor that shared deeper than its successor
    full = [int(np.argmin(np.append(q[i] == q[j], False))) for i, j in zip(order, order[1:])]
    assert 16 in full and any(16 < n < 150 for n in full) and 150 in full   # exactly 16, beyond the first window, duplicates


@pytest.mark.parametrize("qlen,slen", SHAPES)
@pytest.mark.parametrize("depths", [(5, 6, 7), (2, 3)], ids=["5,6,7", "2,3"])
def test_packed_segments_equal_the_restatement(qlen, slen, depths):
    L = B.lib()
    nw, h = (slen + 31) // 32, R.myers_band_half(max(qlen, slen))
    assert L.bgsa_hip_myers_band_half(qlen, slen) == h
    d = (ctypes.c_int * len(depths))(*depths)
    for row in family(qlen)[:6]:
        mapped = CODE[row]
        want, offsets = R.myers_band_segments(mapped, qlen, slen, h, nw, depths)
        buf = (ctypes.c_ubyte * (len(want) + 8))()
        off = (ctypes.c_int * (len(depths) + 2))()
        n = L.bgsa_hip_myers_band_segments(mapped.ctypes.data_as(ctypes.c_void_p), qlen, slen, d, len(depths), buf, len(buf), off)
        assert n == len(want) and bytes(buf[:n]) == want and list(off) == offsets
        assert all(o % 8 == 0 for o in offsets) and all(want[o] == 7 for o in offsets[:-1])
        assert n <= len(R.myers_band_stream(mapped, qlen, slen, h, nw)) + 16 * len(depths)   # myers_band.h: band_segments_stride_bound
    # a depth whose rows leave words 0..1, a depth that is no row, depths out of order: no segments
    for bad in ((5, 40), (0, 3), (6, 5), (3, 3)):
        d = (ctypes.c_int * 2)(*bad)
        assert L.bgsa_hip_myers_band_segments(CODE[family(qlen)[0]].ctypes.data_as(ctypes.c_void_p), qlen, slen, d, 2, None, 0, None) == 0


def _words01(state, nw, groups):
    return [state[2 * g * nw + i].copy() for g in range(groups) for i in range(4)]


@pytest.mark.parametrize("groups", [1, 2])
@pytest.mark.parametrize("qlen,slen,depths", [(150, 150, (5, 6, 7)), (97, 97, (5, 6, 7)), (65, 70, (5, 6, 7)), (150, 150, (2, 3))],
                         ids=["150x150", "97x97", "65x70", "150x150 depths 2,3"])
def test_sharing_walk_equals_every_query_alone(oracle, qlen, slen, depths, groups):
    nw, h = (slen + 31) // 32, R.myers_band_half(max(qlen, slen))
    limit = 2 * h + 1
    q = family(qlen)
    subjects = [oracle.gen_reads(900 + qlen + g, LANES, slen) for g in range(groups)]
    for g, s in enumerate(subjects):      # half of the lanes near a query: certified with room to spare
        s[:LANES // 2, :min(qlen, slen)] = oracle.mutate(q[np.arange(LANES // 2) + 6 * g][:, :min(qlen, slen)], np.arange(LANES // 2), 5)
    peq = np.concatenate([R.build_peq32(np.ascontiguousarray(s), nw) for s in subjects], axis=1)
    want_scores = [oracle.dp_edit(q, np.ascontiguousarray(s)).astype(np.int64) for s in subjects]
    order, lcp = sorted_order(q, depths, TILE)
    n = len(depths)
    redo_at = next(k for k in range(TILE + 2, len(order) - 1) if lcp[k] >= depths[0] and lcp[k + 1] >= depths[0])   # inside a run of sharing queries
    slots = [None] * n
    resumed = 0
    for k, i in enumerate(order):
        codes = CODE[q[i]]
        stream, off = R.myers_band_segments(codes, qlen, slen, h, nw, depths)
        alone = R.myers_init_state(nw, groups, LANES)
        R.run_band_stream(nw, alone, peq, R.myers_band_stream(codes, qlen, slen, h, nw), groups=groups)
        # the kernel's walk
        seg = sum(1 for d in depths if d <= lcp[k])
        st = R.myers_init_state(nw, groups, LANES)
        if seg:
            resumed += 1
            for g in range(groups):
                for j in range(4):
                    st[2 * g * nw + j] = slots[seg - 1][4 * g + j].copy()
        for j in range(seg, n + 1):
            R.run_band_stream(nw, st, peq, stream[off[j]:], groups=groups)
            if j < n:
                slots[j] = _words01(st, nw, groups)
        assert all(np.array_equal(a, b) for a, b in zip(st, alone)), (k, i, lcp[k])
        for g in range(groups):
            got = -R.myers_score(st, nw, qlen, slen, group=g).astype(np.int64)
            want = -want_scores[g][i]
            assert (got >= want).all() and np.array_equal(got[want <= limit], want[want <= limit]), (k, i, g)
        if k == redo_at:      # the certificate's fallback: full rows from row 0, nothing restored, nothing stored
            full = R.myers_init_state(nw, groups, LANES)
            for j in range(n + 1):
                R.run_band_stream(nw, full, peq, stream[off[j]:], band=False, groups=groups)
            for g in range(groups):
                assert np.array_equal(R.myers_score(full, nw, qlen, slen, group=g).astype(np.int64), want_scores[g][i])
    assert resumed >= len(order) // 3 and lcp[TILE] == 0


def test_prefix_depths_of_a_launch_shape():
    """Host only: the depths follow the query count, off below the threshold and wherever the band is off; the call answers, it never launches."""
    L = B.lib()
    d = (ctypes.c_int * 8)()
    if not os.environ.get("BGSA_MYERS_PREFIX_SHARE"):                                     # the default rule: d0 = floor(log4 nq), from 2,000 queries
        assert L.bgsa_hip_myers_prefix_depths(5, 1 << 20, 150, 150, 10000, 0, d, 8) == 3 and list(d[:3]) == [5, 6, 7]
        assert L.bgsa_hip_myers_prefix_depths(5, 1 << 20, 150, 150, 2000, 0, d, 8) == 3 and list(d[:3]) == [4, 5, 6]
        assert L.bgsa_hip_myers_prefix_depths(3, 1 << 20, 65, 70, 5000, 0, d, 8) == 3 and list(d[:3]) == [5, 6, 7]
        assert L.bgsa_hip_myers_prefix_depths(5, 1 << 20, 150, 150, 1999, 0, d, 8) == 0
        assert L.bgsa_hip_myers_prefix_depths(5, 640, 150, 150, 10000, 0, d, 8) == 0      # the order is n^2: not with 15 queries per subject
    assert L.bgsa_hip_myers_prefix_depths(5, 1 << 20, 150, 150, 4, 0, d, 8) == 0          # a handful of queries: no tile to share in
    assert L.bgsa_hip_myers_prefix_depths(5, 1 << 20, 150, 150, 10000, 1, d, 8) == 0      # mixed lengths: no band
    assert L.bgsa_hip_myers_prefix_depths(32, 1 << 20, 1000, 1000, 10000, 0, d, 8) == 0   # no band at 32 words
    assert L.bgsa_hip_myers_prefix_depths(0, 1 << 20, 150, 150, 10000, 0, d, 8) < 0

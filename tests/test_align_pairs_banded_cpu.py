"""Band-limited pair alignment without a GPU: the window rule of tests/banded_align_reference.py against the canonical
traceback, bgsa_hip_align_pairs_band_words against the rule, the workspace sizes, and the C ABI's argument checks (they come
before any HIP call)."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import align_reference as A  # noqa: E402
import banded_align_reference as R  # noqa: E402
import bgsa_amd as B  # noqa: E402
from oracle import band_edge as E  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MAX_WORDS = 32   # kBandTraceMaxWords


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- 1. the rule against the canonical traceback ------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 33), (33, 32), (64, 65), (96, 97), (150, 150), (150, 140), (140, 150), (40, 150), (150, 40), (300, 290),
          (1100, 1056)]
BOUNDS = [0, 1, 3, 31, 32, 33, 64, 97]


@functools.lru_cache(maxsize=None)
def _shape_pairs(m, n):
    """(queries, subjects, canonical) of one shape: mutated random pairs, every cell a tie, all mismatch."""
    import oracle as O
    seed = 104729 * m + n
    longest = max(m, n)
    count = 4 if longest >= 1000 else 12
    base = O.gen_reads(seed, count, longest)
    edits = np.array([0, 1, 2, 3, 5, 8, 13, 16, 24, 32, 40, 48][:count]) % (longest + 1)
    mutants = O.mutate(base, edits, seed + 1)
    q = np.concatenate([base[:, :m], np.full((2, m), ord("A"), np.uint8)])
    s = np.concatenate([mutants[:, :n], np.full((1, n), ord("A"), np.uint8), np.full((1, n), ord("C"), np.uint8)])
    return q, s, A.canonical(q, s)


def _check_rule(q, s, want, bound, what):
    for p, (got, (d, runs)) in enumerate(zip(R.align_rows(q, s, bound), want)):     # raises BandFault if a traceback leaves its windows
        dist, got_runs, width = got
        assert width == R.band_words(q.shape[1], s.shape[1], bound)
        if d <= bound:
            assert (dist, got_runs) == (d, runs), f"pair {p} of {what} at B = {bound}: D = {d}"
        else:
            assert dist is None and got_runs == [], f"pair {p} of {what} at B = {bound}: D = {d} came out as {dist}"


@pytest.mark.parametrize("m,n", SHAPES)
def test_rule_equals_the_canonical_script_within_the_bound_and_reports_beyond_above_it(m, n):
    q, s, want = _shape_pairs(m, n)
    for bound in BOUNDS:
        _check_rule(q, s, want, bound, f"{m} x {n}")
    assert any(d <= BOUNDS[-1] for d, _ in want) or abs(n - m) > BOUNDS[-1]


@pytest.mark.parametrize("m,n,h", [(150, 150, 8), (150, 140, 10), (140, 150, 10), (200, 203, 16)])
def test_rule_on_the_band_edge_ladders(m, n, h):
    q = E.seeded_runs_query(m, 31 * m + n)
    s, tags = E.band_edge_pairs(q, n, h)
    qq = np.repeat(q[None, :], len(s), axis=0)
    want = A.canonical(qq, s)
    bound = 2 * h + 1
    dists = {d for d, _ in want}
    assert bound in dists and bound + 1 in dists, "the ladders hold no pair at B or at B + 1"
    for b in (bound - 1, bound, bound + 1):
        _check_rule(qq, s, want, b, f"ladder {m} x {n}")


# ---- 2. band_words ------------------------------------------------------------------------------------------------------
def test_band_words_equal_the_rule(L):
    lens = [1, 31, 32, 33, 64, 150, 1000, 1024, 1025, 4000, 10000]
    for m in lens:
        for n in lens:
            for bound in (0, 1, 31, 32, 33, 100, 500, 900):
                got = L.bgsa_hip_align_pairs_band_words(m, n, bound)
                assert got == R.band_words(m, n, bound), (m, n, bound)
                assert got <= (n + 31) // 32
                assert (got == 0) == (abs(n - m) > bound)
    f = L.bgsa_hip_align_pairs_band_words
    assert f(0, 150, 10) == 0 and f(150, 0, 10) == 0 and f(-1, 150, 10) == 0 and f(150, 150, -1) == 0
    assert f(150, 150, 0) == 1 and f(150, 150, 20) == 3 and f(10000, 10000, 500) == 17 and f(4000, 4000, 128) == 5


# ---- 3. sizes -----------------------------------------------------------------------------------------------------------
def _slice(m, n, bound):
    raw = m * 2 * R.band_words(m, n, bound) * 256 + 2 * ((n + 31) // 32) * 256 + (m + n) * 64
    return (raw + 255) // 256 * 256


def test_workspace_sizes(L):
    f, fmin = L.bgsa_hip_align_pairs_banded_workspace_bytes, L.bgsa_hip_align_pairs_banded_min_workspace_bytes
    cap = 1 << 30
    assert fmin(0, 150, 10) == 0 and fmin(150, -1, 10) == 0 and fmin(150, 150, -1) == 0
    assert f(0, 150, 10, 5) == 0 and f(150, 150, -1, 5) == 0 and f(150, 150, 10, -1) == 0
    shapes = [(1, 1), (33, 32), (150, 150), (150, 140), (1000, 1024), (1100, 1056), (4000, 4000), (10000, 10000)]
    bounds = [0, 1, 31, 32, 33, 100, 500, 900]
    pairs = [0, 1, 64, 65, 200, 10_000, 1_000_000, 1 << 40]
    for m, n in shapes:
        mins = [fmin(m, n, b) for b in bounds]
        assert mins == [_slice(m, n, b) for b in bounds], (m, n)
        assert all(x > 0 and x % 256 == 0 for x in mins)
        live = [x for b, x in zip(bounds, mins) if b >= abs(n - m)]
        assert live == sorted(live), (m, n)                                   # monotone in B once the shape has a band
        for b, per in zip(bounds, mins):
            row = [f(m, n, b, k) for k in pairs]
            assert row == sorted(row) and row[0] == row[1] == row[2] == per      # up to 64 pairs: one wave
            assert all(per <= x <= max(cap, per) for x in row)
            assert row[-1] == max(cap, per)                                      # 2^40 pairs: the cap; one wave always fits
            assert row[3] == min(2 * per, cap) or per > cap
    assert fmin(150, 150, 20) == 64 * (150 * 8 * 3 + 8 * 5 + 300)
    assert f(150, 150, 20, 130) == 3 * fmin(150, 150, 20)
    # short subjects: no larger than the unbanded call's slice plus the state
    assert fmin(150, 150, 300) == L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150) + 2 * 5 * 256
    # 10,000 bp at B = 500: a tenth of the full history
    full = 10000 * 2 * ((10000 + 31) // 32) * 256
    assert fmin(10000, 10000, 500) < full // 10
    assert fmin(10000, 10000, 500) == 10000 * 2 * 17 * 256 + 2 * 313 * 256 + 20000 * 64      # 88 MB


# ---- 4. refusals, before any HIP call -----------------------------------------------------------------------------------
def _call(L, content=P, peq=P, ref_len=150, read_len=150, read_count=640, word_num=5, pq=P, ps=P, n_pairs=100, n_queries=10,
          base=0, bound=20, dist=P, n_ops=P, cigar=P, cap=300, ws=None, ws_bytes=0):
    return L.bgsa_hip_myers_align_pairs_banded_dev(content, peq, ref_len, read_len, read_count, word_num, pq, ps, n_pairs, n_queries,
                                                   base, bound, dist, n_ops, cigar, cap, ws, ws_bytes, None)


def test_argument_checks_come_before_any_hip_call(L):
    for name in ("content", "peq", "pq", "ps", "dist", "n_ops", "cigar"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert b"NULL" in L.bgsa_hip_last_error() and b"myers_align_pairs_banded_dev" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=-1) == EINVAL
    assert _call(L, ref_len=0) == EINVAL and _call(L, read_len=-1, word_num=0) == EINVAL
    assert _call(L, n_queries=0) == EINVAL and _call(L, cap=0) == EINVAL
    for rc in (0, -64, 1, 63, 65, 100):
        assert _call(L, read_count=rc) == EINVAL, rc
    assert b"multiple of 64" in L.bgsa_hip_last_error()
    for wn in (0, 4, 6, 32):
        assert _call(L, word_num=wn) == EINVAL, wn
    assert b"word_num" in L.bgsa_hip_last_error()
    assert _call(L, bound=-1) == EINVAL and b"max_distance is negative" in L.bgsa_hip_last_error()
    need = L.bgsa_hip_align_pairs_banded_min_workspace_bytes(150, 150, 20)
    assert _call(L, ws=P, ws_bytes=need - 1) == EINVAL and _call(L, ws=P, ws_bytes=0) == EINVAL
    assert b"bgsa_hip_align_pairs_banded_min_workspace_bytes" in L.bgsa_hip_last_error()
    # the order: a NULL pointer, n_pairs, the counts, word_num, max_distance, the window width, the workspace
    assert _call(L, peq=None, n_pairs=-1, word_num=4, bound=-1) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=-1, read_count=63) == EINVAL and b"n_pairs" in L.bgsa_hip_last_error()
    assert _call(L, read_count=63, word_num=4) == EINVAL and b"multiple of 64" in L.bgsa_hip_last_error()
    assert _call(L, word_num=4, bound=-1) == EINVAL and b"word_num" in L.bgsa_hip_last_error()
    assert _call(L, bound=-1, ws=P, ws_bytes=1) == EINVAL and b"max_distance" in L.bgsa_hip_last_error()
    # the errors also win over an empty list
    assert _call(L, n_pairs=0, peq=None) == EINVAL and _call(L, n_pairs=0, word_num=4) == EINVAL and _call(L, n_pairs=0, bound=-1) == EINVAL


def test_a_window_wider_than_the_kernels_is_unsupported_and_names_the_largest_bound(L):
    wn = L.bgsa_hip_word_num(B.ALGO_MYERS, 4000, 4000, 0)
    assert wn == 125
    widths = [L.bgsa_hip_align_pairs_band_words(4000, 4000, b) for b in range(0, 2001)]
    assert widths == sorted(widths)
    largest = max(b for b, w in enumerate(widths) if w <= MAX_WORDS)
    assert widths[largest + 1] == MAX_WORDS + 1
    kw = dict(ref_len=4000, read_len=4000, word_num=wn, cap=8000)
    assert _call(L, bound=largest, n_pairs=0, **kw) == 0
    assert _call(L, bound=largest + 1, **kw) == EUNSUPPORTED
    text = L.bgsa_hip_last_error().decode()
    assert f"max_distance <= {largest}" in text and "33 words" in text, text
    assert _call(L, bound=largest + 1, ws=P, ws_bytes=1, **kw) == EUNSUPPORTED      # ... before the workspace is looked at
    assert _call(L, bound=8000, n_pairs=0, **kw) == EUNSUPPORTED
    # a short subject's window is at most the whole subject: every bound passes
    assert _call(L, ref_len=1000, read_len=1024, word_num=32, bound=2024, n_pairs=0, cap=1) == 0


def test_lengths_whose_sum_passes_int_are_unsupported(L):
    kw = dict(ref_len=2_147_483_600, read_len=150, word_num=5, bound=2_147_483_600, cap=10)
    assert _call(L, **kw) == EUNSUPPORTED and b"2^31" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=0, ws=P, ws_bytes=1, **kw) == EUNSUPPORTED                    # before the workspace, also for an empty list
    assert _call(L, **dict(kw, bound=-1)) == EINVAL and _call(L, **dict(kw, word_num=4)) == EINVAL     # the earlier checks still come first
    assert L.bgsa_hip_align_pairs_band_words(2_147_483_600, 150, 2_147_483_600) == 0
    assert _call(L, ref_len=2_147_483_497, read_len=150, word_num=5, bound=0, cap=10, n_pairs=0) == 0   # the sum is 2^31 - 1: |delta| > B, no window


def test_an_empty_pair_list_and_long_subjects_pass_the_checks(L):
    assert _call(L, n_pairs=0) == 0
    need = L.bgsa_hip_align_pairs_banded_min_workspace_bytes(150, 150, 20)
    assert _call(L, n_pairs=0, ws=P, ws_bytes=need) == 0            # every pointer is fake: nothing may look at them
    assert _call(L, n_pairs=0, bound=0) == 0
    assert _call(L, n_pairs=0, read_len=140, bound=3) == 0           # |delta| > B: every pair is beyond the bound, still no error
    for length, bound in ((4000, 80), (4000, 200), (10000, 200), (10000, 500)):
        wn = L.bgsa_hip_word_num(B.ALGO_MYERS, length, length, 0)
        assert wn > 32
        assert _call(L, ref_len=length, read_len=length, word_num=wn, bound=bound, n_pairs=0, cap=2 * length) == 0
    # the existing call keeps its refusal
    assert L.bgsa_hip_myers_align_pairs_dev(P, P, 4000, 4000, 640, 125, P, P, 0, 10, 0, P, P, P, 8000, None, 0, None) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()


# ---- 5. symbols ---------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_wired(L):
    import ctypes
    names = B.declared_symbols()
    calls = ("bgsa_hip_align_pairs_band_words", "bgsa_hip_align_pairs_banded_min_workspace_bytes",
             "bgsa_hip_align_pairs_banded_workspace_bytes", "bgsa_hip_myers_align_pairs_banded_dev")
    for fn in calls:
        assert fn in names and hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert L.bgsa_hip_align_pairs_banded_workspace_bytes.restype is ctypes.c_size_t
    assert L.bgsa_hip_align_pairs_banded_min_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.bgsa_hip_myers_align_pairs_banded_dev.argtypes) == 19
    header = B.INCLUDE.read_text()
    assert "#define BGSA_HIP_DISTANCE_BEYOND (-2)" in header and "#define BGSA_HIP_FAULT_BAND 8" in header
    for method in ("align_pairs_banded", "align_hits_banded"):
        assert callable(getattr(B.DeviceAligner, method))
    assert callable(B.align_top_alignments_banded)

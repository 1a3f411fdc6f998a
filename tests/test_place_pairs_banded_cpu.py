"""Band-limited semi-global placement without a GPU: the rule of tests/place_reference.py against the canonical semi-global
traceback, bgsa_hip_place_pairs_band_words against the rule, the workspace sizes, and the C ABI's argument checks (they come
before any HIP call)."""
import functools
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import place_reference as R  # noqa: E402
import trace_reference as T  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
MAX_WORDS = 32


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- 1. the rule against the canonical traceback ------------------------------------------------------------------------
KINDS = ("mid", "start", "prefix", "suffix", "end", "unrelated")
SHAPES = [(20, 1), (20, 7), (33, 32), (40, 33), (64, 31), (64, 64), (97, 65), (100, 90), (130, 100), (150, 150), (160, 128),
          (200, 96), (200, 129), (230, 150), (259, 40), (259, 140)]
PER_SHAPE = 66   # 16 shapes x 66 = 1,056 pairs


def _edit(rng, seq, edits, letters):
    seq = list(seq)
    for _ in range(edits):
        kind, at = rng.integers(3), int(rng.integers(len(seq) + 1))
        if kind == 0 and at < len(seq):
            seq[at] = letters[rng.integers(len(letters))]
        elif kind == 1:
            seq.insert(at, letters[rng.integers(len(letters))])
        elif at < len(seq) and len(seq) > 1:
            del seq[at]
    return seq


def make_pairs(m, n, count, seed):
    """(queries[count, m], subjects[count, n]): reads planted mid-window, hanging off the window's start, as its prefix, as
    its suffix, hanging off its end, and unrelated; every third pair from a two-letter alphabet so that end rows tie."""
    rng = np.random.default_rng(seed)
    q = np.empty((count, m), np.uint8)
    s = np.empty((count, n), np.uint8)
    for p in range(count):
        letters = np.frombuffer(b"AC" if p % 3 == 2 else b"ACGT", np.uint8)
        q[p] = letters[rng.integers(len(letters), size=m)]
        kind = KINDS[p % len(KINDS)]
        hang = int(rng.integers(1, max(2, min(n, 10))))
        noise = list(letters[rng.integers(len(letters), size=n)])
        span = min(n, m)
        if kind == "mid":
            at = int(rng.integers(0, m - span + 1))
            src = list(q[p, at: at + span])
        elif kind == "start":
            src = noise[:hang] + list(q[p, : span])
        elif kind == "prefix":
            src = list(q[p, : span])
        elif kind == "suffix":
            src = list(q[p, m - span:])
        elif kind == "end":
            src = list(q[p, m - span + min(hang, span - 1):]) + noise[:hang]
        else:
            src = noise
        if kind != "unrelated":
            src = _edit(rng, src, int(rng.integers(0, 9)), letters)
        s[p] = (noise + src)[-n:] if kind == "suffix" else (src + noise)[:n]   # an edited read is cut or filled up to n
    return q, s


@functools.lru_cache(maxsize=None)
def shape_case(m, n):
    q, s = make_pairs(m, n, PER_SHAPE, 7919 * m + n)
    return q, s, T.canonical(q, s, T.FREE_QUERY, T.UNIT)


def check_rule(q, s, want, bounds_of, tally):
    qc, sc = A.classes(q), A.classes(s)
    for p, (score, span, runs) in enumerate(want):
        d, (q_begin, e, _, _) = -score, span
        for bound in bounds_of(d):
            if bound < 0:
                continue
            dist, end, begin, got_runs, width = R.place(qc[p], sc[p], bound)     # raises BandFault
            assert (dist, end) == (d, e), f"pair {p} at B = {bound}"
            assert width == R.band_words(sc.shape[1], bound)
            if d <= min(bound, sc.shape[1]):
                assert (begin, got_runs) == (q_begin, runs), f"pair {p} at B = {bound}: D* = {d}"
                tally["within"] += 1
            else:
                assert begin is None and got_runs == [], f"pair {p} at B = {bound}: D* = {d}"
        tally["pairs"] += 1
        tally["hang"] += bool(runs) and runs[0][1] == A.OP_D
        tally["last_row"] += e == q.shape[1]
        tally["row_zero"] += q_begin == 0


def test_rule_equals_the_canonical_placement_within_the_bound_and_the_distance_beyond_it():
    tally = dict(pairs=0, within=0, hang=0, last_row=0, row_zero=0)
    for m, n in SHAPES:
        q, s, want = shape_case(m, n)
        check_rule(q, s, want, lambda d: (d - 1, d, d + 1, d + 7, 40), tally)
    # conditions on the inputs, not measurements
    assert tally["pairs"] >= 1000 and tally["within"] >= 3000, tally
    assert tally["hang"] >= 100 and tally["last_row"] >= 100 and tally["row_zero"] >= 100, tally


def test_end_rows_tie_on_the_two_letter_pairs_and_the_smallest_wins():
    ties = 0
    for m, n in SHAPES[4:10]:
        q, s, want = shape_case(m, n)
        h = T.h_matrices(q, s, T.FREE_QUERY, T.UNIT)
        for p, (score, span, _) in enumerate(want):
            rows = np.flatnonzero(h[p, :, n] == score)
            assert rows[0] == span[1]
            ties += rows.size > 1
    assert ties >= 50, ties


def test_rule_on_reads_of_34_words():
    rng = np.random.default_rng(1057)
    m, n = 1300, 1057
    letters = np.frombuffer(b"ACGT", np.uint8)
    q = letters[rng.integers(4, size=(3, m))]
    s = np.empty((3, n), np.uint8)
    s[0] = (_edit(rng, list(q[0, 100: 100 + n]), 12, letters) + list(q[0, :40]))[:n]               # mid-window
    s[1] = (list(letters[rng.integers(4, size=9)]) + _edit(rng, list(q[1, :n]), 6, letters))[:n]   # hangs off the start
    s[2] = (list(q[2, :40]) + _edit(rng, list(q[2, m - n:]), 9, letters))[-n:]                     # ends at the last row
    want = T.canonical(q, s, T.FREE_QUERY, T.UNIT)
    assert want[1][2][0][1] == A.OP_D and want[2][1][1] == m
    tally = dict(pairs=0, within=0, hang=0, last_row=0, row_zero=0)
    check_rule(q, s, want, lambda d: (d - 1, d, d + 1, d + 7, 40, 480), tally)
    assert tally["within"] >= 12


# ---- 2. band_words ------------------------------------------------------------------------------------------------------
def test_band_words_equal_the_rule(L):
    f = L.bgsa_hip_place_pairs_band_words
    for n in (1, 31, 32, 33, 150, 1024, 1057, 4000):
        for bound in (0, 1, 16, 17, 33, 480, 481, 496, 497, 10 ** 6):
            got = f(n, bound)
            assert got == R.band_words(n, bound), (n, bound)
            assert 1 <= got <= (n + 31) // 32
    assert f(0, 10) == 0 and f(-5, 10) == 0 and f(150, -1) == 0
    # a window of w >= 2 words first appears at B = 16 (w - 2) + 1
    for w in range(2, 34):
        assert f(4000, 16 * (w - 2) + 1) == w and f(4000, 16 * (w - 2)) == max(1, w - 1), w
    assert f(150, 12) == 2 and f(150, 150) == 5 and f(1024, 10 ** 6) == 32 and f(1057, 496) == 32 and f(1057, 497) == 33


# ---- 3. sizes -----------------------------------------------------------------------------------------------------------
def test_workspace_sizes(L):
    f, fmin = L.bgsa_hip_place_pairs_banded_workspace_bytes, L.bgsa_hip_place_pairs_banded_min_workspace_bytes
    cap = 1 << 30
    assert fmin(0, 150, 10) == 0 and fmin(400, -1, 10) == 0 and fmin(400, 150, -1) == 0
    assert f(0, 150, 10, 5) == 0 and f(400, 150, -1, 5) == 0 and f(400, 150, 10, -1) == 0
    pairs = [0, 1, 64, 65, 200, 10_000, 1_000_000, 1 << 40]
    for m, n in [(20, 1), (400, 150), (1300, 1000), (2100, 1024), (1300, 1057), (5000, 4000), (12000, 10000)]:
        mins = [fmin(m, n, b) for b in (0, 1, 12, 64, 200, 496)]
        assert all(x > 0 and x % 256 == 0 for x in mins) and mins == sorted(mins), (m, n)
        for b, per in zip((0, 1, 12, 64, 200, 496), mins):
            # the history alone: (n + B) virtual rows of two vectors over the widest window
            assert per >= (n + min(b, n)) * 2 * R.band_words(n, b) * 256
            row = [f(m, n, b, k) for k in pairs]
            assert row == sorted(row) and row[0] == row[1] == row[2] == per      # up to 64 pairs: one wave
            assert all(per <= x <= max(cap, per) for x in row)
            assert row[-1] == max(cap, per)                                      # 2^40 pairs: the cap; one wave always fits
            assert row[3] == min(2 * per, cap) or per > cap
    # 10,000 bp at B = 200: 14 words of 313 have history
    assert fmin(12000, 10000, 200) < 10200 * 2 * 15 * 256


# ---- 4. refusals, before any HIP call -----------------------------------------------------------------------------------
def _call(L, content=P, peq=P, ref_len=400, read_len=150, read_count=640, word_num=5, pq=P, ps=P, n_pairs=100, n_queries=10,
          base=0, bound=12, dist=P, span=P, n_ops=P, cigar=P, cap=550, ws=None, ws_bytes=0):
    return L.bgsa_hip_myers_place_pairs_banded_dev(content, peq, ref_len, read_len, read_count, word_num, pq, ps, n_pairs, n_queries,
                                                   base, bound, dist, span, n_ops, cigar, cap, ws, ws_bytes, None)


def test_argument_checks_come_before_any_hip_call(L):
    for name in ("content", "peq", "pq", "ps", "dist", "span", "n_ops", "cigar"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert b"NULL" in L.bgsa_hip_last_error() and b"myers_place_pairs_banded_dev" in L.bgsa_hip_last_error()
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
    need = L.bgsa_hip_place_pairs_banded_min_workspace_bytes(400, 150, 12)
    assert _call(L, ws=P, ws_bytes=need - 1) == EINVAL and _call(L, ws=P, ws_bytes=0) == EINVAL
    assert b"bgsa_hip_place_pairs_banded_min_workspace_bytes" in L.bgsa_hip_last_error()
    # the order: a NULL pointer, n_pairs, the counts, word_num, max_distance, the lengths' sum, the window width, the workspace
    assert _call(L, peq=None, n_pairs=-1, word_num=4, bound=-1) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=-1, read_count=63) == EINVAL and b"n_pairs" in L.bgsa_hip_last_error()
    assert _call(L, read_count=63, word_num=4) == EINVAL and b"multiple of 64" in L.bgsa_hip_last_error()
    assert _call(L, word_num=4, bound=-1) == EINVAL and b"word_num" in L.bgsa_hip_last_error()
    assert _call(L, bound=-1, ws=P, ws_bytes=1) == EINVAL and b"max_distance" in L.bgsa_hip_last_error()
    # the errors also win over an empty list
    assert _call(L, n_pairs=0, peq=None) == EINVAL and _call(L, n_pairs=0, word_num=4) == EINVAL and _call(L, n_pairs=0, bound=-1) == EINVAL


def test_a_window_wider_than_the_kernels_is_unsupported_and_names_the_largest_bound(L):
    wn = L.bgsa_hip_word_num(B.ALGO_MYERS, 1300, 1057, 0)
    assert wn == 34
    kw = dict(ref_len=1300, read_len=1057, word_num=wn, cap=2400)
    assert _call(L, bound=496, n_pairs=0, **kw) == 0
    assert _call(L, bound=497, **kw) == EUNSUPPORTED
    text = L.bgsa_hip_last_error().decode()
    assert "max_distance <= 496" in text and "33 words" in text, text
    assert _call(L, bound=497, ws=P, ws_bytes=1, **kw) == EUNSUPPORTED      # ... before the workspace is looked at
    assert _call(L, bound=10 ** 6, n_pairs=0, **kw) == EUNSUPPORTED
    assert _call(L, ref_len=12000, read_len=10000, word_num=L.bgsa_hip_word_num(B.ALGO_MYERS, 12000, 10000, 0), bound=497, cap=1) == EUNSUPPORTED
    assert "max_distance <= 496" in L.bgsa_hip_last_error().decode()
    # a read of up to 1,024 bp takes any bound: its window is at most the whole read
    assert _call(L, ref_len=2100, read_len=1024, word_num=32, bound=2 ** 31 - 1, n_pairs=0, cap=1) == 0
    assert _call(L, ref_len=2100, read_len=1024, word_num=32, bound=1024, n_pairs=0, cap=1) == 0


def test_lengths_whose_sum_passes_int_are_unsupported(L):
    # ref_len + read_len + B, B = min(max_distance, read_len): what the op bytes of one lane count
    kw = dict(ref_len=2_147_483_000, read_len=400, word_num=13, cap=10)
    assert _call(L, bound=300, **kw) == EUNSUPPORTED and b"2^31" in L.bgsa_hip_last_error()
    assert _call(L, bound=300, n_pairs=0, ws=P, ws_bytes=1, **kw) == EUNSUPPORTED      # before the workspace, also for an empty list
    assert _call(L, bound=-1, **kw) == EINVAL and _call(L, bound=300, **dict(kw, word_num=4)) == EINVAL   # the earlier checks still come first
    assert _call(L, ref_len=2_147_483_647 - 400 - 300, read_len=400, word_num=13, cap=10, bound=300, n_pairs=0) == 0


def test_an_empty_pair_list_and_long_reads_pass_the_checks(L):
    assert _call(L, n_pairs=0) == 0
    need = L.bgsa_hip_place_pairs_banded_min_workspace_bytes(400, 150, 12)
    assert _call(L, n_pairs=0, ws=P, ws_bytes=need) == 0            # every pointer is fake: nothing may look at them
    assert _call(L, n_pairs=0, bound=0) == 0
    assert _call(L, n_pairs=0, ref_len=100, word_num=5) == 0          # a query shorter than the read is a shape like any other
    for m, n, bound in ((5000, 4000, 80), (5000, 4000, 200), (12000, 10000, 200), (12000, 10000, 496)):
        wn = L.bgsa_hip_word_num(B.ALGO_MYERS, m, n, 0)
        assert wn > 32
        assert _call(L, ref_len=m, read_len=n, word_num=wn, bound=bound, n_pairs=0, cap=m + n) == 0


# ---- 5. symbols ---------------------------------------------------------------------------------------------------------
CALLS = ("bgsa_hip_place_pairs_band_words", "bgsa_hip_place_pairs_banded_min_workspace_bytes",
         "bgsa_hip_place_pairs_banded_workspace_bytes", "bgsa_hip_myers_place_pairs_banded_dev")


def test_symbols_are_declared_and_wired(L):
    import ctypes
    names = B.declared_symbols()
    for fn in CALLS:
        assert fn in names and hasattr(L, fn), fn
        assert getattr(L, fn).argtypes is not None, fn
    assert L.bgsa_hip_place_pairs_banded_workspace_bytes.restype is ctypes.c_size_t
    assert L.bgsa_hip_place_pairs_banded_min_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.bgsa_hip_myers_place_pairs_banded_dev.argtypes) == 20
    for method in ("place_pairs_banded", "place_hits_banded"):
        assert callable(getattr(B.DeviceAligner, method))
    assert callable(B.place_top_queries_banded)


def test_both_library_flavours_export_the_symbols(L):
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        assert path.exists(), path
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], check=True, capture_output=True, text=True).stdout
        exported = {line.split()[-1] for line in out.splitlines() if line.strip()}
        for fn in CALLS:
            assert fn in exported, (path.name, fn)

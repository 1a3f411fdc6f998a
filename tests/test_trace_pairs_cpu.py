"""Traced pairs without a GPU: the reference of tests/trace_reference.py against the oracle's DPs in every mode, the tie-break
contract as literal cases, and the C ABI's refusals (they come before any HIP call) and `n_pairs == 0`."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import trace_reference as T  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SCORE_SETS = [(2, -3, -5), (1, -1, -2), (10, -9, -15), (0, -1, -1)]


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- the reference itself -------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def random_pairs(oracle):
    rng = np.random.default_rng(0x7ACE)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for t in range(300):
        m, n = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        q = acgt[rng.integers(0, 4, m)]
        if t % 3 == 0:                                  # unrelated reads of unequal lengths
            s = acgt[rng.integers(0, 4, n)]
        elif t % 3 == 1:                                # a mutated copy, cut or extended to n
            s = oracle.mutate(q[None, :], [int(rng.integers(0, 12))], 3000 + t)[0]
            s = np.concatenate([s, acgt[rng.integers(0, 4, max(0, n - s.size))]])[:n]
        else:                                           # a mutated window of the longer one inside the other
            k = min(m, n)
            lo = int(rng.integers(0, max(m, n) - k + 1))
            if m >= n:
                s = oracle.mutate(q[None, lo: lo + k], [int(rng.integers(0, 6))], 3000 + t)[0]
            else:
                s = acgt[rng.integers(0, 4, n)]
                s[lo: lo + k] = oracle.mutate(q[None, :], [int(rng.integers(0, 6))], 3000 + t)[0]
        pairs.append((q, s))
    assert sum(q.size != s.size for q, s in pairs) > 100
    return pairs


def _oracle_score(oracle, mode, scores, q, s):
    if mode == T.GLOBAL:
        return int(oracle.dp_nw(q[None, :], s[None, :], *scores)[0, 0])
    if mode == T.FREE_SUBJECT:
        return int(oracle.dp_semiglobal(q[None, :], s[None, :], *scores)[0, 0])
    assert tuple(scores) == T.UNIT
    return int(oracle.dp_edit_semiglobal(q[None, :], s[None, :])[0, 0])


@pytest.mark.parametrize("mode,scores", [(T.GLOBAL, x) for x in SCORE_SETS] + [(T.FREE_SUBJECT, x) for x in SCORE_SETS] +
                         [(T.FREE_QUERY, T.UNIT)])
def test_reference_scores_are_the_oracles_and_its_scripts_are_valid(oracle, random_pairs, mode, scores):
    for q, s in random_pairs:
        (score, span, runs), = T.canonical(q[None, :], s[None, :], mode, scores)
        assert score == _oracle_score(oracle, mode, scores, q, s), (mode, scores, q.tobytes(), s.tobytes())
        T.validate(q, s, mode, scores, score, span, runs)
        if mode == T.GLOBAL and tuple(scores) == T.UNIT:
            (distance, want), = A.canonical(q[None, :], s[None, :])
            assert (score, span, runs) == (-distance, (0, q.size, 0, s.size), want)


@pytest.mark.parametrize("scores", [(2, -3, -5), (1, -1, -2), (10, -9, -15)])
def test_reference_free_query_mode_is_valid_with_every_score_set(random_pairs, scores):
    # the oracle knows this mode at unit cost only; with other sets the score is checked through the script's worth and
    # against the definition: the best of the last column, no later row reaching it first
    for q, s in random_pairs[::5]:
        h = T.h_matrices(q[None, :], s[None, :], T.FREE_QUERY, scores)[0]
        (score, span, runs), = T.canonical(q[None, :], s[None, :], T.FREE_QUERY, scores)
        T.validate(q, s, T.FREE_QUERY, scores, score, span, runs)
        assert score == h[:, -1].max() and (h[: span[1], -1] < score).all()


def _script(q, s, mode, scores=(2, -3, -5)):
    (score, span, runs), = T.canonical(np.frombuffer(q, np.uint8)[None, :], np.frombuffer(s, np.uint8)[None, :], mode, scores)
    T.validate(np.frombuffer(q, np.uint8), np.frombuffer(s, np.uint8), mode, scores, score, span, runs)
    return score, span, A.to_string(runs)


def test_tie_breaks_are_the_contracts():
    G, FQ, FS = T.GLOBAL, T.FREE_QUERY, T.FREE_SUBJECT
    # all-'A' pairs of unequal length.  Global: walking back the diagonal comes first, so the gap lands at the front.
    assert _script(b"AAAA", b"AA", G) == (2 * 2 - 2 * 5, (0, 4, 0, 2), "2I2=")
    assert _script(b"AA", b"AAAA", G) == (2 * 2 - 2 * 5, (0, 2, 0, 4), "2D2=")
    assert _script(b"AAAA", b"AA", G, T.UNIT) == (-2, (0, 4, 0, 2), "2I2=")
    # free query overhangs: every row from 2 on ends a full match of the subject; the smallest end row wins
    assert _script(b"AAAA", b"AA", FQ, T.UNIT) == (0, (0, 2, 0, 2), "2=")
    assert _script(b"AAAAAAA", b"AAA", FQ, T.UNIT) == (0, (0, 3, 0, 3), "3=")
    # ... and a subject longer than the query cannot avoid its gaps: they land at the front of the aligned span
    assert _script(b"AA", b"AAAA", FQ, T.UNIT) == (-2, (0, 2, 0, 4), "2D2=")
    # free subject overhangs: the smallest end column wins, the query is consumed whole
    assert _script(b"AA", b"AAAA", FS) == (4, (0, 2, 0, 2), "2=")
    assert _script(b"AAA", b"AAAAAAA", FS, (1, -1, -2)) == (3, (0, 3, 0, 3), "3=")
    assert _script(b"AAAA", b"AA", FS) == (2 * 2 - 2 * 5, (0, 4, 0, 2), "2I2=")
    # a mismatch diagonal is preferred to I + D of the same cost (unit cost); at 2/-3/-5 it is simply cheaper
    assert _script(b"AC", b"CA", G, T.UNIT) == (-2, (0, 2, 0, 2), "2X")
    assert _script(b"AC", b"CA", G) == (-6, (0, 2, 0, 2), "2X")
    # a subject that occurs twice in the query: the first end wins
    assert _script(b"TTACGTTTACGTT", b"ACGT", FQ, T.UNIT) == (0, (2, 6, 0, 4), "4=")
    assert _script(b"ACGT", b"TTACGTTTACGTT", FS) == (8, (0, 4, 2, 6), "4=")
    # an empty span: nothing of the free sequence is worth aligning
    assert _script(b"CCCC", b"A", FQ, T.UNIT) == (-1, (0, 0, 0, 1), "1D")          # i* = 0: H[0][n] is already the best
    assert _script(b"AA", b"CCCC", FS, (1, -3, -1)) == (-2, (0, 2, 0, 0), "2I")    # j* = 0: a mismatch costs more than a gap
    assert _script(b"A", b"CCCC", FS) == (-3, (0, 1, 0, 1), "1X")                  # ... at 2/-3/-5 it does not: the first column
    assert _script(b"ANNA", b"ANxA", G, T.UNIT) == (-1, (0, 4, 0, 4), "2=1X1=")    # 'N' its own class, a foreign byte class 0


def test_ac_ca_in_the_free_modes_spelled_out():
    # AC / CA, subject inside the query at unit cost: the last column holds (-2, -1, -1) — 'C' deleted then A = A ends at
    # row 1, and row 2 reaches the same -1 — the smallest row wins
    score, span, text = _script(b"AC", b"CA", T.FREE_QUERY, T.UNIT)
    assert (score, span, text) == (-1, (0, 1, 0, 2), "1D1=")
    # query inside the subject at 2/-3/-5: the last row holds (-10, -3, -3): 'A' inserted (-5) then C = C (+2) ends at
    # column 1, and column 2 reaches the same -3 — the smallest column wins
    score, span, text = _script(b"AC", b"CA", T.FREE_SUBJECT)
    assert (score, span, text) == (-3, (0, 2, 0, 1), "1I1=")


# ---- the C ABI, before any HIP call ---------------------------------------------------------------------------------
def _params(algo=B.ALGO_BITPAL, alignment=0, match=2, mismatch=-3, gap=-5, k=0):
    return B.Params(algo, alignment, match, mismatch, gap, k)


def _call(L, params="default", content=P, peq=P, ref_len=150, read_len=150, read_count=640, word_num=5, pq=P, ps=P, n_pairs=100,
          n_queries=10, base=0, score=P, span=P, n_ops=P, cigar=P, cap=300, ws=None, ws_bytes=0):
    p = _params() if params == "default" else params
    return L.bgsa_hip_trace_pairs_dev(ctypes.byref(p) if p is not None else None, content, peq, ref_len, read_len, read_count,
                                      word_num, pq, ps, n_pairs, n_queries, base, score, span, n_ops, cigar, cap, ws, ws_bytes, None)


MYERS = dict(algo=B.ALGO_MYERS, match=0, mismatch=-1, gap=-1)


def test_symbol_is_declared_and_exported(L):
    assert "bgsa_hip_trace_pairs_dev" in B.declared_symbols() and hasattr(L, "bgsa_hip_trace_pairs_dev")
    if B.LIB_AB_PATH.exists():
        assert hasattr(ctypes.CDLL(str(B.LIB_AB_PATH)), "bgsa_hip_trace_pairs_dev")


def test_argument_checks_come_before_any_hip_call(L):
    for name in ("params", "content", "peq", "pq", "ps", "score", "span", "n_ops", "cigar"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert b"NULL" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=-1) == EINVAL
    assert _call(L, ref_len=0) == EINVAL and _call(L, ref_len=-7) == EINVAL
    assert _call(L, read_len=0, word_num=0) == EINVAL and _call(L, read_len=-1, word_num=0) == EINVAL
    assert _call(L, n_queries=0) == EINVAL and _call(L, n_queries=-2) == EINVAL
    assert _call(L, cap=0) == EINVAL and _call(L, cap=-1) == EINVAL
    for rc in (0, -64, 1, 63, 65, 100):
        assert _call(L, read_count=rc) == EINVAL, rc
    assert b"multiple of 64" in L.bgsa_hip_last_error()
    for wn in (0, 4, 6, 32):
        assert _call(L, word_num=wn) == EINVAL, wn
        assert _call(L, _params(**MYERS), word_num=wn) == EINVAL, wn
    assert b"bgsa_hip_word_num" in L.bgsa_hip_last_error()
    assert _call(L, read_len=128, word_num=5) == EINVAL and _call(L, read_len=161, word_num=5) == EINVAL
    need = L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150)
    assert _call(L, ws=P, ws_bytes=need - 1) == EINVAL and _call(L, ws=P, ws_bytes=0) == EINVAL
    assert b"workspace" in L.bgsa_hip_last_error()
    for alignment in (0, 1):
        assert _call(L, _params(alignment=alignment, gap=0)) == EINVAL and _call(L, _params(alignment=alignment, gap=3)) == EINVAL
        assert _call(L, _params(alignment=alignment, match=-3)) == EINVAL and _call(L, _params(alignment=alignment, match=-4)) == EINVAL
    assert b"gap < 0" in L.bgsa_hip_last_error()
    assert _call(L, _params(algo=7)) == EINVAL and _call(L, _params(alignment=2)) == EINVAL
    # the errors also win over an empty list
    assert _call(L, n_pairs=0, peq=None) == EINVAL and _call(L, n_pairs=0, word_num=4) == EINVAL and _call(L, _params(gap=0), n_pairs=0) == EINVAL


def test_banded_and_plus_distance_are_unsupported(L):
    for n_pairs in (100, 0):
        assert _call(L, _params(algo=B.ALGO_BANDED, match=0, mismatch=-1, gap=-1, k=8), word_num=8, n_pairs=n_pairs) == EUNSUPPORTED
        assert b"banded" in L.bgsa_hip_last_error()
        for alignment in (0, 1):
            assert _call(L, _params(algo=B.ALGO_MYERS, alignment=alignment, match=0, mismatch=1, gap=1), n_pairs=n_pairs) == EUNSUPPORTED
            assert b"-distance" in L.bgsa_hip_last_error() and b"(0, -1, -1)" in L.bgsa_hip_last_error()
    assert _call(L, _params(algo=B.ALGO_BITPAL, match=0, mismatch=1, gap=1)) == EINVAL      # no +distance for BitPAl: plain bad scores


def test_subjects_beyond_1024_bp_are_unsupported(L):
    for read_len in (1025, 1056, 4000):
        wn = L.bgsa_hip_word_num(B.ALGO_BITPAL, 150, read_len, 0)
        assert wn > 32 and _call(L, _params(match=1, mismatch=-1, gap=-1), read_len=read_len, word_num=wn) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()
    assert _call(L, read_len=1025, word_num=32) == EINVAL          # a word_num that is not the layout's comes first
    assert _call(L, _params(**MYERS), ref_len=1024, read_len=1024, word_num=32, n_pairs=0) == 0


def test_the_sixteen_bit_bound_is_refused_and_quoted(L):
    # max(|match|, |mismatch|, |gap|) * (ref_len + read_len) <= 32767: the DP row is kept in 16 bits
    wide = dict(ref_len=1024, read_len=1024, word_num=32)
    assert _call(L, _params(match=10, mismatch=-9, gap=-15), n_pairs=0, **wide) == 0            # 15 * 2,048 = 30,720
    assert _call(L, _params(match=15, mismatch=-9, gap=-15), ref_len=1160, read_len=1024, word_num=32, n_pairs=0) == 0   # 32,760
    for params in (_params(match=10, mismatch=-9, gap=-16), _params(match=16, mismatch=-9, gap=-15), _params(match=1, mismatch=-16, gap=-1),
                   _params(match=10, mismatch=-9, gap=-16, alignment=1)):
        for n_pairs in (100, 0):
            assert _call(L, params, n_pairs=n_pairs, **wide) == EUNSUPPORTED                    # 16 * 2,048 = 32,768
            assert b"32767" in L.bgsa_hip_last_error() and b"32768" in L.bgsa_hip_last_error() and b"16 bits" in L.bgsa_hip_last_error()
    assert _call(L, _params(match=300, mismatch=-200, gap=-250), ref_len=100, read_len=10, word_num=1) == EUNSUPPORTED   # 33,000
    assert _call(L, _params(match=300, mismatch=-200, gap=-250), ref_len=99, read_len=10, word_num=1, n_pairs=0) == 0    # 32,700
    # Myers scores 0 / -1 / -1 whatever the ints hold (as the scoring calls), so its bound is ref_len + read_len
    assert _call(L, _params(algo=B.ALGO_MYERS, match=10, mismatch=-9, gap=-16), n_pairs=0, **wide) == 0
    assert _call(L, _params(**MYERS), ref_len=32000, read_len=1024, word_num=32) == EUNSUPPORTED


def test_an_empty_pair_list_is_ok_and_launches_nothing(L):
    need = L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150)
    for params in (_params(), _params(alignment=1), _params(**MYERS), _params(alignment=1, **MYERS), _params(match=7, mismatch=-2, gap=-3)):
        assert _call(L, params, n_pairs=0) == 0
        assert _call(L, params, n_pairs=0, ws=P, ws_bytes=need) == 0        # every pointer is fake: nothing may look at them

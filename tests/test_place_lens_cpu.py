"""Read placement on buckets of mixed read lengths (Myers semi-global with every lane's own n), the parts that need no GPU: the
two new C symbols, every answer bgsa_hip_myers_place_score_lens_dev / bgsa_hip_myers_place_trace_pairs_lens_dev give before
anything is allocated or launched — reached through ctypes with pointers nothing may look at —, and the premise of the kernel
restated with the project's own row IR: right-align every lane by its OWN length (rows_ir.semi_align per lane), run the
unchanged myers_semi_body, and the score is the semi-global DP of the unpadded read whatever lies behind its end."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import trace_reference as T  # noqa: E402

P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
EINVAL, EUNSUPPORTED = -1, -2
NEW_SYMBOLS = ("bgsa_hip_myers_place_score_lens_dev", "bgsa_hip_myers_place_trace_pairs_lens_dev")


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


def test_new_symbols_are_declared_and_exported(L):
    names = B.declared_symbols()
    for fn in NEW_SYMBOLS:
        assert fn in names, f"{fn} is not declared in include/bgsa_hip.h"
        assert hasattr(L, fn), f"{fn} is not exported"
    if B.LIB_AB_PATH.exists():
        ab = ctypes.CDLL(str(B.LIB_AB_PATH))
        for fn in NEW_SYMBOLS:
            assert hasattr(ab, fn), f"{fn} is not exported by the A/B flavour"


def _score(L, ref_len, read_len, wn=None, lens=P, read_count=128, window=(0, 4), work=1 << 40):
    wn = B.word_num(B.ALGO_MYERS, ref_len, read_len, 0) if wn is None else wn
    return L.bgsa_hip_myers_place_score_lens_dev(P, P, P, lens, ref_len, read_len, read_count, window[0], window[1], wn, P, work, None)


def _trace(L, ref_len, read_len, wn=None, lens=P, n_pairs=10):
    wn = B.word_num(B.ALGO_MYERS, ref_len, read_len, 0) if wn is None else wn
    return L.bgsa_hip_myers_place_trace_pairs_lens_dev(P, P, lens, ref_len, read_len, 128, wn, P, P, n_pairs, 4, 0, P, P, P, P, 300, P,
                                                       1 << 40, None)


def test_score_refuses_33_words_and_names_the_limit(L):
    assert B.word_num(B.ALGO_MYERS, 200, 1056, 0) == 33
    assert _score(L, 200, 1056) == EUNSUPPORTED
    err = L.bgsa_hip_last_error()
    assert b"word_num > 32" in err and b"1,024 bp" in err, err
    assert _trace(L, 200, 1056) == EUNSUPPORTED and b"word_num > 32" in L.bgsa_hip_last_error()


def test_null_lengths_are_einval(L):
    assert _score(L, 200, 150, lens=None) == EINVAL
    assert _trace(L, 200, 150, lens=None) == EINVAL and b"d_read_lens" in L.bgsa_hip_last_error()


def test_argument_checks_are_those_of_the_plain_call(L):
    assert _score(L, 200, 150, wn=4) == EINVAL                       # a word_num that is not the layout's
    assert _score(L, 200, 150, wn=6) == EINVAL
    assert _score(L, 200, 150, read_count=100) == EINVAL             # not a multiple of 64
    assert _score(L, 200, 150, window=(3, 2)) == EINVAL
    assert _score(L, 200, 150, work=16) == EINVAL and b"workspace" in L.bgsa_hip_last_error()
    assert _trace(L, 200, 150, wn=4) == EINVAL


def test_nothing_to_do_is_ok_and_touches_nothing(L):
    assert _score(L, 200, 150, window=(3, 3), work=0) == 0           # an empty query window
    assert _score(L, 200, 150, read_count=0) == 0                    # an empty bucket
    assert _trace(L, 200, 150, n_pairs=0) == 0                       # no pairs


def test_the_existing_lens_calls_keep_refusing_semi_global(L):
    p = B.Params(B.ALGO_MYERS, 1, 0, -1, -1, 0)
    assert L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), P, P, P, P, 200, 150, 128, 0, 4, 5, P, 1 << 40, None) == EUNSUPPORTED
    assert L.bgsa_hip_trace_pairs_lens_dev(ctypes.byref(p), P, P, P, 200, 150, 128, 5, P, P, 10, 4, 0, P, P, P, P, 300, P, 1 << 40,
                                           None) == EUNSUPPORTED


# ---- the premise, with rows_ir ----------------------------------------------------------------------------------------------
def edge_lengths(slen):
    """Both edges of every word, the ends, and 2: 1, 2, 31, 32, 33, ..., slen - 1, slen."""
    out = {1, 2, slen - 1, slen}
    for w in range(1, (slen + 31) // 32 + 1):
        out |= {32 * w - 1, 32 * w, 32 * w + 1}
    return sorted(n for n in out if 1 <= n <= slen)


def semi_dp(query, read):
    """max over i of H[i][n]: the numpy DP of tests/trace_reference.py in the Myers semi-global mode, on the unpadded read."""
    h = T.h_matrices(query[None, :], read[None, :], T.FREE_QUERY, T.UNIT)[0]
    return int(h[:, -1].max())


@pytest.mark.parametrize("slen,nw", [(150, 5), (150, 6), (288, 10)])
def test_per_lane_alignment_scores_the_unpadded_read(slen, nw):
    rng = np.random.default_rng(slen * 100 + nw)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    qlen = slen + 50
    query = acgt[rng.integers(4, size=qlen)]
    lens = edge_lengths(slen)
    assert {1, 2, 31, 32, 33, slen - 1, slen} <= set(lens)
    # rows are the query's own text from a lane-dependent offset with a few substitutions, `slen` bytes each: what lies behind
    # a read's end is the source's continuation — the worst a pad can hold, an alignment would gladly go on into it
    rows = np.empty((len(lens), slen), np.uint8)
    for lane in range(len(lens)):
        at = int(rng.integers(0, qlen - slen + 1))
        rows[lane] = query[at: at + slen]
        if lane % 4 == 3:
            rows[lane] = acgt[rng.integers(4, size=slen)]
        else:
            hit = rng.integers(0, slen, size=lane % 5)
            rows[lane, hit] = acgt[rng.integers(4, size=hit.size)]
    peq = R.build_peq32(rows, (slen + 31) // 32)          # planes of the PADDED rows, as the bucket's preprocess builds them
    aligned = np.zeros((5, nw, len(lens)), np.uint32)
    state = [np.zeros(len(lens), np.uint32) for _ in range(2 * nw + 2)]
    for lane, n in enumerate(lens):                        # the kernel's per-lane set-up
        planes, vp0 = R.semi_align(peq[:, :, lane: lane + 1], n, nw)
        aligned[:, :, lane] = planes[:, :, 0]
        for w in range(nw):
            state[2 * w][lane] = vp0[w]
        state[2 * nw][lane] = state[2 * nw + 1][lane] = n
    body = R.myers_semi_body(nw)
    code = {ord("A"): 0, ord("C"): 1, ord("G"): 2, ord("T"): 3}
    for ch in query:                                       # the row loop: nothing in it knows a length
        body.simulate(state, [aligned[code[int(ch)], w] for w in range(nw)])
    got = -state[2 * nw + 1].astype(np.int64)
    want = np.array([semi_dp(query, rows[lane, :n]) for lane, n in enumerate(lens)])
    assert np.array_equal(got, want), (lens, got.tolist(), want.tolist())
    # and the pad would have mattered: scored at the full width, some lane differs
    full = np.array([semi_dp(query, rows[lane]) for lane in range(len(lens))])
    assert (full != want).any()

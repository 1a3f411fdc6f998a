"""Subject buckets of mixed read lengths, the parts that need no GPU: the host helpers (pad_ragged, bin_by_words), the three
new C symbols, and every refusal bgsa_hip_cal_align_score_lens_ex / bgsa_hip_trace_pairs_lens_dev give before anything is
allocated or launched — reached through ctypes with pointers nothing may look at."""
import ctypes

import numpy as np
import pytest

import bgsa_amd as B

P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
EUNSUPPORTED = -2


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- pad_ragged ---------------------------------------------------------------------------------------------------------
def test_pad_ragged_pads_behind_each_end_with_N():
    rows, lens = B.pad_ragged([b"ACGT", np.frombuffer(b"GG", dtype=np.uint8), b"TTTTTTT", bytearray(b"C")])
    assert rows.dtype == np.uint8 and rows.shape == (4, 7)
    assert lens.dtype == np.int32 and lens.tolist() == [4, 2, 7, 1]
    assert [bytes(r) for r in rows] == [b"ACGTNNN", b"GGNNNNN", b"TTTTTTT", b"CNNNNNN"]


def test_pad_ragged_of_equal_lengths_is_the_rows():
    rows, lens = B.pad_ragged([b"ACG", b"TTT"])
    assert [bytes(r) for r in rows] == [b"ACG", b"TTT"] and lens.tolist() == [3, 3]


@pytest.mark.parametrize("subjects", [[b"ACGT", b"", b"AC"], [np.zeros(0, dtype=np.uint8)], []])
def test_pad_ragged_raises_on_an_empty_subject(subjects):
    with pytest.raises(B.BgsaHipError, match="pad_ragged"):
        B.pad_ragged(subjects)


def test_pad_ragged_raises_on_a_matrix():
    with pytest.raises(B.BgsaHipError, match="one-dimensional"):
        B.pad_ragged([np.zeros((2, 3), dtype=np.uint8)])


# ---- bin_by_words -------------------------------------------------------------------------------------------------------
def test_bin_by_words_boundaries():
    # lengths 1, 32, 33, 64, 65 land in bins 1, 1, 2, 2, 3
    bins = B.bin_by_words([1, 32, 33, 64, 65])
    assert [b.tolist() for b in bins] == [[0, 1], [2, 3], [4]]


def test_bin_by_words_is_stable_and_ascending():
    lens = [150, 20, 97, 33, 64, 1, 128, 129, 32, 96, 65]
    bins = B.bin_by_words(lens)
    words = [-(-n // 32) for n in lens]
    assert [sorted(set(words[i] for i in b)) for b in bins] == [[w] for w in sorted(set(words))]   # one word count each, ascending
    for b in bins:
        assert b.tolist() == sorted(b.tolist())                                                    # the caller's order within a bin
    assert sorted(np.concatenate(bins).tolist()) == list(range(len(lens)))                         # every index exactly once
    assert [b.tolist() for b in bins] == [[1, 5, 8], [3, 4], [9, 10], [2, 6], [0, 7]]


def test_bin_by_words_refuses_a_length_of_zero():
    with pytest.raises(B.BgsaHipError, match="not positive"):
        B.bin_by_words([3, 0])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("bgsa_hip_cal_align_score_lens_ex", "bgsa_hip_myers_align_pairs_lens_dev", "bgsa_hip_trace_pairs_lens_dev")


def test_new_symbols_are_declared_and_exported(L):
    names = B.declared_symbols()
    for fn in NEW_SYMBOLS:
        assert fn in names, f"{fn} is not declared in include/bgsa_hip.h"
        assert hasattr(L, fn), f"{fn} is not exported"
    if B.LIB_AB_PATH.exists():
        ab = ctypes.CDLL(str(B.LIB_AB_PATH))
        for fn in NEW_SYMBOLS:
            assert hasattr(ab, fn), f"{fn} is not exported by the A/B flavour"


def _score(L, params, ref_len, read_len, lens=P):
    wn = B.word_num(params.algo, ref_len, read_len, params.k)
    return L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(params), P, P, P, lens, ref_len, read_len, 128, 0, 4, wn, P, 1 << 40, None)


REFUSALS = [
    # (params, ref_len, read_len, what the text names)
    ("banded", B.Params(B.ALGO_BANDED, 0, 0, -1, -1, 8), 150, 150, b"banded filter"),
    ("myers semi-global", B.Params(B.ALGO_MYERS, 1, 0, -1, -1, 0), 150, 150, b"semi-global"),
    ("myers +distance semi-global", B.Params(B.ALGO_MYERS, 1, 0, 1, 1, 0), 150, 150, b"semi-global"),
    ("bitpal semi-global", B.Params(B.ALGO_BITPAL, 1, 2, -3, -5, 0), 150, 150, b"semi-global"),
    ("edit scores under bitpal, semi-global", B.Params(B.ALGO_BITPAL, 1, 0, -1, -1, 0), 150, 150, b"semi-global"),
    ("myers beyond 32 words", B.Params(B.ALGO_MYERS, 0, 0, -1, -1, 0), 150, 1056, b"word_num > 32"),
    ("edit scores under bitpal beyond 32 words", B.Params(B.ALGO_BITPAL, 0, 0, -2, -2, 0), 150, 1025, b"word_num > 32"),
]


@pytest.mark.parametrize("name,params,ref_len,read_len,text", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_lens_refusals_before_any_launch(L, name, params, ref_len, read_len, text):
    rc = _score(L, params, ref_len, read_len)
    assert rc == EUNSUPPORTED, (rc, L.bgsa_hip_last_error())
    err = L.bgsa_hip_last_error()
    assert b"per-subject lengths" in err and text in err, err


def test_lens_refusal_of_a_bitpal_set_beyond_its_register_resident_kernel(L):
    # every compiled set: the first word count its plain kernel does not reach (found through the kernel's name) is refused,
    # with the set and both word counts in the text
    found = 0
    for m, x, g in B.score_sets():
        assert L.bgsa_hip_select_scores(m, x, g) == 0
        try:
            widths = [w for w in range(1, 33) if not L.bgsa_hip_kernel_name(B.ALGO_BITPAL, w).startswith(b"bitpal_asm_kernel")]
        finally:
            assert L.bgsa_hip_select_algorithm(B.ALGO_MYERS) == 0
        if not widths or (m, x, g) == (0, -1, -1):   # 0/-1/-1 in global mode runs on the Myers kernels: nothing to refuse
            continue
        wn = widths[0]
        rc = _score(L, B.Params(B.ALGO_BITPAL, 0, m, x, g, 0), 150, 32 * wn)
        err = L.bgsa_hip_last_error()
        assert rc == EUNSUPPORTED and b"per-subject lengths" in err and f"{m}/{x}/{g}".encode() in err, (rc, err)
        assert f"reaches {wn - 1} words, the bucket has {wn}".encode() in err, err
        found += 1
    assert found >= 1, "no compiled score set has column blocks below 33 words: the refusal went untested"


def test_trace_pairs_lens_refuses_semi_global(L):
    for algo, scores in ((B.ALGO_MYERS, (0, -1, -1)), (B.ALGO_BITPAL, (2, -3, -5))):
        p = B.Params(algo, 1, *scores, 0)
        wn = B.word_num(algo, 150, 150, 0)
        rc = L.bgsa_hip_trace_pairs_lens_dev(ctypes.byref(p), P, P, P, 150, 150, 128, wn, P, P, 10, 4, 0, P, P, P, P, 300, P, 1 << 40, None)
        assert rc == EUNSUPPORTED and b"per-subject lengths" in L.bgsa_hip_last_error(), (rc, L.bgsa_hip_last_error())


def test_lens_entry_points_check_their_arguments_as_the_plain_ones(L):
    p = B.Params(B.ALGO_MYERS, 0, 0, -1, -1, 0)
    # word_num that is not the layout's: EINVAL, with or without lengths
    for lens in (P, None):
        assert L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), P, P, P, lens, 150, 150, 128, 0, 4, 4, P, 1 << 40, None) == -1
        assert L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), P, P, P, lens, 150, 150, 100, 0, 4, 5, P, 1 << 40, None) == -1
    # an empty query window is OK and touches nothing
    assert L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), P, P, P, P, 150, 150, 128, 3, 3, 5, P, 0, None) == 0
    # no pairs: OK, nothing launched
    assert L.bgsa_hip_myers_align_pairs_lens_dev(P, P, P, 150, 150, 128, 5, P, P, 0, 4, 0, P, P, P, 300, P, 1 << 40, None) == 0
    assert L.bgsa_hip_trace_pairs_lens_dev(ctypes.byref(p), P, P, P, 150, 150, 128, 5, P, P, 0, 4, 0, P, P, P, P, 300, P, 1 << 40, None) == 0
    assert L.bgsa_hip_myers_align_pairs_lens_dev(P, P, P, 150, 1056, 128, 33, P, P, 10, 4, 0, P, P, P, 300, P, 1 << 40, None) == EUNSUPPORTED

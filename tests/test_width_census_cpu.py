"""The width census (tests/width_census.py) proves its own completeness on the host: every kernel name the BitPAl dispatch of
either library flavour can produce is reached by a census word count, the pair and band widths are all of 1 .. 32, the listed
block widths no word count reaches are the known ones, and the census inputs are worth launching — the DP oracle alone gives
varied scores on every scoring case and pairs on both sides of the bound on every band case.  No GPU: names, word counts and
window widths are host logic, the conditions are the oracle's."""
import functools
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "bgsa_amd" / "csrc"))

import align_reference as A  # noqa: E402
import banded_align_reference as R  # noqa: E402
import bgsa_amd as B  # noqa: E402
import gen_rows_asm as G  # noqa: E402
import rows_ir  # noqa: E402
import width_census as W  # noqa: E402

FLAVOURS = ["libbgsa_hip.so", "libbgsa_hip_ab.so"]
EDIT_SET = (0, -1, -1)   # global mode: minus the edit distance, on the Myers body (capi.hip make_plan), which has its own census

# The knobs are read once per process, so every library flavour answers from a child of its own (test_kernel_select_cpu.py).
_CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.bgsa_hip_kernel_name.restype = ctypes.c_char_p
ip = ctypes.POINTER(ctypes.c_int)
L.bgsa_hip_score_set.argtypes = [ctypes.c_int, ip, ip, ip, ip]
out = []
for i in range(L.bgsa_hip_score_set_count()):
    m, x, g = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.bgsa_hip_score_set(i, ctypes.byref(m), ctypes.byref(x), ctypes.byref(g), None) == 0
    names = {}
    for mode in (0, 1):
        assert L.bgsa_hip_select_scores(m.value, x.value, g.value) == 0 and L.bgsa_hip_select_alignment(mode) == 0
        names[mode] = [L.bgsa_hip_kernel_name(2, w).decode() for w in range(1, int(sys.argv[2]) + 1)]
    out.append({"scores": [m.value, x.value, g.value], "global": names[0], "semi_global": names[1]})
print(json.dumps(out))
"""


@functools.lru_cache(maxsize=None)
def flavour_names(flavour):
    """{(match, mismatch, gap): {"global" | "semi_global": names of 1 .. 130 words}} of one library flavour."""
    path = B.HERE / flavour
    if not path.exists():
        B.build_library()
    knobs = ("BGSA_MYERS_", "BGSA_BANDED_", "BGSA_BITPAL_", "BGSA_HIP_LIB", "BGSA_DYNAMIC_")
    env = {k: v for k, v in os.environ.items() if not k.startswith(knobs)}
    p = subprocess.run([sys.executable, "-c", _CHILD, str(path), str(W.NAME_WORDS)], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    return {tuple(e["scores"]): {"global": e["global"], "semi_global": e["semi_global"]} for e in json.loads(p.stdout)}


def every_set():
    return sorted(set().union(*(flavour_names(f) for f in FLAVOURS)))


def bitpal_modes():
    """(scores, mode) of every compiled set of either flavour that runs BitPAl kernels."""
    return [(scores, mode) for scores in every_set() for mode in ("global", "semi_global") if (scores, mode) != (EDIT_SET, "global")]


def names_of(scores, mode):
    return next(flavour_names(f)[scores][mode] for f in FLAVOURS if scores in flavour_names(f))


# ---- BitPAl names -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_bitpal_kernel_name_is_reached_by_a_census_word_count(flavour):
    table = flavour_names(flavour)
    assert (2, -3, -5) in table and EDIT_SET in table and len(table) >= 5
    for scores, by_mode in table.items():
        assert all("myers" in n for n in by_mode["global"]) == (scores == EDIT_SET)
        for mode, names in by_mode.items():
            if (scores, mode) == (EDIT_SET, "global"):
                continue
            assert len(names) == W.NAME_WORDS and all(n.startswith("bitpal_") for n in names)
            counts = W.word_counts(names)
            missed = set(names) - {names[w - 1] for w in counts}
            assert not missed, f"{flavour} {scores} {mode}: no census word count reaches {sorted(missed)}"
            # every plain width is a word count of its own, and every (block width, 2 | 3 | 4 blocks) the dispatch picks is reached
            plain, wide = W.max_plain(names), W.widest_block(names)
            assert names[:plain] == [f"{W.PLAIN}{w}>" for w in range(1, plain + 1)] and set(range(1, plain + 1)) <= set(counts)
            blocks = {(W.name_width(names[w - 1]), -(-w // W.name_width(names[w - 1]))) for w in range(plain + 1, W.NAME_WORDS + 1)}
            reached = {(W.name_width(names[w - 1]), -(-w // W.name_width(names[w - 1]))) for w in counts if w > plain}
            assert {b for b in blocks if b[1] <= 4} <= reached, (flavour, scores, mode)
            assert any(n >= 5 for _, n in reached)                      # the wider case
            assert counts[-1] == W.WIDER_WORDS and counts[:-1] == list(range(1, 4 * wide + 2))


def test_the_census_ranges_are_the_issues():
    # 1 .. 33 for the sets with register-resident kernels up to 12 words, 1 .. 17 for the two whose blocks stop at 4 words
    tops = {scores: W.word_counts(names_of(scores, "semi_global"))[-2] for scores in every_set()}
    assert tops == {(0, -1, -1): 33, (1, -1, -2): 33, (1, -3, -2): 33, (1, -4, -2): 33, (2, -3, -5): 33, (5, -4, -10): 17, (10, -9, -15): 17}
    assert {scores: W.max_plain(names_of(scores, "semi_global")) for scores in every_set()} == \
        {(0, -1, -1): 12, (1, -1, -2): 12, (1, -3, -2): 12, (1, -4, -2): 12, (2, -3, -5): 12, (5, -4, -10): 8, (10, -9, -15): 4}


# ---- block widths that are listed and never picked ------------------------------------------------------------------------------
# Widths::pick_blocks takes the narrowest listed width that covers the subject with the fewest blocks of the WIDEST one, and
# the column blocks begin past the widest plain kernel: 13 words over widths 5 .. 8 are 2 x 7, so <5> is never picked; 5 words
# over 1 .. 4 are 2 x 3 and 9 words 3 x 3, so <1> and <2> are never picked.  Removing them is a build change; a change in
# pick_blocks or in a generator list shows here either way.
UNREACHABLE = {
    "libbgsa_hip.so": {(0, -1, -1): ["bitpal_blocked_kernel<5>"], (1, -1, -2): ["bitpal_blocked_kernel<5>"],
                       (1, -4, -2): ["bitpal_blocked_kernel<5>"], (2, -3, -5): ["bitpal_blocked_kernel<5>"],
                       (10, -9, -15): ["bitpal_packed_blocked_kernel<1>", "bitpal_packed_blocked_kernel<2>"]},
    "libbgsa_hip_ab.so": {(0, -1, -1): ["bitpal_blocked_kernel<5>"], (1, -1, -2): ["bitpal_blocked_kernel<5>"],
                          (1, -3, -2): ["bitpal_blocked_kernel<5>"], (1, -4, -2): ["bitpal_blocked_kernel<5>"],
                          (2, -3, -5): ["bitpal_blocked_kernel<5>"],
                          (5, -4, -10): ["bitpal_blocked_kernel<1>", "bitpal_blocked_kernel<2>"],
                          (10, -9, -15): ["bitpal_packed_blocked_kernel<1>", "bitpal_packed_blocked_kernel<2>"]},
}


@pytest.mark.parametrize("flavour", FLAVOURS)
def test_listed_block_widths_no_word_count_reaches(flavour):
    got = {}
    for scores, by_mode in flavour_names(flavour).items():
        plain, blocks, packed = G.bitpal_widths(rows_ir.BitpalScores(*scores))
        names = by_mode["semi_global"]
        assert plain == list(range(1, W.max_plain(names) + 1))          # the generator's list is what the library was built from
        kernel = "bitpal_packed_blocked_kernel" if packed else "bitpal_blocked_kernel"
        got[scores] = [f"{kernel}<{nw}>" for nw in blocks if f"{kernel}<{nw}>" not in names]
        assert {n for n in names if not n.startswith(W.PLAIN)} <= {f"{kernel}<{nw}>" for nw in blocks}
    assert got == UNREACHABLE[flavour]


# ---- pair and band widths ---------------------------------------------------------------------------------------------------------
def test_pair_word_counts_are_all_of_1_to_32():
    assert W.PAIR_WORDS == list(range(1, 33)) == W.LENS_WORDS_MYERS
    for w in W.PAIR_WORDS:
        for m, n in W.pair_shapes(w):
            assert B.word_num(B.ALGO_MYERS, m, n) == w
        assert (W.pair_shapes(w)[1][1] - 1) // 32 == (W.pair_shapes(w)[1][0] - 1) // 32 == w - 1   # near-square: the last word on both sides
        lens = W.lens_lengths(w)
        assert max(lens) == 32 * w and min(lens) >= 1 and 64 <= len(lens) <= 130
        assert {max(1, x) for x in (1, 32 * (w - 1), 32 * (w - 1) + 1, 32 * w - 5, 32 * w - 1, 32 * w)} <= set(lens)


# Window widths 1 .. 32 that bgsa_hip_align_pairs_band_words returns for no scanned shape with n <= 1,100: none.  (It also
# answers 33, 34 and 35 there — the whole subject of 1,025 .. 1,100 bp —, which the kernels refuse: kBandTraceMaxWords = 32.)
BAND_WORDS_NEVER_PRODUCED = []


def test_band_triples_cover_every_window_width_the_helper_returns():
    L = B.lib()
    seen = set()
    for n in list(range(1, W.BAND_MAX_N + 1, 7)) + [1024, 1025, W.BAND_MAX_N]:
        for m in {n, max(1, n - 11), max(1, n - 21), n + 13}:
            delta = abs(n - m)
            for bound in sorted({delta, delta + 1, delta + 9, 31, 32, 33, 64, 100, 150, 250, 400, 550, 700, 850, 962, 1000, 1100, m + n}):
                v = L.bgsa_hip_align_pairs_band_words(m, n, bound)
                assert v == R.band_words(m, n, bound), (m, n, bound)     # the model the triples were found with
                seen.add(v)
    triples = W.band_triples()
    assert {v for v in seen if 1 <= v <= 32} <= set(triples)
    assert sorted(triples) == W.BAND_WORDS == [v for v in range(1, 33) if v not in BAND_WORDS_NEVER_PRODUCED]
    assert max(seen) == 35 and L.bgsa_hip_align_pairs_band_words(100, 111, 10) == 0      # |n - m| beyond the bound: no window
    for v, (m, n, bound) in triples.items():
        assert L.bgsa_hip_align_pairs_band_words(m, n, bound) == v and n <= 1024 and abs(n - m) <= bound < max(m, n)


@pytest.mark.parametrize("v", W.BAND_WORDS)
def test_band_cases_hold_pairs_on_both_sides_of_the_bound(v):
    m, n, bound = W.band_triples()[v]
    q, s = W.band_case(m, n, bound)
    distances = [d for d, _ in A.canonical(q, s)]
    assert min(distances) <= bound < max(distances), (m, n, bound, distances)
    assert sum(d <= bound for d in distances) >= 2


# ---- the oracle alone on the scoring cases ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores,mode", bitpal_modes(), ids=lambda x: x if isinstance(x, str) else "/".join(map(str, x)))
def test_scoring_cases_are_worth_launching(oracle, scores, mode):
    """Conditions, not measurements, on the DP oracle alone:
    * at least 5 distinct scores per case (measured minimum: 6, in the global cases of every set);
    * the worst possible score gap * (qlen + slen) stays inside int16 (most negative: -17,760 = -15 * (64 + 1,120), the
      35-word case of 10/-9/-15; -16,800 up to 33 words);
    * global cases: a planted row 0 .. 11 never scores below the median of the random rows against its own query, and strictly
      above it wherever slen <= 2 qlen.  Strictly above cannot hold at every width: with the gaps that slen - qlen forces
      paid by every subject alike, a random subject of three query lengths or more holds the whole query as a subsequence and
      reaches the same optimum as the planted copy (from 40 x 123 and 64 x 256 on, in every set);
    * 2/-3/-5 global: the DP checker and the restated reference kernel agree on the census inputs."""
    semi = mode == "semi_global"
    names = names_of(scores, mode)
    cases = W.scoring_cases(names, semi)
    assert len(cases) == 3 * len(W.word_counts(names))
    for w, qlen, slen in cases:
        q, s = W.scoring_case(w, qlen, slen, semi)
        assert q.shape == (W.N_QUERIES, qlen) and s.shape == (W.N_SUBJECTS, slen) and B.word_num(B.ALGO_BITPAL, qlen, slen) == w
        want = (oracle.dp_semiglobal if semi else oracle.dp_nw)(q, s, *scores)
        assert len(np.unique(want)) >= 5, (w, qlen, slen)
        assert -32768 <= scores[2] * (qlen + slen), (w, qlen, slen)
        if semi:
            continue
        median = np.median(want[:, W.FIRST_RANDOM:], axis=1)
        for i in range(W.PLANTED):
            assert want[i % W.N_QUERIES, i] >= median[i % W.N_QUERIES], (w, qlen, slen, i)
            if slen <= 2 * qlen:
                assert want[i % W.N_QUERIES, i] > median[i % W.N_QUERIES], (w, qlen, slen, i)
        if scores == (2, -3, -5):
            assert np.array_equal(want, oracle.bitpal(q, s)), (w, qlen, slen)
    if semi:   # the planted queries of rows 16 .. 23 straddle a word boundary, and a block boundary where there are blocks
        for w, qlen, slen in cases:
            if slen > qlen + 32:
                spans = [(off // 32, (off + qlen - 1) // 32) for off in W.plant_offsets(w, qlen, slen)]
                assert all(a < b for a, b in spans), (w, qlen, slen)
                nw = W.name_width(names[w - 1])
                assert w <= W.max_plain(names) or any(a < nw * k <= b for a, b in spans for k in range(1, 5)), (w, qlen, slen)

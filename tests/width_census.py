"""The width census — a helper, not a test: the ONE place that says which shapes launch every BitPAl, length-aware (LENS),
align_pairs and align_pairs_banded instantiation.  tests/test_width_census_cpu.py proves on the host that these shapes reach
every kernel name the dispatch can produce; tests/test_width_census_gpu.py launches them against the DP.

Word counts are derived from the library's own answers (bgsa_hip_kernel_name, bgsa_hip_align_pairs_band_words), never from a
list copied here: a width added to a generator list changes the names, and the CPU test fails until the census reaches it."""
import functools
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import banded_align_reference as R  # noqa: E402
import oracle as O  # noqa: E402

BITPAL = 2                      # BGSA_ALGO_BITPAL
NAME_WORDS = 130                # kernel names are asked for 1 .. 130 words (4,160 bp), as tests/golden/kernel_names.json does
WIDER_WORDS = 35                # one case per set beyond 4 blocks: 5 blocks of 7 words, 9 blocks of 4
PLAIN = "bitpal_asm_kernel<"

A_, C_, N_ = ord("A"), ord("C"), ord("N")


# ---- which word counts --------------------------------------------------------------------------------------------------------
def bitpal_names(L, scores, semi, upto=NAME_WORDS):
    """bgsa_hip_kernel_name(BITPAL, w) for w = 1 .. upto under the score set and alignment mode, which are left selected.
    L: a CDLL of either flavour whose bgsa_hip_kernel_name has restype c_char_p."""
    assert L.bgsa_hip_select_scores(*scores) == 0
    assert L.bgsa_hip_select_alignment(1 if semi else 0) == 0
    return [L.bgsa_hip_kernel_name(BITPAL, w).decode() for w in range(1, upto + 1)]


def name_width(name):
    return int(re.search(r"<(\d+)", name).group(1))


def max_plain(names):
    """The widest subject, in words, the register-resident kernel of the set takes: names[w - 1] is its name up to there."""
    return sum(1 for n in names if n.startswith(PLAIN))


def widest_block(names):
    """W: the widest column-block width the dispatch ever names for the set (0: none)."""
    return max((name_width(n) for n in names if not n.startswith(PLAIN)), default=0)


def word_counts(names):
    """1 .. 4 W + 1 — every plain width and every reachable (block width, 2 | 3 | 4 blocks), with the first count of 5 blocks —
    and one wider case."""
    top = max(4 * widest_block(names) + 1, max_plain(names))
    return list(range(1, top + 1)) + ([WIDER_WORDS] if WIDER_WORDS > top else [])


# ---- scoring cases ------------------------------------------------------------------------------------------------------------
N_QUERIES, N_SUBJECTS = 4, 128   # two subject groups: the second wave of a workgroup and the two-group paths are live
PLANTED = 12                     # rows 0 .. 11: mutated query prefixes
FIRST_RANDOM = 24                # rows from here on are random reads in every mode


def shapes(w):
    """(qlen, slen): one 32-row chunk plus a tail and a partial last word; two full chunks (tail_rows == 0); a full last word
    (the rem >= 32 side of the column masks)."""
    return [(40, 32 * w - 5), (64, 32 * w - 5), (64, 32 * w)]


def plant_offsets(w, qlen, slen):
    """Where the semi-global cases put a query inside rows 16 .. 23: centred on the word boundaries 1, 3, 4, 6, 7, 8 (the
    column-block widths, so a block boundary where there are blocks), the middle and the last one."""
    words = [1, 3, 4, 6, 7, 8, max(1, w // 2), max(1, w - 1)]
    return [int(np.clip(32 * min(b, w - 1) - qlen // 2, 0, slen - qlen)) for b in words]


@functools.lru_cache(maxsize=None)
def queries(qlen):
    q = O.gen_reads(0xC0DE + qlen, N_QUERIES, qlen)
    q[2] = A_
    q[3, 0::2], q[3, 1::2] = A_, C_
    q.setflags(write=False)
    return q


@functools.lru_cache(maxsize=512)
def scoring_case(w, qlen, slen, semi):
    """(queries[4, qlen], subjects[128, slen]); shared and never modified."""
    q = queries(qlen)
    s = O.gen_reads(0xC0DF + w, N_SUBJECTS, slen)
    m = min(qlen, slen)
    rows = np.arange(PLANTED)
    s[:PLANTED, :m] = O.mutate(q[rows % N_QUERIES][:, :m], rows % 7, 0xBEEF + w)
    s[12] = A_           # with query row 2: every add chain carries through every word and across every block boundary
    s[13] = C_
    s[14] = N_
    s[15, 0::2], s[15, 1::2] = C_, A_
    if semi and slen > qlen:
        for r, off in zip(range(16, 24), plant_offsets(w, qlen, slen)):
            s[r, off: off + qlen] = O.mutate(q[r % N_QUERIES][None, :], [r % 3], 0xFACE + 64 * w + r)[0]
    s.setflags(write=False)
    return q, s


def scoring_cases(names, semi):
    """[(w, qlen, slen)] of one (score set, mode), from its kernel names."""
    return [(w, qlen, slen) for w in word_counts(names) for qlen, slen in shapes(w)]


# ---- pair cases (align_pairs) ---------------------------------------------------------------------------------------------------
PAIR_WORDS = list(range(1, 33))
PAIR_EDITS = [0, 1, 3, 9] * 3


def pair_shapes(w):
    """(m, n): a short query against w words with a partial last word; near-square, so that the traceback crosses every word."""
    return [(40, 32 * w - 5), (32 * w - 3, 32 * w)]


@functools.lru_cache(maxsize=None)
def pair_case(m, n):
    """(queries[16, m], subjects[16, n]), pair p = (query p, subject p): 12 mutated copies with 0, 1, 3 and 9 edits, all
    mismatch, homopolymer against homopolymer (every cell a tie), an 'N' run in the subject, an 'N' run in both."""
    seed = 104729 * m + n
    longest = max(m, n)
    base = O.gen_reads(seed, 16, longest)
    mutants = O.mutate(base, PAIR_EDITS + [0, 0, 2, 2], seed + 1)
    q, s = np.array(base[:, :m]), np.array(mutants[:, :n])
    q[12], s[12] = A_, C_
    q[13], s[13] = A_, A_
    s[14, n // 3: n // 3 + max(1, n // 5)] = N_
    q[15, m // 2: m // 2 + max(1, m // 7)] = N_
    s[15, n // 2: n // 2 + max(1, n // 7)] = N_
    q.setflags(write=False)
    s.setflags(write=False)
    return q, s


# ---- band cases (align_pairs_banded) ----------------------------------------------------------------------------------------------
BAND_MAX_N = 1100                # the CPU test scans the helper's answers up to here
BAND_WORDS = list(range(1, 33))   # kBandTraceMaxWords: wider windows are refused
# subjects up to 1,024 bp, so that align_pairs can score the same pairs
BAND_SHAPES = [(m, n) for n in (27, 60, 150, 300, 420, 600, 800, 1000) for m in (n, n - 11, n - 21)]


@functools.lru_cache(maxsize=None)
def band_triples():
    """{band_words: (m, n, max_distance)}: per window width 1 .. 32 the first shape of BAND_SHAPES and its smallest bound that
    give it, the bound below the longer length (an all-mismatch pair then lies beyond it).  Found with the integer model
    (banded_align_reference.band_words, monotone in the bound); the CPU test holds the library's answer against it."""
    out = {}
    for m, n in BAND_SHAPES:
        top = max(m, n) - 1
        for v in BAND_WORDS:
            if v in out or R.band_words(m, n, top) < v:
                continue
            lo, hi = abs(n - m), top                       # the smallest bound whose window is at least v words
            while lo < hi:
                mid = (lo + hi) // 2
                lo, hi = (lo, mid) if R.band_words(m, n, mid) >= v else (mid + 1, hi)
            if R.band_words(m, n, lo) == v:
                out[v] = (m, n, lo)
    return out


@functools.lru_cache(maxsize=None)
def band_case(m, n, bound):
    """(queries[8, m], subjects[8, n]): mutated copies with 0, 1, 3 edits and about half the bound's slack — within the bound
    —, twice the bound and four times the bound, a random pair and all mismatch (beyond it)."""
    seed = 1299709 * m + 31 * n + bound
    slack = bound - abs(n - m)
    longest = max(m, n)
    base = O.gen_reads(seed, 8, longest)
    mutants = O.mutate(base, [0, 1, min(3, slack // 2), slack // 3, 2 * bound + 2, 4 * bound + 4, 0, 0], seed + 1)
    mutants[6] = O.gen_reads(seed + 2, 1, longest)[0]
    q, s = np.array(base[:, :m]), np.array(mutants[:, :n])
    q[7], s[7] = A_, C_
    q.setflags(write=False)
    s.setflags(write=False)
    return q, s


# ---- LENS buckets -----------------------------------------------------------------------------------------------------------------
LENS_WORDS_MYERS = list(range(1, 33))
LENS_QLEN, LENS_QUERIES, LENS_SUBJECTS = 50, 3, 70    # 70 subjects: two groups, 58 padding columns


def lens_lengths(w):
    """70 lengths whose longest has w words: both edges of the last word and of the one before, cycled, and six in between."""
    edge = sorted({max(1, n) for n in (1, 32 * (w - 1), 32 * (w - 1) + 1, 32 * w - 5, 32 * w - 1, 32 * w)})
    rng = np.random.default_rng(0x1E75 + w)
    lens = [edge[i % len(edge)] for i in range(LENS_SUBJECTS - 6)] + [int(x) for x in rng.integers(1, 32 * w + 1, 6)]
    assert max(lens) == 32 * w and len(lens) == LENS_SUBJECTS
    return lens


@functools.lru_cache(maxsize=None)
def lens_bucket(w):
    """(queries[3, 50], subjects: list of 70 1-D arrays) — make_bucket of tests/test_ragged_gpu.py on lens_lengths(w)."""
    from test_ragged_gpu import make_bucket
    q, subjects, _ = make_bucket(0x1E75_0000 + w, LENS_QUERIES, LENS_QLEN, lens_lengths(w))
    return q, subjects

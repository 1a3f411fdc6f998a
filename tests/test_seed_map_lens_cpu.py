"""Seeded read mapping for reads of mixed lengths, without a GPU: seed_plan_ragged, the COMPLETENESS of the per-read candidate rule
(tests/seed_map_reference.py's candidates, called with every read's own length and bound, against a brute-force semi-global DP
over every window) and the refusals of the three *_lens_dev calls, which come before any HIP call, so fake pointers do."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import reference_map_reference as M  # noqa: E402
import seed_map_reference as R  # noqa: E402
from align_reference import classes  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SYMBOLS = ("bgsa_hip_seed_count_candidates_lens_dev", "bgsa_hip_seed_emit_candidates_lens_dev", "bgsa_hip_reference_verify_pairs_lens_dev")


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


def count_dev(L, ref_len=1000, W=64, S=20, offsets=P, positions=P, q=6, reads=P, lens=P, n=32, n_reads=1, bound=4, both=1, cap=100, counts=P):
    return L.bgsa_hip_seed_count_candidates_lens_dev(ref_len, W, S, offsets, positions, q, reads, lens, n, n_reads, bound, both, cap, counts,
                                                     None)


def emit_dev(L, ref_len=1000, W=64, S=20, offsets=P, positions=P, q=6, reads=P, lens=P, n=32, n_reads=1, bound=4, both=1, counts=P,
             prefix=P, base=0, out_read=P, out_window=P):
    return L.bgsa_hip_seed_emit_candidates_lens_dev(ref_len, W, S, offsets, positions, q, reads, lens, n, n_reads, bound, both, counts,
                                                    prefix, base, out_read, out_window, None)


def verify_dev(L, ref=P, ref_len=1000, W=64, S=20, peq=P, lens=P, n=32, read_count=64, wn=1, windows=P, subjects=P, n_pairs=1, base=0,
               distance=P, work=None, work_bytes=0):
    return L.bgsa_hip_reference_verify_pairs_lens_dev(ref, ref_len, W, S, peq, lens, n, read_count, wn, windows, subjects, n_pairs, base,
                                                      distance, work, work_bytes, None)


# ---- 1. the plan ------------------------------------------------------------------------------------------------------------
def test_seed_plan_ragged_bins_and_seed_lengths():
    lens = [30, 32, 33, 64, 65, 80]
    plan = B.seed_plan_ragged(lens, 4)
    assert [(idx.tolist(), q) for idx, q in plan] == [([0, 1], 6), ([2, 3], 6), ([4, 5], 12)]
    assert [((max(lens[i] for i in idx) + 31) // 32, q) for idx, q in plan] == [(1, 6), (2, 6), (3, 12)]
    for (idx, _), want in zip(plan, B.bin_by_words(lens)):          # bin_by_words' bins, in its order
        assert np.array_equal(idx, want)
    shuffled = [80, 30, 65, 33, 32, 64]                             # the caller's order is kept inside a bin
    assert [(idx.tolist(), q) for idx, q in B.seed_plan_ragged(shuffled, 4)] == [([1, 4], 6), ([3, 5], 6), ([0, 2], 12)]
    assert [q for _, q in B.seed_plan_ragged([150, 100, 140], 12)] == [7, 10]      # 100 // 13 = 7; 140 // 13 = 10
    assert [q for _, q in B.seed_plan_ragged([150, 100, 140], 3)] == [12, 12]      # min(12, step)
    assert [q for _, q in B.seed_plan_ragged(lens, 4, seed_len=8)] == [8, 8, 8]
    assert [q for _, q in B.seed_plan_ragged(np.array(lens, np.int32), 0)] == [12, 12, 12]


def test_a_read_shorter_than_the_bound_plus_one_gives_a_seed_of_one():
    assert [q for _, q in B.seed_plan_ragged([4, 30], 4)] == [1]        # 4 // (4 + 1) = 0
    assert [q for _, q in B.seed_plan_ragged([3, 64], 7)] == [1, 8]     # min(7, 3) = 3: 3 // 4 = 0; 64 // 8 = 8
    assert [q for _, q in B.seed_plan_ragged([5, 30], 4)] == [1]        # exactly B + 1: step 1
    assert [q for _, q in B.seed_plan_ragged([1], 0)] == [1]


def test_seed_plan_ragged_refusals():
    for bad in (0, -1, 14):
        with pytest.raises(B.BgsaHipError, match="1..13"):
            B.seed_plan_ragged([30, 64], 4, seed_len=bad)
    assert [q for _, q in B.seed_plan_ragged([30, 64], 4, seed_len=13)] == [13, 13]
    assert [q for _, q in B.seed_plan_ragged([30, 64], 4, seed_len=1)] == [1, 1]
    with pytest.raises(B.BgsaHipError, match="negative"):
        B.seed_plan_ragged([30], -1)
    with pytest.raises(B.BgsaHipError, match="not positive"):
        B.seed_plan_ragged([30, 0], 4)
    assert B.seed_plan_ragged([], 4) == []


# ---- 2. completeness of the per-read rule against brute force ---------------------------------------------------------------
def test_no_window_within_a_reads_own_bound_is_missing_from_its_candidates():
    """Mixed lengths in one list, every read with its own n_r, B_r = min(B, n_r) and the q of its bin (seed_plan_ragged): a read
    that is not flagged -3 (step_r >= q) must have every window within B_r among its candidates, on both strands."""
    rng = np.random.default_rng(20261020)
    shapes = within = reverse_found = anchored = short = exact = explicit = 0
    while shapes < 120:
        letters = np.frombuffer(b"ACGT" if shapes % 2 else b"AC", np.uint8)
        L_ = int(rng.integers(100, 181))
        bound = int(rng.integers(0, 5))
        lens = [int(x) for x in rng.integers(6, 71, size=5)] + [bound + 1]           # a length of exactly B + 1: step 1
        if shapes % 3 == 0:
            lens.append(int(rng.integers(1, bound + 1)) if bound else 1)                # not longer than the bound (or 1 bp)
        longest = max(lens)
        W = int(rng.integers(longest + bound, min(L_, longest + bound + 30) + 1))
        S = int(rng.integers(1, min(W, M.largest_stride(W, longest, min(bound, longest))) + 1))
        ref = letters[rng.integers(letters.size, size=L_)].copy()
        n_windows = M.window_count(L_, W, S)
        seed_len = int(rng.integers(1, 9)) if shapes % 4 == 3 else None
        explicit += seed_len is not None
        plan = B.seed_plan_ragged(lens, bound, seed_len)
        assert sorted(i for idx, _ in plan for i in idx.tolist()) == list(range(len(lens)))
        shapes += 1
        anchored += (L_ - W) % S != 0
        for idx, q in plan:
            buckets = R.buckets_of(classes(ref), q)
            for at, i in enumerate(idx.tolist()):
                n = lens[i]
                kind = (at + shapes) % 3
                begin = L_ - n - 4 if kind == 2 else int(rng.integers(0, L_ - n - 4))   # kind 2: at the end, in the anchored last window
                b_r = min(bound, n)
                src = _edit(rng, list(ref[begin: begin + n + 4]), int(rng.integers(0, b_r + 1)), letters)     # 4 spare: up to 4 deletions
                read = np.array(src[:n], np.uint8)
                if kind == 1:
                    read = M.reverse_complement(read)
                assert read.size == n
                if n // (b_r + 1) < q:                                                  # flag -3: the exhaustive path answers
                    short += 1
                    continue
                exact += n == bound + 1
                distances = R.window_distances(ref, W, S, read)
                assert distances.size == 2 * n_windows
                cands = set(R.candidates(lambda value: buckets.get(value, ()), L_, W, S, read, b_r, q))
                assert all(0 <= g < 2 * n_windows for g in cands)
                near = np.flatnonzero(distances <= b_r)
                missing = [int(g) for g in near if int(g) not in cands]
                assert not missing, (L_, W, S, n, bound, q, kind, missing)
                within += near.size
                reverse_found += int((near >= n_windows).sum())
    assert within >= 1000 and reverse_found >= 200, (within, reverse_found)       # the test cannot pass vacuously
    assert anchored >= 30 and short >= 30 and exact >= 30 and explicit >= 25, (anchored, short, exact, explicit)


def test_the_pad_behind_a_reads_end_is_outside_every_piece():
    """What flag -1 looks at: the pieces of n_r, on both strands, end at or before n_r whenever the read is not flagged -3."""
    for n in range(1, 90):
        for bound in range(0, 14):
            b_r = min(bound, n)
            step = n // (b_r + 1)
            for q in range(1, min(step, 13) + 1):
                assert max(R.piece_starts(n, b_r)) + q <= n
                row = np.concatenate([np.frombuffer(b"ACGT" * 23, np.uint8)[:n], np.full(7, ord("N"), np.uint8)])   # a padded row
                assert not R.has_n_piece(row[:n], b_r, q)


# ---- 3. the C calls' refusals, no device ------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_flavours(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared, name
            assert hasattr(flavour, name), (path.name, name)
    assert hasattr(B, "seed_plan_ragged") and hasattr(B.ReferenceMapper, "map_reads_seeded_ragged")


def test_a_null_length_array_is_refused(L):
    assert count_dev(L, lens=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert emit_dev(L, lens=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert verify_dev(L, lens=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert verify_dev(L, lens=None, n_pairs=0) == EINVAL and count_dev(L, lens=None, n_reads=0) == EINVAL


def test_null_outputs_and_inputs_are_refused(L):
    for name in ("offsets", "positions", "reads", "counts"):
        assert count_dev(L, **{name: None}) == EINVAL, name
    for name in ("offsets", "positions", "reads", "counts", "prefix", "out_read", "out_window"):
        assert emit_dev(L, **{name: None}) == EINVAL, name
    for name in ("ref", "peq", "windows", "subjects", "distance"):
        assert verify_dev(L, **{name: None}) == EINVAL, name


def test_word_num_and_read_count_are_checked(L):
    assert verify_dev(L, n=32, wn=2) == EINVAL and verify_dev(L, n=33, wn=1) == EINVAL and verify_dev(L, n=32, wn=0) == EINVAL
    assert verify_dev(L, n=150, wn=4, W=400) == EINVAL and b"ceil(read_len / 32)" in L.bgsa_hip_last_error()
    for read_count in (63, 65, 0, -64):
        assert verify_dev(L, read_count=read_count) == EINVAL and b"multiple of 64" in L.bgsa_hip_last_error()
    assert verify_dev(L, n=1056, wn=33, W=2000, ref_len=5000, work=P, work_bytes=1 << 40) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()
    assert verify_dev(L, n=513, wn=17, W=600) == EINVAL and b"workspace" in L.bgsa_hip_last_error()       # column blocks need carries
    assert verify_dev(L, n=513, wn=17, W=600, work=P, work_bytes=100) == EINVAL


def test_the_other_checks_are_those_of_the_equal_length_calls(L):
    for q in (0, 14):
        assert count_dev(L, q=q) == EINVAL and b"1..13" in L.bgsa_hip_last_error() and emit_dev(L, q=q) == EINVAL
    for ref_len, W, S in ((1000, 64, 0), (1000, 64, 65), (63, 64, 20)):
        assert count_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL and emit_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
        assert verify_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
    assert count_dev(L, n_reads=-1) == EINVAL and emit_dev(L, n_reads=-1) == EINVAL and verify_dev(L, n_pairs=-1) == EINVAL
    assert count_dev(L, cap=-1) == EINVAL and count_dev(L, bound=-1) == EINVAL and emit_dev(L, base=-1) == EINVAL
    # nothing to do is fine once the checks pass: fake pointers, so a launch would fault
    assert count_dev(L, n_reads=0) == 0 and emit_dev(L, n_reads=0) == 0 and verify_dev(L, n_pairs=0) == 0
    assert verify_dev(L, n=513, wn=17, W=600, n_pairs=0, work=P, work_bytes=1 << 20) == 0


def test_overlapping_seeds_are_a_flag_not_a_refusal(L):
    """step < seed_len for the bucket's width refuses the equal-length calls; the lens calls leave it to every read's flag -3."""
    assert L.bgsa_hip_seed_count_candidates_dev(1000, 64, 20, P, P, 7, P, 32, 0, 4, 1, 100, P, None) == EINVAL
    assert count_dev(L, n=32, bound=4, q=7, n_reads=0) == 0 and emit_dev(L, n=32, bound=4, q=7, n_reads=0) == 0
    assert count_dev(L, n=32, bound=40, q=1, n_reads=0) == 0

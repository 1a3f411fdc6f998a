"""Seeded read mapping, without a GPU: the new symbols in the header and in both library flavours, the C ABI's refusals (they come
before any HIP call, so fake pointers do), the pieces and the seed rule, the flags, and the COMPLETENESS of the candidate rule as
tests/seed_map_reference.py restates it: against a brute-force DP over every window, no window within the bound may be missing."""
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
INT32_MAX = 2 ** 31 - 1
SYMBOLS = ("bgsa_hip_seed_index_offsets", "bgsa_hip_seed_index_workspace_bytes", "bgsa_hip_seed_index_build_dev",
           "bgsa_hip_seed_count_candidates_dev", "bgsa_hip_seed_emit_candidates_dev", "bgsa_hip_reference_verify_workspace_bytes",
           "bgsa_hip_reference_verify_pairs_dev", "bgsa_hip_seed_select_dev")


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


def build_dev(L, ref=P, ref_len=1000, q=6, offsets=P, positions=P, work=P, work_bytes=1 << 40):
    return L.bgsa_hip_seed_index_build_dev(ref, ref_len, q, offsets, positions, work, work_bytes, None)


def count_dev(L, ref_len=1000, W=64, S=20, offsets=P, positions=P, q=6, reads=P, n=32, n_reads=1, bound=4, both=1, cap=100, counts=P):
    return L.bgsa_hip_seed_count_candidates_dev(ref_len, W, S, offsets, positions, q, reads, n, n_reads, bound, both, cap, counts, None)


def emit_dev(L, ref_len=1000, W=64, S=20, offsets=P, positions=P, q=6, reads=P, n=32, n_reads=1, bound=4, both=1, counts=P, prefix=P,
             base=0, out_read=P, out_window=P):
    return L.bgsa_hip_seed_emit_candidates_dev(ref_len, W, S, offsets, positions, q, reads, n, n_reads, bound, both, counts, prefix, base,
                                               out_read, out_window, None)


def verify_dev(L, ref=P, ref_len=1000, W=64, S=20, peq=P, n=32, read_count=64, wn=1, windows=P, subjects=P, n_pairs=1, base=0,
               distance=P, work=None, work_bytes=0):
    return L.bgsa_hip_reference_verify_pairs_dev(ref, ref_len, W, S, peq, n, read_count, wn, windows, subjects, n_pairs, base, distance,
                                                 work, work_bytes, None)


def select_dev(L, windows=P, distance=P, segments=P, n_reads=1, bound=4, k=3, scores=P, hits=P):
    return L.bgsa_hip_seed_select_dev(windows, distance, segments, n_reads, bound, k, scores, hits, None)


# ---- 1. symbols -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_flavours(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared, name
            assert hasattr(flavour, name), (path.name, name)
    for name in ("seed_plan", "blank_beyond"):
        assert hasattr(B, name)
    for name in ("map_reads_seeded", "seed_index", "select_seeded"):
        assert hasattr(B.ReferenceMapper, name)


def test_host_only_sizes(L):
    for q in range(1, 14):
        assert L.bgsa_hip_seed_index_offsets(q) == 4 ** q + 1
        assert L.bgsa_hip_seed_index_workspace_bytes(1000, q) >= 4 * 4 ** q
    for q in (0, -1, 14):
        assert L.bgsa_hip_seed_index_offsets(q) == -1 and b"1..13" in L.bgsa_hip_last_error()
        assert L.bgsa_hip_seed_index_workspace_bytes(1000, q) == 0
    assert L.bgsa_hip_seed_index_workspace_bytes(INT32_MAX + 1, 6) == 0
    assert L.bgsa_hip_reference_verify_workspace_bytes(400, 512, 1000) == 0          # 16 words: everything stays in registers
    one = L.bgsa_hip_reference_verify_workspace_bytes(400, 513, 0)
    assert one == 13 * 3 * 64 * 4 == L.bgsa_hip_reference_verify_workspace_bytes(400, 513, 64)
    assert L.bgsa_hip_reference_verify_workspace_bytes(400, 513, 65) == 2 * one


# ---- 2. refusals with fake pointers, no device ------------------------------------------------------------------------------
def test_null_pointers_are_refused(L):
    for name in ("ref", "offsets", "positions", "work"):
        assert build_dev(L, **{name: None}) == EINVAL, name
    for name in ("offsets", "positions", "reads", "counts"):
        assert count_dev(L, **{name: None}) == EINVAL, name
    for name in ("offsets", "positions", "reads", "counts", "prefix", "out_read", "out_window"):
        assert emit_dev(L, **{name: None}) == EINVAL, name
    for name in ("ref", "peq", "windows", "subjects", "distance"):
        assert verify_dev(L, **{name: None}) == EINVAL, name
    for name in ("segments", "scores", "hits"):
        assert select_dev(L, **{name: None}) == EINVAL, name


def test_seed_len_outside_1_to_13_is_refused(L):
    for q in (0, -3, 14):
        assert build_dev(L, q=q) == EINVAL and b"1..13" in L.bgsa_hip_last_error()
        assert count_dev(L, q=q) == EINVAL and b"1..13" in L.bgsa_hip_last_error()
        assert emit_dev(L, q=q) == EINVAL


def test_bad_shapes_are_refused(L):
    for ref_len, W, S in ((1000, 64, 0), (1000, 64, 65), (63, 64, 20), (0, 1, 1)):
        assert count_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
        assert emit_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
        assert verify_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
    assert build_dev(L, ref_len=-1) == EINVAL


def test_a_reference_beyond_int32_is_refused(L):
    big = INT32_MAX + 1
    assert build_dev(L, ref_len=big) == EINVAL and b"2^31" in L.bgsa_hip_last_error()
    assert count_dev(L, ref_len=big, W=400, S=239) == EINVAL and b"2^31" in L.bgsa_hip_last_error()
    assert emit_dev(L, ref_len=big, W=400, S=239) == EINVAL
    assert verify_dev(L, ref_len=big, W=400, S=239) == EINVAL
    assert count_dev(L, ref_len=2 ** 30 + 10, W=1, S=1, n=1, bound=0, q=1) == EINVAL and b"int32 window ids" in L.bgsa_hip_last_error()


def test_word_num_is_checked(L):
    assert verify_dev(L, n=1056, wn=33, W=2000, ref_len=5000, work=P, work_bytes=1 << 40) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()
    assert verify_dev(L, n=32, wn=2) == EINVAL and verify_dev(L, n=33, wn=1) == EINVAL and verify_dev(L, n=32, wn=0) == EINVAL
    assert verify_dev(L, read_count=63) == EINVAL and verify_dev(L, read_count=0) == EINVAL
    assert verify_dev(L, n=513, wn=17, W=600) == EINVAL and b"workspace" in L.bgsa_hip_last_error()       # column blocks need carries
    assert verify_dev(L, n=513, wn=17, W=600, work=P, work_bytes=100) == EINVAL


def test_negative_counts_are_refused_and_zero_counts_launch_nothing(L):
    assert count_dev(L, n_reads=-1) == EINVAL and emit_dev(L, n_reads=-1) == EINVAL
    assert verify_dev(L, n_pairs=-1) == EINVAL and select_dev(L, n_reads=-1) == EINVAL
    assert count_dev(L, cap=-1) == EINVAL and count_dev(L, bound=-1) == EINVAL and select_dev(L, bound=-1) == EINVAL
    assert emit_dev(L, base=-1) == EINVAL
    for k in (0, 65):
        assert select_dev(L, k=k) == EINVAL and b"1..64" in L.bgsa_hip_last_error()
    # nothing to do is fine once the checks pass: fake pointers, so a launch would fault
    assert count_dev(L, n_reads=0) == 0 and emit_dev(L, n_reads=0) == 0
    assert verify_dev(L, n_pairs=0) == 0 and select_dev(L, n_reads=0) == 0
    assert verify_dev(L, n=513, wn=17, W=600, n_pairs=0, work=P, work_bytes=1 << 20) == 0


def test_overlapping_seeds_are_refused_by_the_c_calls(L):
    assert count_dev(L, n=32, bound=4, q=7) == EINVAL and b"seed_len 7" in L.bgsa_hip_last_error()      # step = 6
    assert emit_dev(L, n=32, bound=4, q=7) == EINVAL
    assert count_dev(L, n=32, bound=4, q=6, n_reads=0) == 0
    assert count_dev(L, n=32, bound=40, q=1) == EINVAL                                                      # B = n: step 0


# ---- 3. pieces and the seed rule --------------------------------------------------------------------------------------------
def test_pieces_are_disjoint_whenever_the_seed_rule_holds():
    checked = 0
    for n in list(range(1, 40)) + [150, 151, 512, 1024]:
        for bound in list(range(0, 14)) + [n - 1, n, n + 5]:
            if bound < 0:
                continue
            B_ = min(bound, n)
            step = n // (B_ + 1)
            for q in range(1, min(step, 13) + 1):
                assert B.seed_plan(n, bound, q) == (B_, step, q) == R.plan(n, bound, q)
                starts = R.piece_starts(n, B_)
                assert len(starts) == B_ + 1 and starts[0] == 0
                covered = np.zeros(n, dtype=np.int64)
                for o in starts:
                    assert o + q <= n
                    covered[o: o + q] += 1
                assert covered.max() == 1
                checked += 1
            if step + 1 <= 13:
                assert R.plan(n, bound, step + 1) is None
                with pytest.raises(B.BgsaHipError):
                    B.seed_plan(n, bound, step + 1)
    assert checked > 2000


def test_default_seed_len():
    assert B.seed_plan(150, 12) == (12, 11, 11) == R.plan(150, 12)
    assert B.seed_plan(150, 3) == (3, 37, 12) == R.plan(150, 3)
    assert B.seed_plan(32, 4) == (4, 6, 6)
    with pytest.raises(B.BgsaHipError, match="allows no seed"):
        B.seed_plan(32, 32)             # B = n: step 0, not even a seed of 1 bp


def test_the_refusal_names_the_right_limits():
    with pytest.raises(B.BgsaHipError, match=r"rc=-1.*seed_len 7 allows max_distance <= 3; max_distance 4 allows seed_len <= 6"):
        B.seed_plan(32, 4, 7)
    assert B.seed_plan(32, 3, 7) == (3, 8, 7) and B.seed_plan(32, 4, 6) == (4, 6, 6)      # both limits are attained
    with pytest.raises(B.BgsaHipError, match=r"seed_len 12 allows max_distance <= 11; max_distance 12 allows seed_len <= 11"):
        B.seed_plan(150, 12, 12)
    assert B.seed_plan(150, 11, 12) == (11, 12, 12) and B.seed_plan(150, 12, 11) == (12, 11, 11)
    with pytest.raises(B.BgsaHipError, match=r"no bound allows seed_len 13; max_distance 0 allows seed_len <= 12"):
        B.seed_plan(12, 0, 13)
    with pytest.raises(B.BgsaHipError, match="1..13"):
        B.seed_plan(200, 2, 14)


# ---- 4. the index restated --------------------------------------------------------------------------------------------------
def test_helper_index_on_a_tiny_reference():
    codes = classes(np.frombuffer(b"ACGTNACGA", np.uint8))
    offsets, positions = R.index(codes, 2)
    assert offsets.size == 17 and offsets[-1] == 6                      # AC CG GT | AC CG GA: the two k-mers over the N are left out
    assert positions[offsets[1]: offsets[2]].tolist() == [0, 5]          # AC = 0 * 4 + 1
    assert positions[offsets[6]: offsets[7]].tolist() == [1, 6]          # CG = 1 * 4 + 2
    assert positions[offsets[11]: offsets[12]].tolist() == [2]           # GT = 2 * 4 + 3
    assert positions[offsets[8]: offsets[9]].tolist() == [7]             # GA
    assert R.index(codes[:1], 2)[0].tolist() == [0] * 17                 # L < q: empty
    assert R.SEED_LEN_MAX == B.reference.SEED_LEN_MAX == 13


# ---- 5. flags ---------------------------------------------------------------------------------------------------------------
def test_an_n_in_a_piece_is_flagged_and_an_n_outside_every_piece_is_not():
    n, bound, q = 32, 4, 5
    assert B.seed_plan(n, bound, q) == (4, 6, 5)       # step 6: pieces at 0, 6, 12, 18, 24, five long: position 5, 11, ... 29 .. 31 lie in no piece
    read = np.frombuffer(b"ACGT" * 8, np.uint8).copy()
    assert not R.has_n_piece(read, bound, q)
    for at in range(n):
        one = read.copy()
        one[at] = ord("N")
        forward = any(o <= at < o + q for o in R.piece_starts(n, bound))
        reverse = any(o <= n - 1 - at < o + q for o in R.piece_starts(n, bound))
        assert R.has_n_piece(one, bound, q, both_strands=False) == forward, at
        assert R.has_n_piece(one, bound, q) == (forward or reverse), at
    one = read.copy()
    one[5] = ord("N")                       # in no forward piece; on the reverse strand it is character 26, inside the piece at 24
    assert not R.has_n_piece(one, bound, q, both_strands=False) and R.has_n_piece(one, bound, q)
    one = read.copy()
    one[30] = ord("N")                      # forward: behind the last piece; reverse: character 1, inside the piece at 0
    assert not R.has_n_piece(one, bound, q, both_strands=False) and R.has_n_piece(one, bound, q)
    q = 1                                   # with seeds of 1 bp most of the read is outside every piece, on both strands
    one = read.copy()
    one[[2, 3, 4, 8, 15, 27]] = ord("N")    # forward pieces 0 6 12 18 24, reverse pieces cover 31 25 19 13 7
    assert not R.has_n_piece(one, bound, q)
    assert R.count_or_flag([1, 2, 3], True, 100) == -1 and R.count_or_flag([1, 2, 3], False, 2) == -2
    assert R.count_or_flag([1, 2, 3], False, 3) == 3 and R.count_or_flag([], False, 0) == 0


# ---- 6. completeness of the candidate rule against brute force -------------------------------------------------------------
def test_no_window_within_the_bound_is_missing_from_the_candidates():
    rng = np.random.default_rng(20261019)
    shapes = within = windows_seen = 0
    anchored = reverse_found = 0
    while shapes < 220:
        letters = np.frombuffer(b"ACGT" if shapes % 2 else b"AC", np.uint8)
        L_ = int(rng.integers(80, 161))
        n = int(rng.integers(12, 25))
        bound = int(rng.integers(0, 4))
        step = n // (bound + 1)
        q = int(rng.integers(2, min(step, 13) + 1))
        W = int(rng.integers(n + bound, min(L_, n + bound + 30) + 1))
        S = int(rng.integers(1, min(W, M.largest_stride(W, n, bound)) + 1))
        ref = letters[rng.integers(letters.size, size=L_)].copy()
        n_windows = M.window_count(L_, W, S)
        buckets = R.buckets_of(classes(ref), q)
        assert B.seed_plan(n, bound, q) == (bound, step, q) == R.plan(n, bound, q)
        shapes += 1
        anchored += (L_ - W) % S != 0
        for kind in range(3):
            begin = L_ - n - 3 if kind == 2 else int(rng.integers(0, L_ - n - 3))       # kind 2: at the end, in the anchored last window
            src = _edit(rng, list(ref[begin: begin + n + 3]), int(rng.integers(0, bound + 1)), letters)
            read = np.array(src[:n], np.uint8)
            if kind == 1:
                read = M.reverse_complement(read)
            assert read.size == n
            distances = R.window_distances(ref, W, S, read)
            assert distances.size == 2 * n_windows
            cands = set(R.candidates(lambda value: buckets.get(value, ()), L_, W, S, read, bound, q))
            assert all(0 <= g < 2 * n_windows for g in cands)
            near = np.flatnonzero(distances <= bound)
            missing = [int(g) for g in near if int(g) not in cands]
            assert not missing, (L_, W, S, n, bound, q, kind, missing)
            within += near.size
            windows_seen += distances.size
            reverse_found += int((near >= n_windows).sum())
    assert within >= 500, within            # the test cannot pass vacuously
    assert windows_seen > 10000 and anchored > 50 and reverse_found > 100


def test_the_rule_leaves_windows_out():
    """The filter filters: on a 4-letter reference most windows are no candidate of a read.  Ten pieces of 6 bp meet about
    10 * 2995 / 4096 = 7 chance occurrences, each inside two or three windows, besides the read's own locus: far fewer than half of
    the 124 ids."""
    rng = np.random.default_rng(7)
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(4, size=3000)]
    read = ref[1000:1032].copy()
    assert B.seed_plan(32, 4) == (4, 6, 6)
    offsets, positions = R.index(classes(ref), 6)
    cands = R.deduplicate(R.candidates(R.lookup_of(offsets, positions), 3000, 96, 48, read, 4, 6))
    n_windows = M.window_count(3000, 96, 48)
    assert 1 <= len(cands) < n_windows
    assert set(cands) >= {g for g in range(n_windows) if M.window_start(3000, 96, 48, g) <= 1000 - 4 and 1032 + 4 <= M.window_start(3000, 96, 48, g) + 96}


# ---- 7. selection and blanking restated -------------------------------------------------------------------------------------
def test_helper_select_and_blank():
    scores, windows = R.select([3, 5, 9, 11, 20], [2, 0, 7, 0, 2], 4, 3)
    assert scores.tolist() == [0, 0, -2] and windows.tolist() == [5, 11, 3]
    scores, windows = R.select([3, 5], [9, 1], 4, 3)
    assert scores.tolist() == [-1, R.INT32_MIN, R.INT32_MIN] and windows.tolist() == [5, -1, -1]
    hits = dict(scores=np.array([[0, -3, -9]], np.int32), windows=np.array([[4, 7, 8]], np.int32), strand=np.array([[0, 1, 0]], np.int32),
                ref_begin=np.array([[10, 20, -1]], np.int64), ref_end=np.array([[42, 52, -1]], np.int64), keep=np.array([[1, 1, 0]], np.int32),
                cigars=[["32=", "29=3X", None]])
    out = R.blank(hits, 2)
    assert out["scores"].tolist() == [[0, R.INT32_MIN, R.INT32_MIN]] and out["windows"].tolist() == [[4, -1, -1]]
    assert out["strand"].tolist() == [[0, -1, -1]] and out["ref_begin"].tolist() == [[10, -1, -1]] and out["keep"].tolist() == [[1, 0, 0]]
    assert out["cigars"] == [["32=", None, None]]
    same = B.blank_beyond(B.ReferenceHits(hits["scores"], hits["strand"], hits["ref_begin"], hits["ref_end"], hits["keep"], hits["cigars"],
                                          hits["windows"]), 2)
    for name in ("scores", "windows", "strand", "ref_begin", "ref_end", "keep"):
        assert np.array_equal(getattr(same, name), out[name]) and getattr(same, name).dtype == out[name].dtype
    assert same.cigars == out["cigars"]


# ---- 8. the driver without a device -----------------------------------------------------------------------------------------
def test_the_python_driver_refuses_without_a_device(monkeypatch):
    import torch
    assert callable(B.ReferenceMapper.map_reads_seeded)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(B.BgsaHipError, match="no GPU visible"):       # no CPU fallback: without a device there is no mapper to call
        B.ReferenceMapper(b"ACGT" * 100, 64, 20)

"""A reference as the query set, without a GPU: the four new symbols in the header and in both library flavours, the host-only
geometry calls against window_plan, the C ABI's refusals (they come before any HIP call, so fake pointers do), and the helper
tests/reference_map_reference.py checked against itself."""
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
from align_reference import classes  # noqa: E402

EINVAL = -1
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
INT32_MAX = 2 ** 31 - 1
SYMBOLS = ("bgsa_hip_reference_window_count", "bgsa_hip_reference_window_start", "bgsa_hip_reference_windows_dev",
           "bgsa_hip_reference_placements_dev")
SMALL = [(1000, 64, 40), (64, 64, 1), (65, 64, 64), (1000, 33, 1)]
LARGE = (10 ** 9, 400, 250)


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


def windows_dev(L, ref=P, ref_len=1000, W=64, S=40, ids=None, first=0, n_rows=1, content=P):
    return L.bgsa_hip_reference_windows_dev(ref, ref_len, W, S, ids, first, n_rows, content, None)


def placements_dev(L, ref_len=1000, W=64, S=40, hits=P, n_reads=1, k=3, span=P, n_ops=P, cigar=P, cap=8, outs=(P, P, P, P)):
    return L.bgsa_hip_reference_placements_dev(ref_len, W, S, hits, n_reads, k, span, n_ops, cigar, cap, *outs, None)


# ---- 1. symbols -------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_and_exported_by_both_flavours(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared, name
            assert hasattr(flavour, name), (path.name, name)
    for name in ("ReferenceMapper", "window_plan", "max_stride"):
        assert hasattr(B, name)
    assert hasattr(B.DeviceAligner, "set_query_rows_device")


# ---- 2. geometry ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SMALL)
def test_geometry_calls_equal_window_plan_on_every_window(L, shape):
    ref_len, W, S = shape
    n, starts = B.window_plan(ref_len, W, S)
    assert L.bgsa_hip_reference_window_count(ref_len, W, S) == n == M.window_count(ref_len, W, S)
    got = [L.bgsa_hip_reference_window_start(ref_len, W, S, w) for w in range(n)]
    assert got == starts.tolist() == [M.window_start(ref_len, W, S, w) for w in range(n)]
    assert starts[0] == 0 and starts[-1] == ref_len - W and (np.diff(starts) <= S).all()
    assert L.bgsa_hip_reference_window_start(ref_len, W, S, n) == -1 and L.bgsa_hip_reference_window_start(ref_len, W, S, -1) == -1


def test_geometry_calls_equal_window_plan_on_a_large_reference(L):
    ref_len, W, S = LARGE
    n, starts = B.window_plan(ref_len, W, S)
    assert n == 1 + -(-(ref_len - W) // S) == L.bgsa_hip_reference_window_count(ref_len, W, S)
    for w in (0, 1, n - 2, n - 1):
        assert L.bgsa_hip_reference_window_start(ref_len, W, S, w) == int(starts[w]) == min(w * S, ref_len - W)


def test_anchored_last_window():
    n, starts = B.window_plan(1000, 64, 40)      # 936 = 23.4 strides: the last window is anchored, not on the stride's grid
    assert n == 25 and starts[-2] == 920 and starts[-1] == 936
    n, starts = B.window_plan(65, 64, 64)
    assert n == 2 and starts.tolist() == [0, 1]


def test_bad_shapes_are_refused_everywhere(L):
    for ref_len, W, S in ((1000, 64, 0), (1000, 64, 65), (63, 64, 40), (0, 1, 1)):
        assert L.bgsa_hip_reference_window_count(ref_len, W, S) == -1
        assert L.bgsa_hip_last_error()
        assert L.bgsa_hip_reference_window_start(ref_len, W, S, 0) == -1
        assert windows_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
        assert placements_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
        with pytest.raises(B.BgsaHipError):
            B.window_plan(ref_len, W, S)


# ---- 3. refusals with fake pointers, no device ------------------------------------------------------------------------------
def test_window_ids_must_fit_int32(L):
    ref_len = 2 ** 30 + 10        # W = S = 1: n_windows = L, and 2 n_windows > INT32_MAX
    assert L.bgsa_hip_reference_window_count(ref_len, 1, 1) == ref_len
    assert windows_dev(L, ref_len=ref_len, W=1, S=1) == EINVAL and b"int32" in L.bgsa_hip_last_error()
    assert placements_dev(L, ref_len=ref_len, W=1, S=1) == EINVAL
    assert windows_dev(L, ref_len=(INT32_MAX - 1) // 2, W=1, S=1, n_rows=0) == 0     # 2 n_windows = INT32_MAX - 1 fits


def test_windows_call_refusals(L):
    assert windows_dev(L, ref=None) == EINVAL
    assert windows_dev(L, content=None) == EINVAL
    n = B.window_plan(1000, 64, 40)[0]
    assert windows_dev(L, first=-1) == EINVAL
    assert windows_dev(L, first=2 * n, n_rows=1) == EINVAL
    assert windows_dev(L, first=n, n_rows=n + 1) == EINVAL
    assert windows_dev(L, first=0, n_rows=2 * n + 1) == EINVAL
    assert windows_dev(L, n_rows=-1) == EINVAL
    # nothing to do is fine once the checks pass, whatever the range's begin
    assert windows_dev(L, n_rows=0) == 0
    assert windows_dev(L, first=2 * n, n_rows=0) == 0
    assert windows_dev(L, ids=P, first=-5, n_rows=0) == 0      # first_id is ignored with an id list


def test_placements_call_refusals(L):
    for k in (0, -1, 65):
        assert placements_dev(L, k=k) == EINVAL and b"1..64" in L.bgsa_hip_last_error()
    assert placements_dev(L, hits=None) == EINVAL
    assert placements_dev(L, span=None) == EINVAL
    for i in range(4):
        outs = [P] * 4
        outs[i] = None
        assert placements_dev(L, outs=tuple(outs)) == EINVAL
    assert placements_dev(L, n_ops=None) == EINVAL         # the runs and their counts come together
    assert placements_dev(L, cigar=None) == EINVAL
    assert placements_dev(L, cap=0) == EINVAL
    assert placements_dev(L, n_reads=-1) == EINVAL
    assert placements_dev(L, n_reads=0) == 0
    assert placements_dev(L, n_reads=0, k=64, n_ops=None, cigar=None, cap=0) == 0


# ---- 4. the helper against itself --------------------------------------------------------------------------------------------
def random_reference(rng, length):
    return np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=length, p=[0.24, 0.24, 0.24, 0.24, 0.04])]


def test_reverse_window_of_the_reverse_complement_is_the_mirrored_forward_window():
    rng = np.random.default_rng(11)
    for ref_len, W, S in ((1000, 64, 40), (200, 33, 1), (64, 64, 1)):
        ref = classes(random_reference(rng, ref_len))
        rc = M.comp(ref[::-1])
        n = M.window_count(ref_len, W, S)
        rows_rc = M.window_rows(rc, W, S, range(2 * n))
        for w in range(n):
            at = M.window_start(ref_len, W, S, w)          # window w of rc covers rc[at, at + W) = the mirror of ref[L - at - W, L - at)
            mirror = ref[ref_len - at - W: ref_len - at]
            assert np.array_equal(rows_rc[n + w], mirror)
            assert np.array_equal(rows_rc[w], M.comp(mirror[::-1]))
    assert np.array_equal(M.window_rows(ref, W, S, [-1, 2 * n]), np.full((2, W), 4))


def test_reverse_spans_read_the_forward_reference():
    rng = np.random.default_rng(12)
    ref_len, W, S = 500, 64, 40
    ref = classes(random_reference(rng, ref_len))
    n = M.window_count(ref_len, W, S)
    rows = M.window_rows(ref, W, S, range(2 * n))
    for _ in range(200):
        w = int(rng.integers(n))
        qb = int(rng.integers(0, W + 1))
        qe = int(rng.integers(qb, W + 1))
        hits = np.array([[n + w, w]], dtype=np.int32)
        span = np.array([[qb, qe, 0, 9], [qb, qe, 0, 9]], dtype=np.int32)
        strand, begin, end, keep, _ = M.placements(ref_len, W, S, hits, span, np.zeros(2, np.int32), np.zeros((2, 1), np.int32), 1)
        assert strand.tolist() == [[1, 0]]
        # the reverse window's [qb, qe), read backwards, is the complement of the forward reference over [ref_begin, ref_end)
        assert np.array_equal(rows[n + w][qb:qe][::-1], M.comp(ref[begin[0, 0]: end[0, 0]]))
        assert np.array_equal(rows[w][qb:qe], ref[begin[0, 1]: end[0, 1]])
        assert end[0, 0] - begin[0, 0] == qe - qb == end[0, 1] - begin[0, 1]


def test_reverse_complement_of_ascii_goes_through_the_codes():
    assert bytes(M.reverse_complement(np.frombuffer(b"AACGTNx", np.uint8))) == b"TNACGTT"


@pytest.mark.parametrize("W,n,B_", [(96, 32, 4), (64, 20, 0), (50, 20, 20), (40, 39, 1)])
def test_max_stride_is_exact(W, n, B_):
    ref_len, length = 300, n + min(B_, n)
    S = B.max_stride(W, n, B_)
    assert S == M.largest_stride(W, n, B_) >= 1

    def uncovered(stride):
        starts = B.window_plan(ref_len, W, stride)[1]
        return [x for x in range(ref_len - length + 1) if not ((starts <= x) & (x + length <= starts + W)).any()]
    assert uncovered(S) == []
    if S + 1 <= W:
        assert uncovered(S + 1)
    assert B.max_stride(96, 32, 4) == 61 and B.max_stride(96, 32, 1000) == 33 and B.max_stride(40, 39, 5) < 1


def test_keep_on_hand_made_lists():
    k = M.keep_of
    assert k([0, 0], [100, 110], [132, 142]).tolist() == [1, 0]            # same strand, overlapping: the better view only
    assert k([0, 0], [100, 132], [132, 164]).tolist() == [1, 1]            # same strand, touching is disjoint (half-open)
    assert k([0, 1], [100, 110], [132, 142]).tolist() == [1, 1]            # opposite strands never hide each other
    assert k([0, 0, 0], [100, -1, 120], [132, -1, 150]).tolist() == [1, 0, 0]   # an unplaced hit between two views of one locus
    assert k([1, 1, 1], [100, 120, 140], [132, 150, 170]).tolist() == [1, 0, 1]  # a hidden hit hides nobody
    assert k([-1, 0], [-1, 5], [-1, 9]).tolist() == [0, 1]


def test_runs_are_reversed_within_their_count_only():
    row = np.array([1, 2, 3, 4, 5])
    assert M.reverse_runs(3, row, 5).tolist() == [3, 2, 1, 4, 5]
    assert M.reverse_runs(6, row, 5).tolist() == [1, 2, 3, 4, 5]           # an overflowing row is left untouched
    assert M.reverse_runs(0, row, 5).tolist() == [1, 2, 3, 4, 5]


def test_host_pipeline_finds_reads_of_both_strands_where_they_were_taken():
    rng = np.random.default_rng(13)
    ref = random_reference(rng, 400)
    ref[ref == ord("N")] = ord("A")
    W, S, n = 64, 30, 24
    reads = np.stack([ref[50:74], M.reverse_complement(ref[200:224]), ref[376:400]])
    got = M.map_reads_host(ref, W, S, reads, k_best=1, max_distance=2)
    assert got["scores"][:, 0].tolist() == [0, 0, 0]
    assert got["strand"][:, 0].tolist() == [0, 1, 0]
    assert got["ref_begin"][:, 0].tolist() == [50, 200, 376] and got["ref_end"][:, 0].tolist() == [74, 224, 400]
    assert [c[0] for c in got["cigars"]] == ["24="] * 3
    for c in range(3):      # every other kept hit is another locus
        kept = np.flatnonzero(got["keep"][c])
        assert kept[0] == 0
        for r in kept[1:]:
            assert got["strand"][c, r] != got["strand"][c, 0] or got["ref_end"][c, r] <= got["ref_begin"][c, 0] or \
                got["ref_begin"][c, r] >= got["ref_end"][c, 0]


def test_python_driver_refuses_without_a_device():
    with pytest.raises(B.BgsaHipError, match="rc=-1"):
        B.window_plan(10, 20, 5)

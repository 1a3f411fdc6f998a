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


# ---- 8. the host side of the four map_reads entry points (bgsa_amd/reference.py), no device ----------------------------------
from bgsa_amd import reference as RM  # noqa: E402

WHO = ("map_reads", "map_reads_ragged", "map_reads_seeded", "map_reads_seeded_ragged")
# every refusal, word for word as the four methods raised them before they shared check_call (geometry: see refuse())
REFUSALS = {
    "map_reads": {
        "k_best": "map_reads: rc=-1: k_best must lie in 1..64",
        "negative": "map_reads: rc=-1: max_distance is negative",
        "stride": "map_reads: rc=-1: at stride 62 a placement of a 32 bp read within distance 4 can lie in no window of 96 bp: "
                  "the largest stride allowed is 61",
        "no_stride": "map_reads: rc=-1: at stride 1 a placement of a 32 bp read within distance 4 can lie in no window of 34 bp: "
                     "no stride is (a longer window)",
        "cigar_cap": "map_reads: rc=-1: cigar_cap is not positive",
    },
    "map_reads_ragged": {
        "1024": "map_reads_ragged: rc=-2: reads beyond 1,024 bp have no per-lane form (one length per call: map_reads)",
        "k_best": "map_reads_ragged: rc=-1: k_best must lie in 1..64",
        "negative": "map_reads_ragged: rc=-1: max_distance is negative",
        "stride": "map_reads_ragged: rc=-1: at stride 62 a placement of the longest read (32 bp) within distance 4 can lie in no window "
                  "of 96 bp: the largest stride allowed is 61",
        "no_stride": "map_reads_ragged: rc=-1: at stride 1 a placement of the longest read (32 bp) within distance 4 can lie in no window "
                     "of 34 bp: no stride is (a longer window)",
        "cigar_cap": "map_reads_ragged: rc=-1: cigar_cap is not positive",
    },
    "map_reads_seeded": {
        "1024": "map_reads_seeded: rc=-2: reads beyond 1,024 bp have no verify kernel (map_reads takes them)",
        "k_best": "map_reads_seeded: rc=-1: k_best must lie in 1..64",
        "required": "map_reads_seeded: rc=-1: max_distance is required: the seed filter is derived from it (map_reads takes "
                    "max_distance=None)",
        "negative": "map_reads_seeded: rc=-1: max_distance is negative",
        "seed_plan": "seed_plan: rc=-1: the 5 pieces of a 32 bp read within distance 4 start 6 bp apart, too close for seeds of 7 bp: "
                     "seed_len 7 allows max_distance <= 3; max_distance 4 allows seed_len <= 6",
        "stride": "map_reads_seeded: rc=-1: at stride 62 a placement of a 32 bp read within distance 4 can lie in no window of 96 bp: "
                  "the largest stride allowed is 61",
        "no_stride": "map_reads_seeded: rc=-1: at stride 1 a placement of a 32 bp read within distance 4 can lie in no window of 34 bp: "
                     "no stride is (a longer window)",
        "int32": "map_reads_seeded: rc=-1: the index holds int32 positions: a reference beyond 2^31 - 1 bases goes in parts",
        "cigar_cap": "map_reads_seeded: rc=-1: cigar_cap is not positive",
        "max_candidates": "map_reads_seeded: rc=-1: max_candidates is negative",
    },
    "map_reads_seeded_ragged": {
        "1024": "map_reads_seeded_ragged: rc=-2: reads beyond 1,024 bp have no per-lane form (one length per call: map_reads)",
        "k_best": "map_reads_seeded_ragged: rc=-1: k_best must lie in 1..64",
        "required": "map_reads_seeded_ragged: rc=-1: max_distance is required: the seed filter is derived from it (map_reads_ragged "
                    "takes max_distance=None)",
        "negative": "map_reads_seeded_ragged: rc=-1: max_distance is negative",
        "seed_plan": "seed_plan_ragged: rc=-1: seed_len must lie in 1..13",
        "stride": "map_reads_seeded_ragged: rc=-1: at stride 62 a placement of the longest read (32 bp) within distance 4 can lie in no "
                  "window of 96 bp: the largest stride allowed is 61",
        "no_stride": "map_reads_seeded_ragged: rc=-1: at stride 1 a placement of the longest read (32 bp) within distance 4 can lie in no "
                     "window of 34 bp: no stride is (a longer window)",
        "int32": "map_reads_seeded_ragged: rc=-1: the index holds int32 positions: a reference beyond 2^31 - 1 bases goes in parts",
        "cigar_cap": "map_reads_seeded_ragged: rc=-1: cigar_cap is not positive",
        "max_candidates": "map_reads_seeded_ragged: rc=-1: max_candidates is negative",
    },
}
# what breaks each rule, in the order the rules are checked
BREAKS = [("1024", dict(longest=1025, W=1400)), ("k_best", dict(k_best=0)), ("required", dict(max_distance=None)),
          ("negative", dict(max_distance=-1)), ("seed_plan", None), ("stride", dict(S=62)), ("int32", dict(ref_len=2 ** 31)),
          ("cigar_cap", dict(cigar_cap=0)), ("max_candidates", dict(max_candidates=-1))]


def check_call(who, longest=32, k_best=1, max_distance=4, cigar_cap=None, max_candidates=None, W=96, S=48, ref_len=3000, n_ids=124,
               seed_len=None):
    """check_call as the entry point `who` calls it: 32 bp reads within 4 on the 3,000 bp case of the GPU tests (W 96, S 48)."""
    ragged, seeded = who.endswith("_ragged"), "_seeded" in who
    plan = None
    if seeded:
        lens = np.full(3, longest, np.int32)
        plan = (lambda limit: RM.seed_plan_ragged(lens, limit, seed_len)) if ragged else (lambda limit: RM.seed_plan(longest, limit, seed_len))
    return RM.check_call(who, longest, ragged, k_best, max_distance, seeded, cigar_cap, max_candidates, W, S, ref_len, n_ids,
                         who != "map_reads", plan)


def broken(who, rule):
    over = dict(BREAKS)[rule]
    if over is None:      # the seed plan: overlapping seeds for one length, a seed length outside 1..13 for a list
        over = dict(seed_len=14) if who.endswith("_ragged") else dict(seed_len=7)
    return over


@pytest.mark.parametrize("who", WHO)
def test_every_refusal_keeps_its_text(who):
    for rule, text in REFUSALS[who].items():
        over = dict(W=34, S=1) if rule == "no_stride" else broken(who, rule)
        with pytest.raises(B.BgsaHipError) as e:
            check_call(who, **over)
        assert str(e.value) == text, rule
    for k_best in (65, -1):
        with pytest.raises(B.BgsaHipError) as e:
            check_call(who, k_best=k_best)
        assert str(e.value) == REFUSALS[who]["k_best"]


@pytest.mark.parametrize("who", WHO)
def test_of_two_broken_rules_the_earlier_one_is_reported(who):
    rules = [rule for rule, _ in BREAKS if rule in REFUSALS[who]]
    for i, first in enumerate(rules):
        for second in rules[i + 1:]:
            over = {**broken(who, second), **broken(who, first)}
            if len(over) < len(broken(who, second)) + len(broken(who, first)):
                continue      # both rules are broken through the same argument: one call cannot break both
            if "W" in over and "S" in over:
                over["S"] = 1400      # beyond 1,024 bp the window is 1,400 bp: a stride that breaks the rule there too
            with pytest.raises(B.BgsaHipError) as e:
                check_call(who, **over)
            assert str(e.value) == REFUSALS[who][first], (first, second)


def test_only_map_reads_takes_a_read_beyond_1024_bp():
    assert check_call("map_reads", longest=1025, W=1400, S=100)[:3] == (1, 4, 1400 + 1025)
    for who in WHO[1:]:
        with pytest.raises(B.BgsaHipError, match="rc=-2"):
            check_call(who, longest=1025, W=1400, S=100)
        assert check_call(who, longest=1024, W=1400, S=100)[2] == 1400 + 1024


def test_max_distance_none_is_for_the_exhaustive_calls():
    for who in WHO[:2]:
        assert check_call(who, max_distance=None) == (1, 0, 96 + 32, None, None)          # the stride rule of an exact placement
        with pytest.raises(B.BgsaHipError, match="within distance 0 .*largest stride allowed is 65"):
            check_call(who, max_distance=None, S=66)
    for who in WHO[2:]:
        with pytest.raises(B.BgsaHipError, match="max_distance is required"):
            check_call(who, max_distance=None)


def test_what_an_accepted_call_returns():
    assert check_call("map_reads", k_best=3, max_distance=40, cigar_cap=9, S=33) == (3, 32, 9, None, None)    # the bound stops at the read
    assert check_call("map_reads_seeded") == (1, 4, 128, max(124 // 8, 256), (4, 6, 6))
    assert check_call("map_reads_seeded", n_ids=83_682)[3] == 83_682 // 8
    assert check_call("map_reads_seeded", max_candidates=0)[3] == 0
    k_best, bound, cap, max_candidates, plan = check_call("map_reads_seeded_ragged", k_best=64, n_ids=4000)
    assert (k_best, bound, cap, max_candidates) == (64, 4, 128, 500)
    assert [(idx.tolist(), q) for idx, q in plan] == [([0, 1, 2], 6)]


def test_cigars_are_decoded_into_the_callers_order():
    eq, x, i = 7, 8, 1                                                      # the BAM op codes
    keep = np.array([[1, 0], [0, 0], [0, 1]], np.int32)
    n_ops = np.array([[3, 2], [1, 0], [0, 1]], np.int32)                    # a count in a slot that is not kept is not looked at
    runs = np.zeros((3, 2, 4), np.uint32)
    runs[0, 0, :3] = [(5 << 4) | eq, (1 << 4) | x, (26 << 4) | eq]
    runs[0, 1, :2] = [(7 << 4) | i, (7 << 4) | i]
    runs[2, 1, :2] = [(32 << 4) | eq, (9 << 4) | x]                         # beyond its count: not part of the script
    idx = np.array([6, 2, 3])
    cigars = [[None, None] for _ in range(8)]
    cigars[5][1] = "kept"
    RM.decode_cigars("map_reads_ragged", keep, n_ops, runs, 4, idx, cigars)
    want = [[None, None] for _ in range(8)]
    want[6][0], want[3][1], want[5][1] = "5=1X26=", "32=", "kept"
    assert cigars == want
    n_ops[2, 1] = 5
    with pytest.raises(B.BgsaHipError) as e:
        RM.decode_cigars("map_reads_seeded_ragged", keep, n_ops, runs, 4, idx, [[None, None] for _ in range(8)])
    assert str(e.value) == "map_reads_seeded_ragged: hit 1 of read 3 has 5 runs, its row holds 4 (raise cigar_cap)"


def hand_made_hits(ns, k_sel, base):
    grid = base + np.arange(ns * k_sel).reshape(ns, k_sel)
    return B.ReferenceHits(grid.astype(np.int32), (grid + 1).astype(np.int32), (grid + 2).astype(np.int64), (grid + 3).astype(np.int64),
                           (grid + 4).astype(np.int32), [[f"{base}:{c}:{r}" for r in range(k_sel)] for c in range(ns)],
                           (grid + 5).astype(np.int32))


def test_the_fallback_lands_in_its_rows_and_nowhere_else():
    out, before, full = hand_made_hits(6, 2, 0), hand_made_hits(6, 2, 0), hand_made_hits(2, 2, 1000)
    RM.merge_fallback(out, np.array([4, 1]), full)
    for name in B.ReferenceHits._fields:
        got, old, new = getattr(out, name), getattr(before, name), getattr(full, name)
        for c in range(6):
            want = new[[4, 1].index(c)] if c in (4, 1) else old[c]
            assert np.array_equal(got[c], want), (name, c)
        if name != "cigars":
            assert got.dtype == old.dtype


def test_seed_stats_has_the_two_key_sets():
    flags = np.array([5, 0, -1, -2, -2, -3, 17], np.int32)
    one = RM.seed_stats(flags, (40, 30, 7), 6, 256)
    assert one == dict(reads_seeded=3, reads_fallback_n=1, reads_fallback_cap=2, candidates_emitted=40, candidates_unique=30,
                       candidates_within_bound=7, seed_len=6, max_candidates=256)
    assert all(type(v) is int for v in one.values())
    bins = [dict(words=1, reads=7, q=6, emitted=40, unique=30)]
    for seed_len in (None, 6):
        mixed = RM.seed_stats(flags, [40, 30, 7], seed_len, 256, bins)
        assert mixed == dict(reads_seeded=3, reads_fallback_n=1, reads_fallback_cap=2, reads_fallback_short=1, candidates_emitted=40,
                             candidates_unique=30, candidates_within_bound=7, seed_len=seed_len, max_candidates=256, bins=bins)

"""Band-limited pair alignment on the MI355X: bgsa_hip_myers_align_pairs_banded_dev through DeviceAligner.align_pairs_banded /
align_hits_banded — within max_distance every distance, run count and run EXACTLY as the canonical traceback of
tests/align_reference.py, beyond it -2 / 0 and an untouched cigar row; subjects beyond 1,024 bp included."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import banded_align_reference as R  # noqa: E402
import bgsa_amd as B  # noqa: E402
from oracle import band_edge as E  # noqa: E402
from test_align_pairs_gpu import SENT, _aligner, _np, _sentinels, assert_pairs_exact, shape_case  # noqa: E402

pytestmark = pytest.mark.gpu

BEYOND = -2
FAULT_PAIR = 4
MAX_WORDS = 32   # kBandTraceMaxWords


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def assert_banded_exact(got, want, bound, cap, queries=None, subjects=None, scores=None, what=""):
    """want = [(distance, runs)] canonical, or None for a pair that must hold sentinels.  A pair with distance <= bound must
    be exact; any other owned pair holds BEYOND / 0 and a cigar row of sentinels."""
    distance, n_ops, cigar = got
    cigar = cigar.view(np.uint32)
    inside = [w is None or w[0] <= bound for w in want]
    for p, w in enumerate(want):
        if not inside[p]:
            assert distance[p] == BEYOND and n_ops[p] == 0, f"pair {p}: D = {w[0]} > {bound} came out as {distance[p]} / {n_ops[p]} {what}"
            assert (cigar[p] == SENT).all(), f"pair {p}: beyond the bound, but its cigar row was written {what}"
    keep = [p for p, ok in enumerate(inside) if ok]
    assert_pairs_exact((distance[keep], n_ops[keep], cigar[keep]), [want[p] for p in keep], cap,
                       None if queries is None else queries[keep], None if subjects is None else subjects[keep],
                       None if scores is None else np.asarray(scores)[keep], f"(B = {bound}) {what}")


def _diag_scores(a, pairs):
    return a.score().cpu().numpy()[np.arange(pairs), np.arange(pairs)]


# ---- block and word edges ---------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(31, 31), (32, 32), (33, 32), (64, 65), (65, 64), (96, 97), (150, 140), (40, 150), (150, 40)]


@pytest.mark.parametrize("m,n", EDGE_SHAPES)
def test_block_and_word_edges(torch_gpu, m, n):
    torch = torch_gpu
    L = B.lib()
    q, s, want = shape_case(m, n)
    pairs = q.shape[0]
    a = _aligner(q, s)
    idx = torch.arange(pairs, device="cuda")
    cap = m + n
    scores = _diag_scores(a, pairs)
    delta = abs(n - m)
    for bound in (delta, delta + 1, 31, 32, 33, m + n):
        got = _np(a.align_pairs_banded(idx, idx, bound, into=_sentinels(torch, pairs, cap)))
        assert_banded_exact(got, want, bound, cap, q, s, scores, f"(shape {m} x {n})")
        assert (L.bgsa_hip_align_pairs_band_words(m, n, bound) == 0) == (bound < delta)
    a.check_faults()
    assert L.bgsa_hip_align_pairs_band_words(m, n, m + n) == a.wn                 # the last bound: the window is the whole subject
    assert sum(d <= 33 for d, _ in want) > 10 or delta > 33


# ---- the certificate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,h", [(150, 150, 8), (150, 140, 10), (140, 150, 10), (200, 203, 16)])
def test_certificate_on_the_band_edge_ladders(torch_gpu, m, n, h):
    torch = torch_gpu
    q = E.seeded_runs_query(m, 31 * m + n)
    s, _ = E.band_edge_pairs(q, n, h)
    pairs = len(s)
    assert pairs <= 200
    qq = np.repeat(q[None, :], pairs, axis=0)
    want = A.canonical(qq, s)
    bound = 2 * h + 1
    at, above = [p for p, (d, _) in enumerate(want) if d == bound], [p for p, (d, _) in enumerate(want) if d == bound + 1]
    assert at and above, "the ladders hold no pair at B or at B + 1"
    a = _aligner(q[None, :], s)
    scores = a.score().cpu().numpy()[0, :pairs]
    pq, ps = np.zeros(pairs, dtype=np.int64), np.arange(pairs)
    cap = m + n
    for b in (bound - 1, bound, bound + 1):
        got = _np(a.align_pairs_banded(pq, ps, b, into=_sentinels(torch, pairs, cap)))
        assert_banded_exact(got, want, b, cap, qq, s, scores, f"(ladder {m} x {n})")
        if b == bound:
            assert (got[0][at] == bound).all() and (got[1][at] > 0).all()            # D == B is traced
            assert (got[0][above] == BEYOND).all() and (got[1][above] == 0).all()    # D == B + 1 is not
    a.check_faults()


# ---- agreement with the existing kernel -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n,bound", [(150, 150, 12), (150, 150, 300), (1000, 1024, 30), (1000, 1024, 64)])
def test_pairs_within_the_bound_equal_align_pairs_bit_for_bit(torch_gpu, m, n, bound):
    torch = torch_gpu
    q, s, want = shape_case(m, n)
    pairs = q.shape[0]
    a = _aligner(q, s)
    idx = torch.arange(pairs, device="cuda")
    cap = m + n
    full = _np(a.align_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    band = _np(a.align_pairs_banded(idx, idx, bound, into=_sentinels(torch, pairs, cap)))
    a.check_faults()
    inside = full[0] <= bound
    assert inside.any() and (bound >= m + n or not inside.all())
    for x, y in zip(full, band):
        assert x[inside].tobytes() == y[inside].tobytes()
    assert (band[0][~inside] == BEYOND).all() and (band[1][~inside] == 0).all() and (band[2][~inside] == SENT).all()


# ---- beyond 32 words ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_case(m, n, edits):
    """Mutated copies cut to (m, n): pair p carries edits[p] random edits on top of the |n - m| the lengths force."""
    import oracle as O
    seed = 15485863 * m + n
    longest = max(m, n)
    base = O.gen_reads(seed, len(edits), longest)
    mutants = O.mutate(base, list(edits), seed + 1)
    q, s = np.ascontiguousarray(base[:, :m]), np.ascontiguousarray(mutants[:, :n])
    q.setflags(write=False)
    s.setflags(write=False)
    return q, s, A.canonical(q, s)


@pytest.mark.parametrize("m,n,bound,edits", [(1056, 1056, 40, (0, 1, 3, 9, 17, 25, 33, 60)),
                                             (1100, 1025, 100, (0, 1, 4, 8, 12, 20, 30, 120)), (1100, 1025, 140, (0, 1, 4, 8, 12, 20, 30, 120)),
                                             (1025, 1100, 100, (0, 1, 4, 8, 12, 20, 30, 120)), (1025, 1100, 140, (0, 1, 4, 8, 12, 20, 30, 120)),
                                             (2100, 2080, 64, (0, 6, 25, 70))])
def test_subjects_beyond_1024_bp(torch_gpu, m, n, bound, edits):
    torch = torch_gpu
    q, s, want = long_case(m, n, edits)
    pairs = q.shape[0]
    assert any(d <= bound for d, _ in want) and any(d > bound for d, _ in want)
    a = _aligner(q, s)
    assert a.wn > 32
    idx = torch.arange(pairs, device="cuda")
    cap = 400
    got = _np(a.align_pairs_banded(idx, idx, bound, cigar_cap=cap, into=_sentinels(torch, pairs, cap)))
    scores = _diag_scores(a, pairs)
    a.check_faults()
    assert_banded_exact(got, want, bound, cap, q, s, scores, f"(shape {m} x {n})")


def test_4000_bp_pairs_against_the_integer_model(torch_gpu, oracle):
    torch = torch_gpu
    m = n = 4000
    base = oracle.gen_reads(0xBA4D_4000, 2, m)
    q, s = base, oracle.mutate(base, [40, 37], 0xBA4D_4001)
    a = _aligner(q, s)
    assert a.wn == 125 and B.lib().bgsa_hip_align_pairs_band_words(m, n, 128) == 5
    cap = 600
    got = _np(a.align_pairs_banded([0, 1], [0, 1], 128, cigar_cap=cap, into=_sentinels(torch, 2, cap)))
    scores = _diag_scores(a, 2)
    a.check_faults()
    model = R.align_rows(q, s, 128)
    for p in range(2):
        dist, runs, width = model[p]
        assert width == 5 and dist is not None and 30 < dist <= 80
        assert got[0][p] == dist == -int(scores[p]) and got[1][p] == len(runs) <= cap
        assert A.unpack(got[2][p].view(np.uint32)[: len(runs)]) == runs
        assert (got[2][p, len(runs):] == SENT).all()
        A.validate(q[p], s[p], int(got[0][p]), runs)


# ---- the widest window ----------------------------------------------------------------------------------------------------------
def test_the_widest_instantiated_window_and_a_window_that_is_the_whole_subject(torch_gpu):
    torch = torch_gpu
    L = B.lib()
    # 1,116 bp = 35 words: the smallest bound whose window is 32 words, three short of the subject (equal lengths give odd widths only)
    q, s, want = long_case(1100, 1116, (0, 1, 3, 9, 17, 25, 33, 60))
    bound = next(b for b in range(2200) if L.bgsa_hip_align_pairs_band_words(1100, 1116, b) == MAX_WORDS)
    assert L.bgsa_hip_align_pairs_band_words(1100, 1116, bound - 1) == MAX_WORDS - 1 and max(d for d, _ in want) <= bound
    a = _aligner(q, s)
    assert a.wn == 35
    idx = torch.arange(8, device="cuda")
    got = _np(a.align_pairs_banded(idx, idx, bound, cigar_cap=400, into=_sentinels(torch, 8, 400)))
    a.check_faults()
    assert_banded_exact(got, want, bound, 400, q, s, what="(32 of 35 words)")
    # 1,000 x 1,024 bp at B = m + n: the window is all 32 words of every block
    q, s, want = shape_case(1000, 1024)
    assert L.bgsa_hip_align_pairs_band_words(1000, 1024, 2024) == MAX_WORDS == L.bgsa_hip_word_num(B.ALGO_MYERS, 1000, 1024, 0)
    a = _aligner(q, s)
    pairs = q.shape[0]
    idx = torch.arange(pairs, device="cuda")
    got = _np(a.align_pairs_banded(idx, idx, 2024, into=_sentinels(torch, pairs, 2024)))
    a.check_faults()
    assert_banded_exact(got, want, 2024, 2024, q, s, what="(the whole subject)")


# ---- chunks ---------------------------------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_workspace(torch_gpu):
    torch = torch_gpu
    L = B.lib()
    q, s, want = shape_case(96, 97)
    q, s, want = q[:130], s[:130], want[:130]
    bound = 14
    assert any(d > bound for d, _ in want) and sum(d <= bound for d, _ in want) > 64
    a = _aligner(q, s)
    idx = np.arange(130)
    small = int(L.bgsa_hip_align_pairs_banded_min_workspace_bytes(96, 97, bound))
    assert int(L.bgsa_hip_align_pairs_banded_workspace_bytes(96, 97, bound, 130)) == 3 * small       # three chunks of one wave
    cap = 193
    outs = [_np(a.align_pairs_banded(idx, idx, bound, into=_sentinels(torch, 130, cap), workspace_bytes=w)) for w in (small, 0, None)]
    a.check_faults()
    assert_banded_exact(outs[0], want, bound, cap, q, s, what="(minimum workspace)")
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert x.tobytes() == y.tobytes()
    with pytest.raises(B.BgsaHipError, match="rc=-1"):
        a.align_pairs_banded(idx, idx, bound, workspace_bytes=small - 256)


# ---- ownership ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes_case():
    """40 queries x 100 subjects of 70 x 75 bp, the bucket padded to 128; pair (i, j) is close when j % 40 == i."""
    import oracle as O
    q = O.gen_reads(601, 40, 70)
    s = np.concatenate([O.mutate(np.concatenate([q, q, q[:20]]), np.arange(100) % 9, 602), O.gen_reads(603, 100, 5)], axis=1)
    padded, _ = B.pad_rows(s)

    @functools.lru_cache(maxsize=None)
    def want(qi, sj):
        return A.canonical(q[qi][None, :], padded[sj][None, :])[0]
    return q, s, padded, want


BOUND = 20   # close pairs lie within it, unrelated ones (D ~ 40) beyond


def test_pairs_of_other_buckets_and_unused_slots_are_untouched(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    a = _aligner(q, s)
    base = 1000
    ps = np.array([base + 5, -1, base - 1, base + 128, base + 127, 5, base, -1, base + 128 + 5, 1 << 40, base + 46, base + 47])
    pq = np.array([5, 1, 2, 3, 4, 5, 0, 7, 8, 9, 6, 30])
    own = [True, False, False, False, True, False, True, False, False, False, True, True]
    cap = 145
    got = _np(a.align_pairs_banded(pq, ps, BOUND, subject_base=base, into=_sentinels(torch, len(ps), cap)))
    a.check_faults()
    wants = [want(int(i), int(j - base)) if o else None for i, j, o in zip(pq, ps, own)]
    assert wants[0][0] <= BOUND and wants[10][0] <= BOUND and wants[11][0] > BOUND and wants[4][0] > BOUND
    assert_banded_exact(got, wants, BOUND, cap)
    fresh = _np(a.align_pairs_banded(pq, ps, BOUND, subject_base=base))
    for p, o in enumerate(own):
        if not o:
            assert fresh[0][p] == -1 and fresh[1][p] == 0 and not fresh[2][p].any()
        else:
            assert fresh[0][p] == got[0][p] and fresh[1][p] == got[1][p]
    assert fresh[0][11] == BEYOND and not fresh[2][11].any()


def test_two_buckets_walked_with_into_equal_one_bucket(torch_gpu, lanes_case):
    q, s, padded, want = lanes_case
    rng = np.random.default_rng(9)
    pq = rng.integers(0, 40, 150)
    ps = np.where(rng.integers(0, 2, 150) == 0, pq + 40 * rng.integers(0, 2, 150), rng.integers(0, 100, 150))
    ps[::17] = -1
    whole = _aligner(q, s)
    one = _np(whole.align_pairs_banded(pq, ps, BOUND))
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    out = None
    for lo, hi in ((0, 64), (64, 100)):                 # the second bucket's last group is padded
        a.set_subjects(s[lo:hi])
        out = a.align_pairs_banded(pq, ps, BOUND, subject_base=lo, into=out)
    a.check_faults()
    for x, y in zip(one, _np(out)):
        assert x.tobytes() == y.tobytes()
    seen = set()
    for p, (i, j) in enumerate(zip(pq, ps)):
        if j < 0:
            assert one[0][p] == -1 and one[1][p] == 0
            continue
        d, runs = want(int(i), int(j))
        seen.add(d <= BOUND)
        if d <= BOUND:
            assert (one[0][p], one[1][p], A.unpack(one[2][p, : len(runs)])) == (d, len(runs), runs), p
        else:
            assert one[0][p] == BEYOND and one[1][p] == 0 and not one[2][p].any()
    assert seen == {True, False}


def test_a_query_index_out_of_range_touches_nothing_and_raises_the_pair_bit(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    L = B.lib()
    a = _aligner(q, s)
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == 0
    pq, ps = np.array([4, -1, 40, 7, 1 << 30]), np.array([44, 9, 9, 47, 11])
    got = _np(a.align_pairs_banded(pq, ps, BOUND, into=_sentinels(torch, 5, 145)))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == FAULT_PAIR and L.bgsa_hip_stream_faults(1) == 0
    assert_banded_exact(got, [want(4, 44), None, None, want(7, 47), None], BOUND, 145)
    assert got[0][0] >= 0 and got[0][3] >= 0
    # ... also where the lengths alone put every pair beyond the bound
    got = _np(a.align_pairs_banded(pq, ps, 4, into=_sentinels(torch, 5, 145)))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == FAULT_PAIR
    assert got[0].tolist() == [BEYOND, SENT, SENT, BEYOND, SENT] and got[1].tolist() == [0, SENT, SENT, 0, SENT] and (got[2] == SENT).all()


def test_a_cap_of_one_keeps_the_true_count_and_the_first_run(torch_gpu):
    torch = torch_gpu
    q, s, want = shape_case(150, 140)
    pairs = q.shape[0]
    a = _aligner(q, s)
    idx = np.arange(pairs)
    bound = 40
    assert max(len(runs) for d, runs in want if d <= bound) > 3
    dist, n_ops, _ = _sentinels(torch, pairs, 1)
    room = torch.full((pairs + 16,), SENT, dtype=torch.int32, device="cuda")     # the rows, and 16 slots behind the last one
    got = _np(a.align_pairs_banded(idx, idx, bound, cigar_cap=1, into=(dist, n_ops, room[:pairs].view(pairs, 1))))
    a.check_faults()
    assert (room[pairs:] == SENT).all()
    assert_banded_exact(got, want, bound, 1, what="(cap 1)")


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def test_align_hits_banded_shapes(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    a = _aligner(q, s)
    hit_scores, hit_subjects = a.top_hits(4)
    hit_subjects[::5, 3:] = -1
    distance, n_ops, cigar = a.align_hits_banded(hit_subjects, BOUND)
    a.check_faults()
    assert tuple(distance.shape) == (40, 4) and tuple(n_ops.shape) == (40, 4) and tuple(cigar.shape) == (40, 4, 145)
    assert distance.dtype == torch.int32 and n_ops.dtype == torch.int32 and cigar.dtype == torch.int32
    sc, sj, d, k, c = _np((hit_scores, hit_subjects, distance, n_ops, cigar))
    for i in range(40):
        for r in range(4):
            if sj[i, r] < 0:
                assert d[i, r] == -1 and k[i, r] == 0 and not c[i, r].any()
            elif -sc[i, r] <= BOUND:
                w = want(i, int(sj[i, r]))
                assert (d[i, r], k[i, r], A.unpack(c[i, r].view(np.uint32)[: k[i, r]])) == (w[0], len(w[1]), w[1]) and d[i, r] == -sc[i, r]
            else:
                assert d[i, r] == BEYOND and k[i, r] == 0 and not c[i, r].any()
    assert (d[:, 0] >= 0).all() and (d == BEYOND).any()
    again = a.align_hits_banded(hit_subjects, BOUND, into=(distance, n_ops, cigar))
    assert again[0].data_ptr() == distance.data_ptr()
    with pytest.raises(B.BgsaHipError):
        a.align_hits_banded(hit_subjects[:5], BOUND)
    with pytest.raises(B.BgsaHipError, match="rc=-1"):
        a.align_hits_banded(hit_subjects, -1)


def test_align_top_alignments_banded_on_1056_bp_reads(torch_gpu, oracle):
    q = oracle.gen_reads(0xBA4D_0001, 6, 1056)
    s = oracle.gen_reads(0xBA4D_1001, 300, 1056)
    for i in range(6):
        s[50 * i: 50 * i + 3] = oracle.mutate(np.repeat(q[i: i + 1], 3, axis=0), [0, 7, 21], 3000 + i)
    scores, subjects, cigars = B.align_top_alignments_banded(q, s, 3, cigar_cap=200)
    assert scores.shape == (6, 3) and subjects.shape == (6, 3)
    for i in range(6):
        assert sorted(subjects[i].tolist()) == [50 * i, 50 * i + 1, 50 * i + 2] and scores[i, 0] == 0 and cigars[i][0] == "1056="
        for r in range(3):
            A.validate(q[i], s[subjects[i, r]], -int(scores[i, r]), A.from_string(cigars[i][r]))
    want = A.canonical(q, s[subjects[:, 2]])
    assert [(-int(scores[i, 2]), A.from_string(cigars[i][2])) for i in range(6)] == want
    # a caller's own bound: the hits beyond it have no script
    _, subjects5, cigars5 = B.align_top_alignments_banded(q, s, 3, max_distance=10, cigar_cap=200)
    assert (subjects5 == subjects).all()
    for i in range(6):
        assert [c is not None for c in cigars5[i]] == [-int(x) <= 10 for x in scores[i]]
        assert cigars5[i][0] == "1056=" and cigars5[i][2] is None


@pytest.mark.parametrize("kind", ["semi_global", "bitpal", "banded", "plus_distance", "ragged"])
def test_other_aligners_and_ragged_buckets_are_refused_before_any_launch(torch_gpu, oracle, kind):
    q, s = oracle.gen_reads(71, 4, 150), oracle.gen_reads(72, 64, 150)
    kw = {"semi_global": dict(algo=B.ALGO_MYERS, semi_global=True), "bitpal": dict(algo=B.ALGO_BITPAL, scores=(2, -3, -5)),
          "banded": dict(algo=B.ALGO_BANDED, k=8), "plus_distance": dict(algo=B.ALGO_MYERS, scores=(0, 1, 1)),
          "ragged": dict(algo=B.ALGO_MYERS)}[kind]
    a = B.DeviceAligner(kw.pop("algo"), "cuda:0", **kw)
    a.set_queries(q)
    if kind == "ragged":
        a.set_subjects_ragged([row[: 150 - (i % 7)] for i, row in enumerate(s)])
    else:
        a.set_subjects(s)
    into = _sentinels(torch_gpu, 3, 300)
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.align_pairs_banded([0, 1, 2], [0, 1, 2], 300, into=into)
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.align_hits_banded(torch_gpu.zeros((4, 2), dtype=torch_gpu.int64, device="cuda"), 300)
    torch_gpu.cuda.synchronize()
    assert all((t == SENT).all() for t in into)


def test_a_bound_too_wide_for_the_kernels_is_refused_with_the_largest_one(torch_gpu, oracle):
    a = _aligner(oracle.gen_reads(1, 2, 4000), oracle.gen_reads(2, 64, 4000))
    with pytest.raises(B.BgsaHipError, match="max_distance <= 961"):
        a.align_pairs_banded([0], [0], 962)

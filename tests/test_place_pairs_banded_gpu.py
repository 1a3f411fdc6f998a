"""Band-limited semi-global placement on the MI355X: bgsa_hip_myers_place_pairs_banded_dev through
DeviceAligner.place_pairs_banded / place_hits_banded / place_top_queries_banded — bit for bit trace_pairs' score, span, run count
and runs where that call applies, the canonical walk of tests/trace_reference.py beyond 1,024 bp, every distance the score() of
the same aligner, the stream-fault word clean, and sentinel-filled outputs untouched wherever nothing is owned."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import place_reference as R  # noqa: E402
import trace_reference as T  # noqa: E402
from test_place_pairs_banded_cpu import _edit, make_pairs  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 12345          # what pre-filled outputs hold where nothing may be written
ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _aligner(q, s):
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _sentinels(torch, n, cap):
    def full(*shape):
        return torch.full(shape, SENT, dtype=torch.int32, device="cuda")
    return full(n), full(n, 4), full(n), full(n, cap)


def plant(rng, window, n, kind, edits, at=0, hang=5):
    """A read of n bp: a piece of `window` at `at` ("mid"), hanging `hang` bp off its start or its end, or unrelated; then
    `edits` random edits, cut or filled up to n."""
    m = window.size
    noise = list(ACGT[rng.integers(4, size=n)])
    if kind == "mid":
        src = list(window[at: at + n])
    elif kind == "start":
        src = noise[:hang] + list(window[: n - hang])
    elif kind == "end":
        src = list(window[m - n + hang:]) + noise[:hang]
    else:
        return np.array(noise, np.uint8)
    src = _edit(rng, src, edits, ACGT)
    return np.array((src + noise)[:n], np.uint8)


def assert_place_matches_trace(place, trace, owned, tile, bound, n, what=""):
    """place / trace = numpy quadruples that both started from sentinels; owned[p] = (query, column) or None; tile = score()."""
    distance, span, n_ops, cigar = place
    t_score, t_span, t_ops, t_cigar = trace
    within = 0
    for p, own in enumerate(owned):
        if own is None:
            assert distance[p] == SENT and (span[p] == SENT).all() and n_ops[p] == SENT and (cigar[p] == SENT).all(), f"pair {p} was touched {what}"
            continue
        assert distance[p] == -int(tile[own[0], own[1]]), f"pair {p}: distance {distance[p]}, score() says {tile[own[0], own[1]]} {what}"
        assert distance[p] == -t_score[p], f"pair {p}: distance {distance[p]}, trace_pairs scores {t_score[p]} {what}"
        if distance[p] <= min(bound, n):
            assert span[p].tolist() == t_span[p].tolist(), f"pair {p}: span {span[p].tolist()}, trace_pairs {t_span[p].tolist()} {what}"
            assert n_ops[p] == t_ops[p], f"pair {p}: {n_ops[p]} runs, trace_pairs {t_ops[p]} {what}"
            assert (cigar[p] == t_cigar[p]).all(), f"pair {p}: the cigar rows differ {what}"
            within += 1
        else:
            assert span[p].tolist() == [-1, t_span[p, 1], 0, n], f"pair {p} beyond the bound: span {span[p].tolist()} {what}"
            assert n_ops[p] == 0 and (cigar[p] == SENT).all(), f"pair {p} beyond the bound: n_ops {n_ops[p]} or a written cigar row {what}"
    return within


def assert_place_matches_canonical(place, want, bound, n, cap, what=""):
    """want[p] = (score, span, runs) of trace_reference.canonical, or None to skip the pair."""
    distance, span, n_ops, cigar = place
    cigar = cigar.view(np.uint32)
    for p, w in enumerate(want):
        if w is None:
            continue
        score, (q_begin, e, _, _), runs = w
        assert distance[p] == -score, f"pair {p}: distance {distance[p]}, canonical {-score} {what}"
        if -score <= min(bound, n):
            assert span[p].tolist() == [q_begin, e, 0, n], f"pair {p}: span {span[p].tolist()}, canonical {(q_begin, e, 0, n)} {what}"
            assert n_ops[p] == len(runs), f"pair {p}: {n_ops[p]} runs, canonical {len(runs)} {what}"
            keep = min(len(runs), cap)
            assert A.unpack(cigar[p, :keep]) == runs[:keep], f"pair {p}: {A.to_string(A.unpack(cigar[p, :keep]))} != {A.to_string(runs[:keep])} {what}"
        else:
            assert span[p].tolist() == [-1, e, 0, n] and n_ops[p] == 0, f"pair {p} beyond the bound: {span[p].tolist()}, {n_ops[p]} runs {what}"


# ---- 1. short reads against trace_pairs, bit for bit -----------------------------------------------------------------------
SHORT = dict(m=400, n=150, bound=12, pairs=64 * 3 + 5)


@functools.lru_cache(maxsize=None)
def short_case():
    q, s = make_pairs(SHORT["m"], SHORT["n"], SHORT["pairs"], 20261)      # planted with 0..8 edits, overhangs, two-letter ties, unrelated
    want = T.canonical(q[:24], s[:24], T.FREE_QUERY, T.UNIT)
    return q, s, want


def test_short_reads_equal_trace_pairs_bit_for_bit(torch_gpu):
    torch = torch_gpu
    q, s, want = short_case()
    m, n, bound, pairs = SHORT["m"], SHORT["n"], SHORT["bound"], SHORT["pairs"]
    a = _aligner(q, s)
    pq = np.arange(pairs, dtype=np.int32)
    ps = np.arange(pairs, dtype=np.int64)
    ps[[3, 70, 130, 196]] = -1                        # unused slots
    ps[[5, 64, 191]] = np.array([a.ns, a.ns + 7, 10 ** 12])   # subjects of another bucket
    owned = [(int(pq[p]), int(ps[p])) if 0 <= ps[p] < a.ns else None for p in range(pairs)]
    cap = m + n
    place = _np(a.place_pairs_banded(pq, ps, bound, into=_sentinels(torch, pairs, cap)))
    trace = _np(a.trace_pairs(pq, ps, into=_sentinels(torch, pairs, cap)))
    tile = a.score().cpu().numpy()
    a.check_faults()
    within = assert_place_matches_trace(place, trace, owned, tile, bound, n)
    beyond = sum(o is not None for o in owned) - within
    assert within >= 100 and beyond >= 20, (within, beyond)          # conditions on the inputs
    assert_place_matches_canonical(place, [w if owned[p] else None for p, w in enumerate(want)], bound, n, cap)
    first_ops = [A.unpack(place[3].view(np.uint32)[p, :1])[0][1] for p in range(pairs) if owned[p] and place[2][p] > 0]
    assert first_ops.count(A.OP_D) >= 10                               # reads hanging off the window's start
    assert (place[1][[p for p in range(pairs) if owned[p]], 1] == m).sum() >= 10   # ... and ending at its last row


# ---- 2. every window width ------------------------------------------------------------------------------------------------
WIDE = dict(m=2100, n=1024, pairs=64 + 3, reference=(0, 1, 2, 5, 9, 33, 66))
LADDER = [0, 0, 0, 1, 2, 5, 9, 16, 17, 18, 24, 33, 34, 40, 49, 50, 65, 66, 80, 97, 100, 113, 130, 145, 161, 177, 200, 209, 225,
          241, 250, 273, 289, 300, 321, 337, 353, 369, 385, 400, 417, 433, 449, 465, 481, 482, 500]


@functools.lru_cache(maxsize=None)
def wide_case():
    """67 pairs of 1,024 bp reads in 2,100 bp windows: a ladder of edit counts in the window's middle, at its start and at its end
    (with overhangs from the fourth pair on), and unrelated reads."""
    rng = np.random.default_rng(1024)
    m, n, pairs = WIDE["m"], WIDE["n"], WIDE["pairs"]
    q = ACGT[rng.integers(4, size=(pairs, m))]
    s = np.empty((pairs, n), np.uint8)
    for p in range(pairs):
        if p < len(LADDER):
            kind = ("mid", "start", "end")[p % 3]      # the first three: exact copies mid-window, as its prefix, as its suffix
            s[p] = plant(rng, q[p], n, kind, LADDER[p], at=int(rng.integers(1, m - n)), hang=int(rng.integers(1, 40)) if p >= 3 else 0)
        else:
            s[p] = plant(rng, q[p], n, "unrelated", 0)
    ref = list(WIDE["reference"])
    want = {p: T.canonical(q[p: p + 1], s[p: p + 1], T.FREE_QUERY, T.UNIT)[0] for p in ref}
    return q, s, want


@functools.lru_cache(maxsize=None)
def wide_trace():
    """(the aligner, trace_pairs' quadruple from sentinels, score()) of wide_case, computed once for all widths."""
    import torch
    q, s, _ = wide_case()
    a = _aligner(q, s)
    idx = np.arange(WIDE["pairs"])
    trace = _np(a.trace_pairs(idx, idx, into=_sentinels(torch, WIDE["pairs"], WIDE["m"] + WIDE["n"])))
    tile = a.score().cpu().numpy()
    a.check_faults()
    return a, trace, tile


@pytest.mark.parametrize("width", range(1, 33))
def test_every_window_width(torch_gpu, width):
    torch = torch_gpu
    m, n, pairs = WIDE["m"], WIDE["n"], WIDE["pairs"]
    bound = 0 if width == 1 else 16 * (width - 2) + 1
    assert B.lib().bgsa_hip_place_pairs_band_words(n, bound) == width
    _, _, want = wide_case()
    a, trace, tile = wide_trace()
    idx = np.arange(pairs)
    cap = m + n
    place = _np(a.place_pairs_banded(idx, idx, bound, into=_sentinels(torch, pairs, cap)))
    a.check_faults()
    within = assert_place_matches_trace(place, trace, [(p, p) for p in range(pairs)], tile, bound, n, f"at B = {bound}")
    assert within >= max(3, sum(e <= bound for e in LADDER[::3])), within     # a mid-window read is within its edit count
    assert_place_matches_canonical(place, [want.get(p) for p in range(pairs)], bound, n, cap, f"at B = {bound}")


# ---- 3. beyond 1,024 bp: only the CPU reference exists ---------------------------------------------------------------------
LONG = [(1300, 1057, 20), (2400, 2100, 40)]


@functools.lru_cache(maxsize=None)
def long_case(m, n, bound):
    """Eight distinct pairs: at the window's start with overhang, mid-window across a word boundary, ending at the last row,
    at and just above the bound, and unrelated."""
    rng = np.random.default_rng(m + n)
    q = ACGT[rng.integers(4, size=(8, m))]
    plan = [("start", 3, 0, 7), ("start", bound // 2, 0, 3), ("mid", 0, 29, 0), ("mid", bound // 2, 97, 0), ("end", 5, 0, 6),
            ("mid", bound - 4, m - n, 0), ("mid", 3 * bound, 60, 0), ("unrelated", 0, 0, 0)]
    s = np.stack([plant(rng, q[d], n, kind, edits, at=at, hang=hang) for d, (kind, edits, at, hang) in enumerate(plan)])
    want = [T.canonical(q[d: d + 1], s[d: d + 1], T.FREE_QUERY, T.UNIT)[0] for d in range(8)]
    return q, s, want


@pytest.mark.parametrize("m,n,bound", LONG)
def test_reads_beyond_1024_bp_equal_the_canonical_placement(torch_gpu, m, n, bound):
    torch = torch_gpu
    q, s, want = long_case(m, n, bound)
    dists = [-w[0] for w in want]
    assert sum(d <= bound for d in dists) >= 5 and sum(d > bound for d in dists) >= 2, dists      # conditions on the inputs
    assert any(w[2][0][1] == A.OP_D for w in want) and any(w[1][1] == m for w in want)
    a = _aligner(q, s)
    assert a.wn == (n + 31) // 32 > 32
    pairs = 70
    which = np.array([(p + p // 8) % 8 for p in range(pairs)])      # the eight pairs over the lanes in rotated order
    cap = 64
    place = _np(a.place_pairs_banded(which, which, bound, cigar_cap=cap, into=_sentinels(torch, pairs, cap)))
    tile = a.score().cpu().numpy()
    a.check_faults()
    assert (place[0] == -tile[which, which]).all()
    assert_place_matches_canonical(place, [want[d] for d in which], bound, n, cap)
    cigar = place[3].view(np.uint32)
    for p, d in enumerate(which):
        used = min(len(want[d][2]), cap) if dists[d] <= bound else 0
        assert (cigar[p, used:] == SENT).all(), f"pair {p}: a slot behind the runs was written"


def test_a_window_of_33_words_is_refused_before_any_launch(torch_gpu):
    torch = torch_gpu
    q, s, _ = long_case(1300, 1057, 20)
    a = _aligner(q, s)
    into = _sentinels(torch, 8, 16)
    for kw in (dict(), dict(workspace_bytes=1 << 20), dict(workspace_bytes=0)):
        with pytest.raises(B.BgsaHipError, match="rc=-2.*max_distance <= 496"):
            a.place_pairs_banded(np.arange(8), np.arange(8), 497, cigar_cap=16, into=into, **kw)
    a.check_faults()
    assert all((t == SENT).all().item() for t in into)
    a.place_pairs_banded(np.arange(8), np.arange(8), 496, cigar_cap=16)
    a.check_faults()


# ---- 4. chunking and accumulation -----------------------------------------------------------------------------------------
def test_chunks_library_scratch_and_fresh_outputs_give_the_same_tensors(torch_gpu):
    torch = torch_gpu
    q, s, _ = short_case()
    m, n, bound, pairs = SHORT["m"], SHORT["n"], SHORT["bound"], SHORT["pairs"]
    a = _aligner(q, s)
    pq = np.arange(pairs, dtype=np.int32)
    ps = np.arange(pairs, dtype=np.int64)
    ps[[0, 100]] = -1
    one_pass = _np(a.place_pairs_banded(pq, ps, bound))
    least = int(B.lib().bgsa_hip_place_pairs_banded_min_workspace_bytes(m, n, bound))
    assert least < int(B.lib().bgsa_hip_place_pairs_banded_workspace_bytes(m, n, bound, pairs))
    for workspace in (least, least + 255, 2 * least, 0):      # one wave per chunk, the same, two waves per chunk, the library's scratch
        again = _np(a.place_pairs_banded(pq, ps, bound, workspace_bytes=workspace))
        for x, y in zip(one_pass, again):
            assert (x == y).all(), workspace
    a.check_faults()
    distance, span, n_ops, cigar = one_pass
    for p in (0, 100):                                           # fresh outputs where nothing is owned
        assert distance[p] == -1 and (span[p] == -1).all() and n_ops[p] == 0 and (cigar[p] == 0).all()
    tile = a.score().cpu().numpy()
    own = np.flatnonzero(ps >= 0)
    assert (distance[own] == -tile[own, own]).all()
    with pytest.raises(B.BgsaHipError, match="rc=-1"):
        a.place_pairs_banded(pq, ps, bound, workspace_bytes=least - 1)
    empty = a.place_pairs_banded(np.zeros(0, np.int32), np.zeros(0, np.int64), bound)
    assert [tuple(t.shape) for t in empty] == [(0,), (0, 4), (0,), (0, m + n)]
    a.check_faults()


def test_into_walks_two_buckets_with_subject_base(torch_gpu):
    torch = torch_gpu
    q, s, _ = short_case()
    n, bound = SHORT["n"], SHORT["bound"]
    a = _aligner(q, s)
    pairs = 150
    pq = np.arange(pairs, dtype=np.int32)
    ps = np.arange(pairs, dtype=np.int64)
    whole = _np(a.place_pairs_banded(pq, ps, bound, cigar_cap=40))
    tile = a.score().cpu().numpy()
    assert (whole[0] == -tile[pq, ps]).all()
    # the same subjects as two buckets: columns 0..79 at base 1000, columns 80..149 at base 1080
    ids = ps + 1000
    into = None
    for lo, hi in ((0, 80), (80, 150)):
        a.set_subjects(s[lo:hi])
        into = a.place_pairs_banded(pq, ids, bound, cigar_cap=40, subject_base=1000 + lo, into=into)
        a.check_faults()
    for x, y in zip(whole, _np(into)):
        assert (x == y).all()


def test_place_hits_banded_equals_place_pairs_banded_on_the_flattened_list(torch_gpu):
    torch = torch_gpu
    q, s, _ = short_case()
    m, n, bound = SHORT["m"], SHORT["n"], SHORT["bound"]
    a = _aligner(q[:40], s)
    rng = np.random.default_rng(5)
    hits = rng.integers(0, SHORT["pairs"], size=(40, 3)).astype(np.int64)
    hits[:, 0] = np.arange(40)                # the planted read of every window
    hits[7, 2] = hits[20, 1] = -1
    got = _np(a.place_hits_banded(hits, bound, cigar_cap=30))
    flat = _np(a.place_pairs_banded(np.repeat(np.arange(40), 3), hits.reshape(-1), bound, cigar_cap=30))
    assert [g.shape for g in got] == [(40, 3), (40, 3, 4), (40, 3), (40, 3, 30)]
    for x, y in zip(got, flat):
        assert (x.reshape(y.shape) == y).all()
    into = _sentinels(torch, 120, 30)
    shaped = (into[0].view(40, 3), into[1].view(40, 3, 4), into[2].view(40, 3), into[3].view(40, 3, 30))
    a.place_hits_banded(hits, bound, into=shaped)
    a.check_faults()
    tile = a.score().cpu().numpy()
    for (r, c), h in np.ndenumerate(hits):
        if h < 0:
            assert got[0][r, c] == -1 and into[0].view(40, 3)[r, c].item() == SENT
        else:
            assert got[0][r, c] == -tile[r, h] == into[0].view(40, 3)[r, c].item()


# ---- 5. top level ---------------------------------------------------------------------------------------------------------
def test_the_read_placement_example_of_the_integration_guide(torch_gpu):
    windows = np.stack([np.frombuffer(b"TTGACCATGCAAGTCCGATTACGGATCCTA", np.uint8),
                        np.frombuffer(b"GGCATTCGAGCTTAACGTGCCAATGGTCAT", np.uint8)])
    reads = np.stack([np.frombuffer(b"AGTCCGTTTACG", np.uint8), np.frombuffer(b"TTAACGTGCCAA", np.uint8)])
    for bound in (None, 1, 5):
        scores, queries, spans, cigars = B.place_top_queries_banded(windows, reads, 1, bound)
        assert queries[:, 0].tolist() == [0, 1] and scores[:, 0].tolist() == [-1, 0]
        assert spans[:, 0].tolist() == [[11, 23, 0, 12], [11, 23, 0, 12]]
        assert cigars == [["6=1X5="], ["12="]]
    scores, queries, spans, cigars = B.place_top_queries_banded(windows, reads, 1, 0)      # the first read is beyond B = 0
    assert scores[:, 0].tolist() == [-1, 0] and spans[:, 0].tolist() == [[-1, 23, 0, 12], [11, 23, 0, 12]]
    assert cigars == [[None], ["12="]]
    scores, queries, spans, cigars = B.place_top_queries_banded(windows, reads, 3)         # one unused slot per read
    assert queries[:, 2].tolist() == [-1, -1] and (spans[:, 2] == -1).all() and cigars[0][2] is None and cigars[1][2] is None


def test_place_top_queries_banded_agrees_with_trace_top_queries(torch_gpu):
    rng = np.random.default_rng(50)
    windows = ACGT[rng.integers(4, size=(50, 300))]
    reads = np.stack([plant(rng, windows[c % 50], 100, ("mid", "start", "end")[c % 3], c % 9, at=int(rng.integers(0, 200)), hang=4)
                      for c in range(200)])
    want = B.trace_top_queries(windows, reads, 2, B.ALGO_MYERS, semi_global=True)
    got = B.place_top_queries_banded(windows, reads, 2)
    assert (got[0] == want[0]).all() and (got[1] == want[1]).all() and (got[2] == want[2]).all()
    assert got[3] == want[3]
    assert (got[1][:, 0] == np.arange(200) % 50).all()
    assert -15 <= want[0][:, 0].min() and want[0][:, 1].max() < -15         # conditions on the inputs
    tight = B.place_top_queries_banded(windows, reads, 2, 15)           # the second-best windows are unrelated: beyond 15 edits
    assert (tight[0] == want[0]).all() and [row[0] for row in tight[3]] == [row[0] for row in want[3]]
    assert all(row[1] is None for row in tight[3]) and (tight[2][:, 1, 0] == -1).all() and (tight[2][:, 1, 1] == want[2][:, 1, 1]).all()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------
def test_other_aligners_are_refused_with_nothing_launched(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(6)
    q = ACGT[rng.integers(4, size=(4, 64))]
    s = ACGT[rng.integers(4, size=(70, 64))]
    kinds = [dict(algo=B.ALGO_MYERS), dict(algo=B.ALGO_BITPAL), dict(algo=B.ALGO_BITPAL, semi_global=True), dict(algo=B.ALGO_BANDED, k=8),
             dict(algo=B.ALGO_MYERS, scores=(0, 1, 1), semi_global=True), dict(algo=B.ALGO_MYERS, scores=(0, 1, 1))]
    for kw in kinds:
        kw = dict(kw)
        a = B.DeviceAligner(kw.pop("algo"), "cuda:0", **kw)
        a.set_queries(q)
        a.set_subjects(s)
        into = _sentinels(torch, 4, 8)
        with pytest.raises(B.BgsaHipError, match="rc=-2"):
            a.place_pairs_banded(np.arange(4), np.arange(4), 10, into=into)
        with pytest.raises(B.BgsaHipError, match="rc=-2"):
            a.place_hits_banded(np.zeros((4, 2), np.int64), 10)
        a.check_faults()
        assert all((t == SENT).all().item() for t in into), kw
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=True)
    a.set_queries(q)
    a.set_subjects_ragged([bytes(row[: 40 + 3 * i]) for i, row in enumerate(s[:8])])
    into = _sentinels(torch, 4, 8)
    with pytest.raises(B.BgsaHipError, match="rc=-2.*mixed read lengths"):
        a.place_pairs_banded(np.arange(4), np.arange(4), 10, into=into)
    a.set_subjects(s)
    with pytest.raises(B.BgsaHipError, match="rc=-1"):
        a.place_pairs_banded(np.arange(4), np.arange(4), -1, into=into)
    a.check_faults()
    assert all((t == SENT).all().item() for t in into)
    assert R.band_words(64, 10) == B.lib().bgsa_hip_place_pairs_band_words(64, 10) == 2

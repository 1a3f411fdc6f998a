"""Traced pairs on the MI355X: bgsa_hip_trace_pairs_dev through DeviceAligner.trace_pairs / trace_hits — every score, span, run
count and run EXACTLY as the canonical walk of tests/trace_reference.py, every script validated, every score the score() of
the same aligner, and sentinel-filled outputs untouched wherever nothing is owned."""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import trace_reference as T  # noqa: E402
from test_align_pairs_gpu import shape_case  # noqa: E402  (the pairs of one shape: mutated copies + the special pairs)

pytestmark = pytest.mark.gpu

SENT = 12345          # what pre-filled outputs hold where nothing may be written
FAULT_PAIR = 4
DEFAULT, CHEAP, WIDE = (2, -3, -5), (1, -1, -2), (10, -9, -15)

# kind -> (mode of the reference, the DeviceAligner); the scores of the two BitPAl kinds are a parameter
KINDS = {"bitpal_global": (T.GLOBAL, dict(algo=B.ALGO_BITPAL)),
         "myers_semi": (T.FREE_QUERY, dict(algo=B.ALGO_MYERS, semi_global=True)),
         "bitpal_semi": (T.FREE_SUBJECT, dict(algo=B.ALGO_BITPAL, semi_global=True))}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _aligner(kind, scores, q, s):
    kw = dict(KINDS[kind][1])
    if kw["algo"] == B.ALGO_BITPAL:
        kw["scores"] = scores
    else:
        assert scores == T.UNIT
    a = B.DeviceAligner(kw.pop("algo"), "cuda:0", **kw)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _scores_of(kind, scores=DEFAULT):
    return T.UNIT if kind == "myers_semi" else scores


def _np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _sentinels(torch, n, cap):
    def full(*shape):
        return torch.full(shape, SENT, dtype=torch.int32, device="cuda")
    return full(n), full(n, 4), full(n), full(n, cap)


@functools.lru_cache(maxsize=None)
def shape_want(m, n, kind, scores):
    """The canonical [(score, span, runs)] of shape_case(m, n) in one mode; computed once and shared."""
    q, s, _ = shape_case(m, n)
    return T.canonical(q, s, KINDS[kind][0], scores)


def assert_traces_exact(got, want, cap, mode=None, scores=None, queries=None, subjects=None, tile_scores=None, what=""):
    """got = numpy (score, span[n, 4], n_ops, cigar[n, cap]); want = [(score, span, runs)] or None for a pair that must hold
    sentinels.  No pair is skipped."""
    score, span, n_ops, cigar = got
    cigar = cigar.view(np.uint32)
    assert len(want) == score.shape[0]
    for p, w in enumerate(want):
        if w is None:
            assert score[p] == SENT and (span[p] == SENT).all() and n_ops[p] == SENT and (cigar[p] == SENT).all(), f"pair {p} was touched {what}"
            continue
        sc, sp, runs = w
        assert score[p] == sc, f"pair {p}: score {score[p]}, canonical {sc} {what}"
        assert tuple(span[p].tolist()) == tuple(sp), f"pair {p}: span {span[p].tolist()}, canonical {sp} {what}"
        assert n_ops[p] == len(runs), f"pair {p}: {n_ops[p]} runs, canonical {len(runs)} {what}"
        keep = min(len(runs), cap)
        assert A.unpack(cigar[p, :keep]) == runs[:keep], f"pair {p}: {A.to_string(A.unpack(cigar[p, :keep]))} != {A.to_string(runs[:keep])} {what}"
        assert (cigar[p, keep:] == SENT).all(), f"pair {p}: a slot behind the runs was written {what}"
        if queries is not None and len(runs) <= cap:
            T.validate(queries[p], subjects[p], mode, scores, int(score[p]), span[p], A.unpack(cigar[p, :keep]))
        if tile_scores is not None:
            assert score[p] == int(tile_scores[p]), f"pair {p}: score {score[p]}, score() says {tile_scores[p]} {what}"


# ---- shapes: the smallest that cross each edge the kernels have ------------------------------------------------------------
SHAPES = [(1, 1), (1, 33), (33, 1), (31, 31), (32, 32), (33, 32), (64, 65), (65, 64), (96, 97), (150, 150), (40, 150), (150, 40),
          (1024, 1024)]          # the last: the widest LDS row, the dynamic-LDS opt-in, one wave
SHAPE_CASES = [(m, n, kind, DEFAULT) for m, n in SHAPES for kind in KINDS] + \
              [(m, n, kind, scores) for m, n in ((150, 150), (33, 32)) for kind in ("bitpal_global", "bitpal_semi") for scores in (CHEAP, WIDE)]


@pytest.mark.parametrize("m,n,kind,scores", SHAPE_CASES)
def test_shapes_in_every_mode(torch_gpu, m, n, kind, scores):
    torch = torch_gpu
    scores = _scores_of(kind, scores)
    q, s, _ = shape_case(m, n)
    want = shape_want(m, n, kind, scores)
    pairs = q.shape[0]
    assert pairs % 64 != 0                           # a last wave is partial
    a = _aligner(kind, scores, q, s)
    idx = torch.arange(pairs, device="cuda")
    cap = m + n
    got = _np(a.trace_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    tile = a.score().cpu().numpy()[np.arange(pairs), np.arange(pairs)]
    a.check_faults()
    assert_traces_exact(got, want, cap, KINDS[kind][0], scores, q, s, tile, f"({kind} {scores}, shape {m} x {n})")


# ---- contained reads: the reason the feature exists ------------------------------------------------------------------------
OFFSETS = (0, 1, 31, 32, 33, 110)                    # of a 40 bp window in 150 bp; 110 is the last possible one
PER_OFFSET = 16


@functools.lru_cache(maxsize=None)
def contained_case():
    """(long [P, 150], short [P, 40], offsets [P]): short p is a mutated copy (0..3 edits) of long p's window at its offset."""
    import oracle as O
    count = PER_OFFSET * len(OFFSETS)
    long_reads = O.gen_reads(0xC0417A, count, 150)
    offsets = np.repeat(np.array(OFFSETS), PER_OFFSET)
    windows = np.stack([long_reads[p, off: off + 40] for p, off in enumerate(offsets)])
    short = O.mutate(windows, np.arange(count) % 4, 0xC0417B)
    long_reads.setflags(write=False)
    short.setflags(write=False)
    return long_reads, short, offsets


@pytest.mark.parametrize("kind", ["myers_semi", "bitpal_semi"])
def test_contained_reads_are_located(torch_gpu, kind):
    torch = torch_gpu
    long_reads, short, offsets = contained_case()
    mode, scores = KINDS[kind][0], _scores_of(kind)
    # Myers semi-global places the SUBJECT inside the query, BitPAl semi-global the QUERY inside the subject
    q, s = (long_reads, short) if kind == "myers_semi" else (short, long_reads)
    want = T.canonical(q, s, mode, scores)
    lo, hi = (0, 1) if kind == "myers_semi" else (2, 3)
    interior = [sp[lo] > 0 and sp[hi] < 150 for _, sp, _ in want]
    assert sum(interior) * 2 >= len(want)
    near = [abs(sp[lo] - off) <= 3 and abs(sp[hi] - off - 40) <= 3 for (_, sp, _), off in zip(want, offsets)]
    assert all(near)                                 # the reference finds the window where it was cut, give or take the edits
    pairs = q.shape[0]
    a = _aligner(kind, scores, q, s)
    idx = torch.arange(pairs, device="cuda")
    cap = 190
    got = _np(a.trace_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    tile = a.score().cpu().numpy()[np.arange(pairs), np.arange(pairs)]
    a.check_faults()
    assert_traces_exact(got, want, cap, mode, scores, q, s, tile, f"({kind}, contained reads)")


# ---- the Myers global aligner: the new kernel against align_pairs ------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(150, 150), (65, 64)])
def test_myers_global_traces_equal_align_pairs(torch_gpu, m, n):
    torch = torch_gpu
    q, s, canonical = shape_case(m, n)
    pairs = q.shape[0]
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    a.set_subjects(s)
    idx = torch.arange(pairs, device="cuda")
    cap = m + n
    distance, n_ops, cigar = _np(a.align_pairs(idx, idx))
    got = _np(a.trace_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    a.check_faults()
    want = [(-d, (0, m, 0, n), runs) for d, runs in canonical]
    assert_traces_exact(got, want, cap, T.GLOBAL, T.UNIT, q, s, -distance, f"(Myers global, shape {m} x {n})")
    assert (got[2] == n_ops).all()
    for p in range(pairs):
        assert (got[3][p, : n_ops[p]] == cigar[p, : n_ops[p]]).all(), p


# ---- chunking and workspace -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", list(KINDS))
def test_outputs_do_not_depend_on_the_workspace(torch_gpu, kind):
    torch = torch_gpu
    L = B.lib()
    scores = _scores_of(kind)
    q, s, _ = shape_case(150, 150)
    want = shape_want(150, 150, kind, scores)
    pairs = q.shape[0]
    assert pairs > 3 * 64                             # the minimum workspace holds one wave: four chunks
    a = _aligner(kind, scores, q, s)
    idx = np.arange(pairs)
    small = int(L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150))
    cap = 300
    outs = [_np(a.trace_pairs(idx, idx, into=_sentinels(torch, pairs, cap), workspace_bytes=w)) for w in (small, small * 2 + 100, 0, None)]
    a.check_faults()
    assert_traces_exact(outs[0], want, cap, KINDS[kind][0], scores, q, s, what="(minimum workspace)")
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert x.tobytes() == y.tobytes()


def test_tracing_is_safe_inside_a_stream_capture(torch_gpu):
    torch = torch_gpu
    L = B.lib()
    kind, scores = "bitpal_semi", DEFAULT
    q, s, _ = shape_case(96, 97)
    want = shape_want(96, 97, kind, scores)
    pairs = q.shape[0]
    a = _aligner(kind, scores, q, s)
    a.score()                                         # the device's fault word exists before the capture
    pq = torch.arange(pairs, dtype=torch.int32, device="cuda")
    ps = torch.arange(pairs, dtype=torch.int64, device="cuda")
    cap = 96 + 97
    work = torch.empty(2 * int(L.bgsa_hip_align_pairs_min_workspace_bytes(96, 97)), dtype=torch.uint8, device="cuda")   # two waves: two chunks
    score, span, n_ops, cigar = _sentinels(torch, pairs, cap)
    params = a.params()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        B.check(L.bgsa_hip_trace_pairs_dev(ctypes.byref(params), a.d_content.data_ptr(), a.d_peq.data_ptr(), 96, 97, a.ns, a.wn, pq.data_ptr(),
                                           ps.data_ptr(), pairs, a.nq, 0, score.data_ptr(), span.data_ptr(), n_ops.data_ptr(), cigar.data_ptr(),
                                           cap, work.data_ptr(), work.numel(), _stream(torch)), "trace_pairs_dev (capture)")
    torch.cuda.synchronize()
    assert (score == SENT).all()                      # captured, not run
    replays = []
    for _ in range(2):
        for t in (score, span, n_ops, cigar):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        replays.append(_np((score, span, n_ops, cigar)))
    assert_traces_exact(replays[0], want, cap, KINDS[kind][0], scores, q, s, what="(replayed)")
    for x, y in zip(*replays):
        assert x.tobytes() == y.tobytes()
    assert L.bgsa_hip_stream_faults(1) == 0


# ---- pairs that are not this call's ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes_case():
    """40 queries x 100 subjects of 70 x 75 bp: the bucket is padded to 128 — the last group holds 36 reads and 28 all-'N' rows."""
    import oracle as O
    q = O.gen_reads(701, 40, 70)
    s = np.concatenate([O.mutate(np.concatenate([q, q, q[:20]]), np.arange(100) % 9, 702), O.gen_reads(703, 100, 5)], axis=1)
    padded, _ = B.pad_rows(s)
    return q, s, padded


def _want_of(lanes_case, kind, pq, ps, own=None):
    q, s, padded = lanes_case
    own = [True] * len(pq) if own is None else own
    rows = [p for p, o in enumerate(own) if o]
    some = iter(T.canonical(q[np.asarray(pq)[rows]], padded[np.asarray(ps)[rows]], KINDS[kind][0], _scores_of(kind)))
    return [next(some) if o else None for o in own]


@pytest.mark.parametrize("kind", list(KINDS))
def test_pairs_of_other_buckets_and_unused_slots_are_untouched(torch_gpu, lanes_case, kind):
    torch = torch_gpu
    q, s, padded = lanes_case
    scores = _scores_of(kind)
    a = _aligner(kind, scores, q, s)
    base = 1000
    ps = np.array([base + 5, -1, base - 1, base + 128, base + 127, 5, base, -1, base + 128 + 5, 1 << 40])
    pq = np.arange(10)
    own = [True, False, False, False, True, False, True, False, False, False]
    cap = 145
    got = _np(a.trace_pairs(pq, ps, subject_base=base, into=_sentinels(torch, 10, cap)))
    tile = a.score().cpu().numpy()
    a.check_faults()
    want = _want_of(lanes_case, kind, pq, np.where(own, ps - base, 0), own)
    assert_traces_exact(got, want, cap, KINDS[kind][0], scores, q[pq], padded[np.where(own, ps - base, 0)],
                        tile[pq, np.where(own, ps - base, 0)], f"({kind})")
    # fresh outputs hold score 0, span -1, n_ops 0 and cigar 0 where nothing was written
    fresh = _np(a.trace_pairs(pq, ps, subject_base=base))
    for p, o in enumerate(own):
        if not o:
            assert fresh[0][p] == 0 and (fresh[1][p] == -1).all() and fresh[2][p] == 0 and not fresh[3][p].any()
        else:
            assert fresh[0][p] == got[0][p] and (fresh[1][p] == got[1][p]).all() and fresh[2][p] == got[2][p]


def test_two_buckets_walked_with_into_equal_one_bucket(torch_gpu, lanes_case):
    q, s, padded = lanes_case
    kind, scores = "bitpal_global", DEFAULT
    rng = np.random.default_rng(8)
    pq, ps = rng.integers(0, 40, 150), rng.integers(0, 100, 150)
    ps[::17] = -1
    whole = _aligner(kind, scores, q, s)
    one = _np(whole.trace_pairs(pq, ps))
    a = B.DeviceAligner(B.ALGO_BITPAL, "cuda:0", scores=scores)
    a.set_queries(q)
    out = None
    for lo, hi in ((0, 64), (64, 100)):                 # the second bucket's last group is padded
        a.set_subjects(s[lo:hi])
        out = a.trace_pairs(pq, ps, subject_base=lo, into=out)
    a.check_faults()
    two = _np(out)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    filled = ps >= 0
    want = _want_of(lanes_case, kind, pq, np.where(filled, ps, 0), list(filled))
    for p, w in enumerate(want):
        if w is not None:
            sc, sp, runs = w
            assert (one[0][p], tuple(one[1][p].tolist()), one[2][p], A.unpack(one[3][p, : len(runs)])) == (sc, sp, len(runs), runs), p
    assert (one[0][~filled] == 0).all() and (one[1][~filled] == -1).all() and (one[2][~filled] == 0).all()
    with pytest.raises(B.BgsaHipError):
        a.trace_pairs(pq, ps, into=(out[0], out[1][:5], out[2], out[3]))


def test_a_query_index_out_of_range_touches_nothing_and_raises_the_pair_bit(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded = lanes_case
    kind, scores = "bitpal_semi", DEFAULT
    L = B.lib()
    a = _aligner(kind, scores, q, s)
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == 0
    pq, ps = np.array([4, -1, 40, 7, 1 << 30]), np.array([9, 9, 9, 10, 11])
    own = [True, False, False, True, False]
    got = _np(a.trace_pairs(pq, ps, into=_sentinels(torch, 5, 145)))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(0) == FAULT_PAIR and b"trace_pairs" in L.bgsa_hip_last_error()
    assert L.bgsa_hip_stream_faults(1) == FAULT_PAIR and L.bgsa_hip_stream_faults(1) == 0          # sticky until cleared
    assert_traces_exact(got, _want_of(lanes_case, kind, np.where(own, pq, 0), ps, own), 145)
    # a bad query index on a pair of another bucket is not this call's business
    a.trace_pairs(np.array([-5, 99]), np.array([-1, 128]))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == 0


# ---- the cap --------------------------------------------------------------------------------------------------------------
def test_cap_keeps_the_true_count_and_the_first_runs(torch_gpu):
    torch = torch_gpu
    kind, scores, m, n = "myers_semi", T.UNIT, 150, 150
    q, s, _ = shape_case(m, n)
    want = shape_want(m, n, kind, scores)
    pairs = q.shape[0]
    a = _aligner(kind, scores, q, s)
    idx = np.arange(pairs)
    assert max(len(runs) for _, _, runs in want) > 3
    for cap in (1, 3, m + n):
        score, span, n_ops, _ = _sentinels(torch, pairs, 1)
        room = torch.full((pairs * cap + 16,), SENT, dtype=torch.int32, device="cuda")     # the rows, and 16 slots behind the last one
        got = _np(a.trace_pairs(idx, idx, cigar_cap=cap, into=(score, span, n_ops, room[: pairs * cap].view(pairs, cap))))
        assert (room[pairs * cap:] == SENT).all(), f"a run was written behind the last row (cap {cap})"
        assert_traces_exact(got, want, cap, what=f"(cap {cap})")
    a.check_faults()
    n_ops, cigar = a.trace_pairs(idx, idx, cigar_cap=3)[2:]
    with pytest.raises(B.BgsaHipError):
        B.cigar_strings(n_ops, cigar)
    assert B.cigar_strings(*a.trace_pairs(idx, idx)[2:]) == [A.to_string(runs) for _, _, runs in want]


# ---- hits to traces: 64 queries x 640 subjects of 150 bp, eight planted mutants per query --------------------------------
NQ, NS, PLANT = 64, 640, 8


@pytest.fixture(scope="module")
def planted(oracle):
    q = oracle.gen_reads(0x7ACE_0001, NQ, 150)
    s = oracle.gen_reads(0x7ACE_1001, NS, 150)
    slots = np.random.default_rng(79).permutation(NS)[: NQ * PLANT].reshape(NQ, PLANT)
    for i in range(NQ):
        s[slots[i]] = oracle.mutate(np.repeat(q[i: i + 1], PLANT, axis=0), np.arange(PLANT), 4000 + i)
    return q, s


@pytest.mark.parametrize("kind", ["bitpal_global", "myers_semi"])
def test_top_hits_then_trace_hits_end_to_end(torch_gpu, planted, kind):
    torch = torch_gpu
    q, s = planted
    mode, scores = KINDS[kind][0], _scores_of(kind)
    a = _aligner(kind, scores, q, s)
    before = a.score().clone()
    hit_scores, hit_subjects = a.top_hits(10)
    hit_subjects[::5, 7:] = -1                        # some unused slots, as a short bucket leaves them
    score, span, n_ops, cigar = a.trace_hits(hit_subjects)
    a.check_faults()
    assert tuple(score.shape) == (NQ, 10) and tuple(span.shape) == (NQ, 10, 4) and tuple(n_ops.shape) == (NQ, 10) and tuple(cigar.shape) == (NQ, 10, 300)
    assert all(t.dtype == torch.int32 for t in (score, span, n_ops, cigar))
    hs, sj, sc, sp, k, c = _np((hit_scores, hit_subjects, score, span, n_ops, cigar))
    c = c.view(np.uint32)
    for i in range(NQ):
        for r in range(10):
            if sj[i, r] < 0:
                assert sc[i, r] == 0 and (sp[i, r] == -1).all() and k[i, r] == 0 and not c[i, r].any()
                continue
            assert sc[i, r] == hs[i, r]
            T.validate(q[i], s[sj[i, r]], mode, scores, int(sc[i, r]), sp[i, r], A.unpack(c[i, r, : k[i, r]]))
    best = 300 if kind == "bitpal_global" else 0      # the planted copy itself
    assert (sc[:, 0] == best).all() and (k[:, 0] == 1).all() and (c[:, 0, 0] == (150 << 4 | A.OP_EQ)).all() and (sp[:, 0] == (0, 150, 0, 150)).all()
    # a spot check against the canonical walk (the shapes above compare every pair)
    rows = np.arange(0, NQ, 7)
    want = T.canonical(q[rows], s[sj[rows, 1]], mode, scores)
    assert [(int(sc[i, 1]), tuple(sp[i, 1].tolist()), A.unpack(c[i, 1, : k[i, 1]])) for i in rows] == want
    assert torch.equal(a.score(), before)             # scoring is untouched
    with pytest.raises(B.BgsaHipError):
        a.trace_hits(hit_subjects[:5])
    with pytest.raises(B.BgsaHipError):
        a.trace_hits(hit_subjects, into=(score, span[:, :, :2], n_ops, cigar))


@pytest.mark.parametrize("kind", ["bitpal_global", "myers_semi"])
def test_trace_top_hits_convenience(torch_gpu, planted, kind):
    q, s = planted
    mode, scores = KINDS[kind][0], _scores_of(kind)
    kw = dict(KINDS[kind][1])
    algo = kw.pop("algo")
    if algo == B.ALGO_BITPAL:
        kw["scores"] = scores
    hit_scores, subjects, spans, cigars = B.trace_top_hits(q[:9], s[:7], 10, algo, **kw)       # seven subjects: three unused slots per query
    assert hit_scores.shape == (9, 10) and subjects.shape == (9, 10) and spans.shape == (9, 10, 4)
    assert len(cigars) == 9 and all(len(row) == 10 for row in cigars)
    for i in range(9):
        for r in range(10):
            if subjects[i, r] < 0:
                assert r >= 7 and cigars[i][r] is None and (spans[i, r] == -1).all()
                continue
            runs = A.from_string(cigars[i][r])
            assert A.to_string(runs) == cigars[i][r]
            T.validate(q[i], s[subjects[i, r]], mode, scores, int(hit_scores[i, r]), spans[i, r], runs)


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["banded", "plus_distance"])
def test_banded_and_plus_distance_are_refused_before_any_launch(torch_gpu, planted, kind):
    q, s = planted
    kw = {"banded": dict(algo=B.ALGO_BANDED, k=8), "plus_distance": dict(algo=B.ALGO_MYERS, scores=(0, 1, 1))}[kind]
    a = B.DeviceAligner(kw.pop("algo"), "cuda:0", **kw)
    a.set_queries(q[:4])
    a.set_subjects(s[:64])
    into = _sentinels(torch_gpu, 3, 300)
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.trace_pairs([0, 1, 2], [0, 1, 2], into=into)
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.trace_hits(torch_gpu.zeros((4, 2), dtype=torch_gpu.int64, device="cuda"))
    # the C call's own answer, for a caller that does not come through DeviceAligner
    p = a.params()
    rc = B.lib().bgsa_hip_trace_pairs_dev(ctypes.byref(p), a.d_content.data_ptr(), a.d_peq.data_ptr(), 150, 150, a.ns, a.wn, into[0].data_ptr(),
                                          into[0].data_ptr(), 3, 4, 0, into[0].data_ptr(), into[1].data_ptr(), into[2].data_ptr(),
                                          into[3].data_ptr(), 300, None, 0, _stream(torch_gpu))
    assert rc == -2
    torch_gpu.cuda.synchronize()
    assert all((t == SENT).all() for t in into)

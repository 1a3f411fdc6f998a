"""Pair alignment on the MI355X: bgsa_hip_myers_align_pairs_dev through DeviceAligner.align_pairs / align_hits — every
distance, run count and run EXACTLY as the canonical traceback of tests/align_reference.py, every script validated, and
every distance the negated score()."""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 12345          # what pre-filled outputs hold where nothing may be written
FAULT_PAIR = 4


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _aligner(q, s, **kw):
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", **kw)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


def _sentinels(torch, n, cap):
    return (torch.full((n,), SENT, dtype=torch.int32, device="cuda"), torch.full((n,), SENT, dtype=torch.int32, device="cuda"),
            torch.full((n, cap), SENT, dtype=torch.int32, device="cuda"))


# ---- the pairs of one shape: pair p = (query p, subject p) ---------------------------------------------------------------
SHAPES = [(1, 1), (1, 33), (31, 31), (32, 32), (33, 32), (64, 65), (65, 64), (96, 97), (150, 150), (150, 140), (140, 150),
          (40, 150), (150, 40), (1024, 1024), (1000, 1024)]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def shape_case(m, n):
    """(queries [P, m], subjects [P, n], canonical [(distance, runs)] per pair); computed once per shape and shared."""
    import oracle as O
    seed = 7919 * m + n
    rng = np.random.default_rng(seed)
    longest = max(m, n)
    count = 8 if longest >= 1000 else 190
    # substitutions, insertions and deletions anywhere in the read: the paths leave the main diagonal and cross word borders
    base = O.gen_reads(seed, count, longest)
    edits = (7 * np.arange(count)) % (min(longest, 24) + 1)
    mutants = O.mutate(base, edits, seed + 1)
    q, s = [base[:, :m]], [mutants[:, :n]]

    def add(qr, sr):
        q.append(np.asarray(qr, dtype=np.uint8)[None, :m])
        s.append(np.asarray(sr, dtype=np.uint8)[None, :n])

    add(np.full(m, ord("A")), np.full(n, ord("A")))                                  # every cell a tie: the tie-break decides it all
    one = ACGT[rng.integers(0, 4, longest)]
    for shift in (1, 31, 32, 33):                                                    # the query, `shift` columns to the right
        add(one, np.concatenate([ACGT[rng.integers(0, 4, shift)], one])[:longest])
    add(np.full(m, ord("A")), np.full(n, ord("C")))                                  # all mismatch
    with_n = ACGT[rng.integers(0, 4, (2, longest))]
    with_n[0, ::3] = ord("N")
    with_n[1, ::4] = ord("N")
    with_n[1, -1] = with_n[0, -1] = ord("N")
    add(with_n[0], with_n[1])                                                        # 'N' on both sides
    foreign = ACGT[rng.integers(0, 4, (2, longest))]
    foreign[0, ::5], foreign[1, ::7], foreign[1, -1] = ord("x"), 200, ord("*")
    add(foreign[0], foreign[1])                                                      # bytes outside the alphabet: class 0
    q, s = np.concatenate(q), np.concatenate(s)
    q.setflags(write=False)
    s.setflags(write=False)
    return q, s, A.canonical(q, s)


def assert_pairs_exact(got, want, cap, queries=None, subjects=None, scores=None, what=""):
    """got = numpy (distance, n_ops, cigar[n, cap]); want = [(distance, runs)] or None for a pair that must hold sentinels."""
    distance, n_ops, cigar = got
    cigar = cigar.view(np.uint32)
    for p, w in enumerate(want):
        if w is None:
            assert distance[p] == SENT and n_ops[p] == SENT and (cigar[p] == SENT).all(), f"pair {p} was touched {what}"
            continue
        d, runs = w
        assert distance[p] == d, f"pair {p}: distance {distance[p]}, canonical {d} {what}"
        assert n_ops[p] == len(runs), f"pair {p}: {n_ops[p]} runs, canonical {len(runs)} {what}"
        keep = min(len(runs), cap)
        assert A.unpack(cigar[p, :keep]) == runs[:keep], f"pair {p}: {A.to_string(A.unpack(cigar[p, :keep]))} != {A.to_string(runs[:keep])} {what}"
        assert (cigar[p, keep:] == SENT).all(), f"pair {p}: a slot behind the runs was written {what}"
        if queries is not None and len(runs) <= cap:
            A.validate(queries[p], subjects[p], int(distance[p]), A.unpack(cigar[p, :keep]))
        if scores is not None:
            assert distance[p] == -int(scores[p]), f"pair {p}: distance {distance[p]}, score {scores[p]} {what}"


@pytest.mark.parametrize("m,n", SHAPES)
def test_word_edges_and_carries(torch_gpu, m, n):
    torch = torch_gpu
    q, s, want = shape_case(m, n)
    pairs = q.shape[0]
    a = _aligner(q, s)
    idx = torch.arange(pairs, device="cuda")
    cap = m + n
    got = _np(a.align_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    scores = a.score().cpu().numpy()[np.arange(pairs), np.arange(pairs)]
    a.check_faults()
    assert_pairs_exact(got, want, cap, q, s, scores, f"(shape {m} x {n})")


# ---- lanes ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lanes_case():
    """40 queries x 100 subjects of 70 x 75 bp: the bucket is padded to 128 — the last group holds 36 reads and 28 all-'N' rows."""
    import oracle as O
    q = O.gen_reads(501, 40, 70)
    s = np.concatenate([O.mutate(np.concatenate([q, q, q[:20]]), np.arange(100) % 9, 502), O.gen_reads(503, 100, 5)], axis=1)
    padded, _ = B.pad_rows(s)

    @functools.lru_cache(maxsize=None)
    def want(qi, sj):
        return A.canonical(q[qi][None, :], padded[sj][None, :])[0]
    return q, s, padded, want


def _lane_lists():
    rng = np.random.default_rng(66)
    lists = {}
    for n_pairs in (1, 63, 64, 65, 200):
        lists[f"{n_pairs} random"] = (rng.integers(0, 40, n_pairs), rng.integers(0, 100, n_pairs))
    lists["one subject in many pairs"] = (np.arange(40).repeat(2), np.full(80, 77))
    lists["the same pair twice"] = (np.array([3, 3, 9, 3]), np.array([5, 5, 5, 5]))
    lists["descending"] = (np.sort(rng.integers(0, 40, 130))[::-1].copy(), np.sort(rng.integers(0, 100, 130))[::-1].copy())
    lists["the last, padded group"] = (rng.integers(0, 40, 70), np.concatenate([np.arange(64, 100), np.arange(100, 128), rng.integers(64, 128, 6)]))
    return lists


@pytest.mark.parametrize("name", list(_lane_lists()))
def test_lanes(torch_gpu, lanes_case, name):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    pq, ps = _lane_lists()[name]
    a = _aligner(q, s)
    assert a.ns == 128 and a.ns_real == 100
    cap = 70 + 75
    got = _np(a.align_pairs(pq, ps, into=_sentinels(torch, len(pq), cap)))
    tile = a.score().cpu().numpy()
    a.check_faults()
    assert_pairs_exact(got, [want(int(i), int(j)) for i, j in zip(pq, ps)], cap, q[pq], padded[ps], tile[pq, ps], f"({name})")


# ---- pairs that are not this call's ---------------------------------------------------------------------------------------
def test_pairs_of_other_buckets_and_unused_slots_are_untouched(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    a = _aligner(q, s)
    base = 1000
    ps = np.array([base + 5, -1, base - 1, base + 128, base + 127, 5, base, -1, base + 128 + 5, 1 << 40])
    pq = np.arange(10)
    own = [True, False, False, False, True, False, True, False, False, False]
    cap = 145
    got = _np(a.align_pairs(pq, ps, subject_base=base, into=_sentinels(torch, 10, cap)))
    a.check_faults()
    assert_pairs_exact(got, [want(int(i), int(j - base)) if o else None for i, j, o in zip(pq, ps, own)], cap)
    # fresh outputs hold distance -1, n_ops 0 and cigar 0 where nothing was written
    fresh = _np(a.align_pairs(pq, ps, subject_base=base))
    for p, o in enumerate(own):
        if not o:
            assert fresh[0][p] == -1 and fresh[1][p] == 0 and not fresh[2][p].any()
        else:
            assert fresh[0][p] == got[0][p] and fresh[1][p] == got[1][p]


def test_two_buckets_walked_with_into_equal_one_bucket(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    rng = np.random.default_rng(8)
    pq, ps = rng.integers(0, 40, 150), rng.integers(0, 100, 150)
    ps[::17] = -1
    whole = _aligner(q, s)
    one = _np(whole.align_pairs(pq, ps))
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    out = None
    for lo, hi in ((0, 64), (64, 100)):                 # the second bucket's last group is padded
        a.set_subjects(s[lo:hi])
        out = a.align_pairs(pq, ps, subject_base=lo, into=out)
    a.check_faults()
    two = _np(out)
    for x, y in zip(one, two):
        assert x.tobytes() == y.tobytes()
    for p, (i, j) in enumerate(zip(pq, ps)):
        if j >= 0:
            d, runs = want(int(i), int(j))
            assert (one[0][p], one[1][p], A.unpack(one[2][p, : len(runs)])) == (d, len(runs), runs), p
    filled = ps >= 0
    assert (one[0][filled] >= 0).all() and (one[0][~filled] == -1).all() and (one[1][~filled] == 0).all()
    with pytest.raises(B.BgsaHipError):
        a.align_pairs(pq, ps, into=(out[0], out[1][:5], out[2]))


def test_a_query_index_out_of_range_touches_nothing_and_raises_the_pair_bit(torch_gpu, lanes_case):
    torch = torch_gpu
    q, s, padded, want = lanes_case
    L = B.lib()
    a = _aligner(q, s)
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == 0
    pq, ps = np.array([4, -1, 40, 7, 1 << 30]), np.array([9, 9, 9, 10, 11])
    got = _np(a.align_pairs(pq, ps, into=_sentinels(torch, 5, 145)))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(0) == FAULT_PAIR and b"align_pairs" in L.bgsa_hip_last_error()
    assert L.bgsa_hip_stream_faults(1) == FAULT_PAIR and L.bgsa_hip_stream_faults(1) == 0          # sticky until cleared
    assert_pairs_exact(got, [want(4, 9), None, None, want(7, 10), None], 145)
    # a bad query index on a pair of another bucket is not this call's business
    a.align_pairs(np.array([-5, 99]), np.array([-1, 128]))
    torch.cuda.synchronize()
    assert L.bgsa_hip_stream_faults(1) == 0


# ---- the cap --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", [(150, 140), (33, 32)])
def test_cap_keeps_the_true_count_and_the_first_runs(torch_gpu, m, n):
    torch = torch_gpu
    q, s, want = shape_case(m, n)
    pairs = q.shape[0]
    a = _aligner(q, s)
    idx = np.arange(pairs)
    assert max(len(runs) for _, runs in want) > 3
    for cap in (1, 3, m + n):
        dist, n_ops, _ = _sentinels(torch, pairs, 1)
        room = torch.full((pairs * cap + 16,), SENT, dtype=torch.int32, device="cuda")     # the rows, and 16 slots behind the last one
        got = _np(a.align_pairs(idx, idx, cigar_cap=cap, into=(dist, n_ops, room[: pairs * cap].view(pairs, cap))))
        assert (room[pairs * cap:] == SENT).all(), f"a run was written behind the last row (cap {cap})"
        assert_pairs_exact(got, want, cap, what=f"(cap {cap})")
    a.check_faults()
    n_ops, cigar = a.align_pairs(idx, idx, cigar_cap=3)[1:]
    with pytest.raises(B.BgsaHipError):
        B.cigar_strings(n_ops, cigar)
    assert B.cigar_strings(*a.align_pairs(idx, idx)[1:]) == [A.to_string(runs) for _, runs in want]


# ---- chunking and workspace -----------------------------------------------------------------------------------------------
def test_outputs_do_not_depend_on_the_workspace(torch_gpu):
    torch = torch_gpu
    L = B.lib()
    q, s, want = shape_case(150, 140)
    pairs = q.shape[0]
    assert pairs > 3 * 64                             # the minimum workspace holds one wave: four chunks
    a = _aligner(q, s)
    idx = np.arange(pairs)
    small = int(L.bgsa_hip_align_pairs_min_workspace_bytes(150, 140))
    full = int(L.bgsa_hip_align_pairs_workspace_bytes(150, 140, pairs))
    assert full == 4 * small
    cap = 290
    outs = [_np(a.align_pairs(idx, idx, into=_sentinels(torch, pairs, cap), workspace_bytes=w)) for w in (small, small * 2 + 100, full, 0, None)]
    a.check_faults()
    assert_pairs_exact(outs[0], want, cap, q, s, what="(minimum workspace)")
    for other in outs[1:]:
        for x, y in zip(outs[0], other):
            assert x.tobytes() == y.tobytes()


def test_alignment_is_safe_inside_a_stream_capture(torch_gpu):
    torch = torch_gpu
    L = B.lib()
    q, s, want = shape_case(96, 97)
    pairs = q.shape[0]
    a = _aligner(q, s)
    a.score()                                         # the device's fault word exists before the capture
    pq = torch.arange(pairs, dtype=torch.int32, device="cuda")
    ps = torch.arange(pairs, dtype=torch.int64, device="cuda")
    cap = 96 + 97
    work = torch.empty(2 * int(L.bgsa_hip_align_pairs_min_workspace_bytes(96, 97)), dtype=torch.uint8, device="cuda")   # two waves: two chunks
    dist, n_ops, cigar = _sentinels(torch, pairs, cap)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        B.check(L.bgsa_hip_myers_align_pairs_dev(a.d_content.data_ptr(), a.d_peq.data_ptr(), 96, 97, a.ns, a.wn, pq.data_ptr(), ps.data_ptr(),
                                                 pairs, a.nq, 0, dist.data_ptr(), n_ops.data_ptr(), cigar.data_ptr(), cap, work.data_ptr(),
                                                 work.numel(), _stream(torch)), "myers_align_pairs_dev (capture)")
    torch.cuda.synchronize()
    assert (dist == SENT).all()                       # captured, not run
    replays = []
    for _ in range(2):
        for t in (dist, n_ops, cigar):
            t.fill_(SENT)
        g.replay()
        torch.cuda.synchronize()
        replays.append(_np((dist, n_ops, cigar)))
    assert_pairs_exact(replays[0], want, cap, q, s, what="(replayed)")
    for x, y in zip(*replays):
        assert x.tobytes() == y.tobytes()
    assert L.bgsa_hip_stream_faults(1) == 0


# ---- end to end: 64 queries x 640 subjects of 150 bp, eight planted mutants per query -----------------------------------
NQ, NS, PLANT = 64, 640, 8


@pytest.fixture(scope="module")
def planted(oracle):
    q = oracle.gen_reads(0xA116_0001, NQ, 150)
    s = oracle.gen_reads(0xA116_1001, NS, 150)
    slots = np.random.default_rng(78).permutation(NS)[: NQ * PLANT].reshape(NQ, PLANT)
    for i in range(NQ):
        s[slots[i]] = oracle.mutate(np.repeat(q[i: i + 1], PLANT, axis=0), np.arange(PLANT), 2000 + i)
    return q, s


def test_top_hits_then_align_hits_end_to_end(torch_gpu, oracle, planted):
    torch = torch_gpu
    q, s = planted
    a = _aligner(q, s)
    before = a.score().clone()
    hit_scores, hit_subjects = a.top_hits(10)
    hit_subjects[::5, 7:] = -1                        # some unused slots, as a short bucket leaves them
    distance, n_ops, cigar = a.align_hits(hit_subjects)
    a.check_faults()
    assert tuple(distance.shape) == (NQ, 10) and tuple(n_ops.shape) == (NQ, 10) and tuple(cigar.shape) == (NQ, 10, 300)
    assert distance.dtype == torch.int32 and n_ops.dtype == torch.int32 and cigar.dtype == torch.int32
    sc, sj, d, k, c = _np((hit_scores, hit_subjects, distance, n_ops, cigar))
    c = c.view(np.uint32)
    scores = oracle.myers64(q, s)
    for i in range(NQ):
        for r in range(10):
            if sj[i, r] < 0:
                assert d[i, r] == -1 and k[i, r] == 0 and not c[i, r].any()
                continue
            assert d[i, r] == -sc[i, r] == -int(scores[i, sj[i, r]])
            A.validate(q[i], s[sj[i, r]], int(d[i, r]), A.unpack(c[i, r, : k[i, r]]))
    assert (d[:, 0] == 0).all() and (k[:, 0] == 1).all() and (c[:, 0, 0] == (150 << 4 | A.OP_EQ)).all()   # the planted copy itself
    # a spot check against the canonical script (the shapes above compare every pair)
    rows = np.arange(0, NQ, 7)
    want = A.canonical(q[rows], s[sj[rows, 1]])
    assert [(int(d[i, 1]), A.unpack(c[i, 1, : k[i, 1]])) for i in rows] == want
    assert torch.equal(a.score(), before)             # scoring is untouched
    with pytest.raises(B.BgsaHipError):
        a.align_hits(hit_subjects[:5])


def test_align_top_alignments_convenience(torch_gpu, oracle, planted):
    q, s = planted
    scores, subjects, cigars = B.align_top_alignments(q[:9], s[:7], 10)       # seven subjects: three unused slots per query
    assert scores.shape == (9, 10) and subjects.shape == (9, 10) and len(cigars) == 9 and all(len(row) == 10 for row in cigars)
    for i in range(9):
        for r in range(10):
            if subjects[i, r] < 0:
                assert r >= 7 and cigars[i][r] is None
                continue
            runs = A.from_string(cigars[i][r])
            assert A.to_string(runs) == cigars[i][r]
            assert sum(n for n, op in runs if op != A.OP_D) == 150 and sum(n for n, op in runs if op != A.OP_I) == 150
            A.validate(q[i], s[subjects[i, r]], -int(scores[i, r]), runs)


# ---- refusals -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["semi_global", "bitpal", "bitpal_edit", "banded", "plus_distance"])
def test_other_aligners_are_refused_before_any_launch(torch_gpu, planted, kind):
    q, s = planted
    kw = {"semi_global": dict(algo=B.ALGO_MYERS, semi_global=True), "bitpal": dict(algo=B.ALGO_BITPAL, scores=(2, -3, -5)),
          "bitpal_edit": dict(algo=B.ALGO_BITPAL, scores=(0, -1, -1)), "banded": dict(algo=B.ALGO_BANDED, k=8),
          "plus_distance": dict(algo=B.ALGO_MYERS, scores=(0, 1, 1))}[kind]
    a = B.DeviceAligner(kw.pop("algo"), "cuda:0", **kw)
    a.set_queries(q[:4])
    a.set_subjects(s[:64])
    into = _sentinels(torch_gpu, 3, 300)
    with pytest.raises(B.BgsaHipError):
        a.align_pairs([0, 1, 2], [0, 1, 2], into=into)
    with pytest.raises(B.BgsaHipError):
        a.align_hits(torch_gpu.zeros((4, 2), dtype=torch_gpu.int64, device="cuda"))
    torch_gpu.cuda.synchronize()
    assert all((t == SENT).all() for t in into)


def test_subjects_beyond_1024_bp_are_refused(torch_gpu, oracle):
    a = _aligner(oracle.gen_reads(1, 2, 100), oracle.gen_reads(2, 64, 1056))
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.align_pairs([0], [0])

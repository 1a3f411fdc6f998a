"""Hit lists per subject on the MI355X: bgsa_hip_top_queries_dev / bgsa_hip_threshold_queries_dev on synthetic tiles, and
DeviceAligner.top_queries / threshold_queries / query_hits_as_pairs and the numpy conveniences end to end — everything bit
for bit against tests/query_hits_reference.py."""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import oracle as O  # noqa: E402
import query_hits_reference as Q  # noqa: E402
import trace_reference as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
DTYPES = {2: np.int16, 1: np.int8}
CANARY = 12345
SPARE = 5        # rows the outputs are allocated beyond valid_count: nothing may be written there


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _device_tile(torch, tile):
    return tile if torch.is_tensor(tile) else torch.from_numpy(np.ascontiguousarray(tile)).cuda()


def _outputs(torch, valid, width, into, n):
    """n canary-filled int32 [valid + SPARE, width] device tensors, the first `valid` rows taken from `into` if given."""
    outs = [torch.full((valid + SPARE, width), CANARY, dtype=torch.int32, device="cuda") for _ in range(n)]
    if into is not None:
        for t, x in zip(outs, into):
            t[:valid] = torch.from_numpy(np.ascontiguousarray(x, dtype=np.int32)).cuda().view(valid, -1)
    return outs


def run_top(torch, tile, valid, k, smallest, base=0, into=None, own_workspace=True):
    """tile: numpy [nq, stride] int16 / int8 (or a device tensor) -> numpy (scores[valid, k], queries[valid, k])."""
    L = B.lib()
    d_tile = _device_tile(torch, tile)
    nq, stride = d_tile.shape[0], d_tile.stride(0)
    sc, hq = _outputs(torch, valid, k, into, 2)
    ws, ws_bytes = None, 0
    if own_workspace:
        ws_bytes = int(L.bgsa_hip_query_hits_workspace_bytes(nq, stride, d_tile.element_size(), k))
        work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        ws = work.data_ptr()
    B.check(L.bgsa_hip_top_queries_dev(d_tile.data_ptr(), d_tile.element_size(), nq, stride, valid, base, k, int(smallest),
                                       int(into is not None), sc.data_ptr(), hq.data_ptr(), ws, ws_bytes, _stream(torch)), "top_queries_dev")
    torch.cuda.synchronize()
    sc, hq = sc.cpu().numpy(), hq.cpu().numpy()
    assert (sc[valid:] == CANARY).all() and (hq[valid:] == CANARY).all(), "written beyond valid_count lists"
    return sc[:valid], hq[:valid]


def run_threshold(torch, tile, valid, cutoff, smallest, cap, base=0, into=None, own_workspace=True):
    L = B.lib()
    d_tile = _device_tile(torch, tile)
    nq, stride = d_tile.shape[0], d_tile.stride(0)
    cnt, = _outputs(torch, valid, 1, None if into is None else into[:1], 1)
    sc, hq = _outputs(torch, valid, cap, None if into is None else into[1:], 2)
    ws, ws_bytes = None, 0
    if own_workspace:
        ws_bytes = int(L.bgsa_hip_query_hits_workspace_bytes(nq, stride, d_tile.element_size(), 1))
        work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        ws = work.data_ptr()
    B.check(L.bgsa_hip_threshold_queries_dev(d_tile.data_ptr(), d_tile.element_size(), nq, stride, valid, base, cutoff, int(smallest),
                                             int(into is not None), cap, cnt.data_ptr(), sc.data_ptr(), hq.data_ptr(), ws, ws_bytes,
                                             _stream(torch)), "threshold_queries_dev")
    torch.cuda.synchronize()
    cnt, sc, hq = cnt.cpu().numpy(), sc.cpu().numpy(), hq.cpu().numpy()
    assert (cnt[valid:] == CANARY).all() and (sc[valid:] == CANARY).all() and (hq[valid:] == CANARY).all(), "written beyond valid_count"
    return cnt[:valid, 0], sc[:valid], hq[:valid]


def assert_top_equal(got, want, what=""):
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), f"scores differ {what}"
    assert np.array_equal(got[1], want[1]), f"queries differ {what}"


def padded(body, stride):
    """body [nq, valid] inside a tile of `stride` columns; the columns behind it hold the best score of BOTH directions
    alternately (the extremes of the type), so a kernel that reads them shows it."""
    dt = body.dtype
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    nq, valid = body.shape
    tile = np.empty((nq, stride), dtype=dt)
    tile[:, :valid] = body
    tile[:, valid:] = np.where((np.arange(stride - valid)[None, :] + np.arange(nq)[:, None]) % 2 == 0, hi, lo).astype(dt)
    return tile


# ---- synthetic tiles straight into the C ABI ---------------------------------------------------------------------------
@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("k", [1, 2, 10, 64])
def test_top_queries_row_counts_around_k(torch_gpu, elem, k):
    rng = np.random.default_rng(1000 * elem + k)
    for rows in sorted({1, 2, max(1, k - 1), k, k + 1, 300}):
        for smallest in (False, True):
            tile = padded(rng.integers(-3, 4, (rows, 130)).astype(DTYPES[elem]), 192)      # seven values: ties everywhere
            got = run_top(torch_gpu, tile, 130, k, smallest, base=40)
            assert_top_equal(got, Q.top_queries(tile, 130, k, smallest, 40), f"(rows {rows}, k {k}, smallest {smallest})")
            if rows < k:     # fewer rows than K: query -1 and the worst int32 in the rest
                assert (got[1][:, rows:] == -1).all() and (got[0][:, rows:] == Q.worst(smallest)).all()
                assert (got[1][:, :rows] >= 40).all()


@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("valid", [1, 63, 64, 65, 130])
def test_valid_count_inside_the_stride_pads_influence_nothing(torch_gpu, elem, valid):
    rng = np.random.default_rng(7 * valid + elem)
    body = rng.integers(-9, 10, (37, valid)).astype(DTYPES[elem])
    tile = padded(body, 192)
    other = tile.copy()
    other[:, valid:] = 0                                   # the same candidates, other pads
    for smallest in (False, True):
        got = run_top(torch_gpu, tile, valid, 5, smallest)
        assert_top_equal(got, Q.top_queries(body, valid, 5, smallest), f"(valid {valid})")
        assert_top_equal(run_top(torch_gpu, other, valid, 5, smallest), got, "(pads changed)")
        thr = run_threshold(torch_gpu, tile, valid, 6 if not smallest else -6, smallest, 4)
        assert Q.threshold_lists_equal(thr, Q.threshold_queries(body, valid, 6 if not smallest else -6, smallest, 4), 4)
        again = run_threshold(torch_gpu, other, valid, 6 if not smallest else -6, smallest, 4)
        assert all(np.array_equal(x, y) for x, y in zip(thr, again))


@pytest.mark.parametrize("elem,stride,offset", [(2, 70, 1), (2, 70, 0), (1, 67, 0), (1, 67, 3)])
def test_unaligned_tiles_equal_their_aligned_copy(torch_gpu, elem, stride, offset):
    torch = torch_gpu
    rng = np.random.default_rng(stride + offset)
    rows = 41
    body = rng.integers(-5, 6, (rows, stride)).astype(DTYPES[elem])
    flat = torch.zeros(offset + rows * stride + 64, dtype=torch.int16 if elem == 2 else torch.int8, device="cuda")
    tile = flat[offset: offset + rows * stride].view(rows, stride)
    tile.copy_(torch.from_numpy(body).cuda())
    assert tile.data_ptr() == flat.data_ptr() + offset * elem
    aligned = np.zeros((rows, 128), dtype=DTYPES[elem])
    for valid in (stride, stride - 3):
        aligned[:, :stride] = body
        for smallest in (False, True):
            got = run_top(torch, tile, valid, 4, smallest, base=9)
            assert_top_equal(got, run_top(torch, aligned, valid, 4, smallest, base=9), "(aligned copy)")
            assert_top_equal(got, Q.top_queries(body, valid, 4, smallest, 9))
            thr = run_threshold(torch, tile, valid, 3, smallest, 6, base=9)
            same = run_threshold(torch, aligned, valid, 3, smallest, 6, base=9)
            assert all(np.array_equal(x, y) for x, y in zip(thr, same))
            assert Q.threshold_lists_equal(thr, Q.threshold_queries(body, valid, 3, smallest, 6, 9), 6)


@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("smallest", [False, True])
def test_order_of_equal_improving_worsening_and_extreme_scores(torch_gpu, elem, smallest):
    dt = DTYPES[elem]
    lo, hi = int(np.iinfo(dt).min), int(np.iinfo(dt).max)
    rows, cols, k, base = 200, 70, 10, 500
    # all scores equal: the lists are the first K query ids
    got = run_top(torch_gpu, np.full((rows, cols), 7, dtype=dt), cols, k, smallest, base=base)
    assert (got[1] == np.arange(base, base + k, dtype=np.int32)[None, :]).all() and (got[0] == 7).all()
    # strictly improving with the row (every row enters every list), and strictly worsening (only the first K do)
    ramp = (np.arange(rows)[:, None] - 100 + np.zeros((1, cols), dtype=np.int64))
    better_later = (-ramp if smallest else ramp).astype(dt)
    got = run_top(torch_gpu, better_later, cols, k, smallest, base=base)
    assert (got[1] == np.arange(base + rows - 1, base + rows - 1 - k, -1, dtype=np.int32)[None, :]).all()
    assert_top_equal(got, Q.top_queries(better_later, cols, k, smallest, base), "(improving)")
    worse_later = np.ascontiguousarray(better_later[::-1])
    got = run_top(torch_gpu, worse_later, cols, k, smallest, base=base)
    assert (got[1] == np.arange(base, base + k, dtype=np.int32)[None, :]).all()
    assert_top_equal(got, Q.top_queries(worse_later, cols, k, smallest, base), "(worsening)")
    # the extremes of the type, several of each per column, among small scores
    rng = np.random.default_rng(3 + elem)
    ext = rng.integers(-20, 20, (rows, cols)).astype(dt)
    ext[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] = lo
    ext[rng.integers(0, rows, 40), rng.integers(0, cols, 40)] = hi
    ext[[0, 1, 198, 199], 0] = [hi, lo, lo, hi]
    ext[:, 1] = hi
    ext[:, 2] = lo
    for kk in (3, 64):
        assert_top_equal(run_top(torch_gpu, ext, cols, kk, smallest, base=base), Q.top_queries(ext, cols, kk, smallest, base), "(extremes)")
    thr = run_threshold(torch_gpu, ext, cols, lo if smallest else hi, smallest, 8, base=base)
    assert Q.threshold_lists_equal(thr, Q.threshold_queries(ext, cols, lo if smallest else hi, smallest, 8, base), 8)


@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("smallest", [False, True])
def test_accumulate_over_query_blocks_and_query_sets(torch_gpu, elem, smallest):
    rng = np.random.default_rng(50 + elem)
    whole = padded(rng.integers(-4, 5, (72, 130)).astype(DTYPES[elem]), 192)
    for k in (6, 64):
        top = None
        for lo, hi in ((0, 7), (7, 71), (71, 72)):
            top = run_top(torch_gpu, whole[lo:hi], 130, k, smallest, base=lo, into=top)
        want = Q.top_queries(whole, 130, k, smallest)
        assert_top_equal(top, want, f"(three blocks, k {k})")
        assert_top_equal(run_top(torch_gpu, whole, 130, k, smallest), want, "(one call)")
        # a second query set joins, and a third whose ids lie BELOW the stored ones: equal scores then go to the newcomer
        second = padded(rng.integers(-4, 5, (20, 130)).astype(DTYPES[elem]), 192)
        third = padded(rng.integers(-4, 5, (9, 130)).astype(DTYPES[elem]), 192)
        got = run_top(torch_gpu, second, 130, k, smallest, base=1000, into=top)
        want = Q.top_queries(second, 130, k, smallest, 1000, into=want)
        assert_top_equal(got, want, "(second set)")
        assert (got[1] >= 1000).any()
        got = run_top(torch_gpu, third, 130, k, smallest, base=500, into=got)
        assert_top_equal(got, Q.top_queries(third, 130, k, smallest, 500, into=want), "(third set, ids between)")
    thr = None
    for lo, hi in ((0, 7), (7, 71), (71, 72)):
        thr = run_threshold(torch_gpu, whole[lo:hi], 130, 2, smallest, 80, base=lo, into=thr)
    assert Q.threshold_lists_equal(thr, Q.threshold_queries(whole, 130, 2, smallest, 80), 80)


@pytest.mark.parametrize("elem", [2, 1])
def test_threshold_lists(torch_gpu, elem):
    rng = np.random.default_rng(60 + elem)
    body = rng.integers(0, 10, (90, 130)).astype(DTYPES[elem])
    body[:, :10] = 9                                        # ten columns with one hit below 3, one of them with none
    body[5, :9] = 0
    tile = padded(body, 192)
    # no hits: counts 0, lists untouched
    cnt, sc, hq = run_threshold(torch_gpu, tile, 130, 50, False, 4)
    assert (cnt == 0).all() and (sc == CANARY).all() and (hq == CANARY).all()
    # cap 1: the first hit of every column and the true count
    cnt, sc, hq = run_threshold(torch_gpu, tile, 130, 8, False, 1, base=3)
    want = Q.threshold_queries(body, 130, 8, False, 1, 3)
    assert Q.threshold_lists_equal((cnt, sc, hq), want, 1) and (cnt > 1).any()
    # overflow: the true count, the lowest ids kept; slots behind a short column's count untouched
    cap = 12
    got = run_threshold(torch_gpu, tile, 130, 2, True, cap)
    want = Q.threshold_queries(body, 130, 2, True, cap)
    assert Q.threshold_lists_equal(got, want, cap)
    assert (got[0] > cap).any() and (got[0] < cap).any()
    for c in range(130):
        n = min(int(got[0][c]), cap)
        assert (got[1][c, n:] == CANARY).all() and (got[2][c, n:] == CANARY).all()
        assert got[2][c, :n].tolist() == sorted(got[2][c, :n].tolist())
    # append behind a non-zero count: the same tile again as another query set
    again = run_threshold(torch_gpu, tile, 130, 2, True, cap, base=1000, into=got)
    assert Q.threshold_lists_equal(again, Q.threshold_queries(body, 130, 2, True, cap, 1000, into=want), cap)
    assert np.array_equal(again[0], 2 * got[0])
    for c in range(130):
        n = min(int(again[0][c]), cap)
        assert (again[2][c, n:] == CANARY).all()


def test_null_workspace_equals_caller_workspace(torch_gpu):
    rng = np.random.default_rng(8)
    tile = rng.integers(-9, 10, (50, 192)).astype(np.int16)
    assert_top_equal(run_top(torch_gpu, tile, 130, 7, False, own_workspace=False), run_top(torch_gpu, tile, 130, 7, False))
    a, b = run_threshold(torch_gpu, tile, 130, 5, False, 6, own_workspace=False), run_threshold(torch_gpu, tile, 130, 5, False, 6)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


# ---- through DeviceAligner, against the oracle's matrix reduced by the helper ----------------------------------------------
def assert_not_degenerate(want_scores, k, smallest):
    """On the CPU, before the GPU is asked: at least three different best queries across the columns, and at least one column
    whose K-th place is decided by the id (its K-th and (K+1)-th best scores are equal)."""
    scores = np.asarray(want_scores, dtype=np.int64)
    best = Q.top_queries(scores, scores.shape[1], 1, smallest)[1][:, 0]
    assert len(np.unique(best)) >= 3, "fewer than three different best queries"
    ranked = np.sort(scores if smallest else -scores, axis=0)
    assert scores.shape[0] > k and (ranked[k - 1] == ranked[k]).any(), "no column whose K-th place is decided by the id"


def planted_subjects(seed, q, ns, slen, every_random=4):
    """ns subjects of slen bp: subject c is a piece of query c % nq with c % 5 edits; every fourth one is a random read."""
    nq, qlen = q.shape
    rng = np.random.default_rng(seed)
    offs = rng.integers(0, qlen - slen + 1, ns)
    src = np.stack([q[c % nq, offs[c]: offs[c] + slen] for c in range(ns)])
    s = O.mutate(src, np.arange(ns) % 5, seed + 1)
    s[every_random - 1:: every_random] = O.gen_reads(seed + 2, ns, slen)[every_random - 1:: every_random]
    return s


def _aligner(q, s, algo=B.ALGO_MYERS, **kw):
    a = B.DeviceAligner(algo, DEV, **kw)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


@functools.lru_cache(maxsize=None)
def semi_case():
    """Myers semi-global: 40 queries of 200 bp x 130 subjects of 60 bp.  Shared and never modified."""
    q = O.gen_reads(0x9A17_0001, 40, 200)
    s = planted_subjects(0x9A17_1001, q, 130, 60)
    return q, s, O.dp_edit_semiglobal(q, s)


def test_myers_semi_global_query_blocks(torch_gpu):
    q, s, want = semi_case()
    assert_not_degenerate(want, 3, False)
    cutoff, cap = -26, 6
    want_thr = Q.threshold_queries(want, 130, cutoff, False, cap)
    assert (want_thr[0] > cap).any() and (want_thr[0] < cap).any()      # overflowing and short lists
    a = _aligner(q, s, semi_global=True)
    got = _np(a.top_queries(3, block_rows=16))                 # three blocks, the last partial
    assert_top_equal(got, Q.top_queries(want, 130, 3, False), "(semi-global, three blocks)")
    assert got[0].shape == (130, 3)
    assert_top_equal(_np(a.top_queries(3)), got, "(one block)")
    thr = _np(a.threshold_queries(cutoff, cap, block_rows=16))
    a.check_faults()
    assert Q.threshold_lists_equal(thr, want_thr, cap)
    # a second query set through into=: the same queries again under other ids lose every tie
    both = _np(a.top_queries(3, block_rows=16, query_base=1000, into=a.top_queries(3, block_rows=16)))
    assert_top_equal(both, Q.top_queries(want, 130, 3, False, 1000, into=Q.top_queries(want, 130, 3, False)), "(into=)")


@functools.lru_cache(maxsize=None)
def global_case():
    """12 queries of 150 bp x 130 subjects of 150 bp: three subject groups, 62 padding columns.  Shared and never modified."""
    q = O.gen_reads(0x9A17_0002, 12, 150)
    s = planted_subjects(0x9A17_1002, q, 130, 150)
    return q, s


@pytest.mark.parametrize("kind", ["myers_global", "plus_distance", "bitpal", "banded_k8"])
def test_global_aligners_follow_their_direction(torch_gpu, kind):
    q, s = global_case()
    if kind == "myers_global":
        want, kw, algo, smallest = O.myers64(q, s), {}, B.ALGO_MYERS, False
    elif kind == "plus_distance":
        want, kw, algo, smallest = -O.myers64(q, s).astype(np.int16), {"scores": (0, 1, 1)}, B.ALGO_MYERS, True
    elif kind == "bitpal":
        want, kw, algo, smallest = O.bitpal(q, s), {"scores": (2, -3, -5)}, B.ALGO_BITPAL, False
    else:
        want, kw, algo, smallest = O.banded64(q, s, 8), {"k": 8}, B.ALGO_BANDED, True
    assert B.default_smallest(algo, kw.get("scores")) == smallest
    assert_not_degenerate(want, 3, smallest)
    a = _aligner(q, s, algo, **kw)
    assert a.ns == 192 and (a.ns // 64) % 2 == 1
    got = _np(a.top_queries(3, block_rows=5))
    a.check_faults()
    assert_top_equal(got, Q.top_queries(want, 130, 3, smallest), f"({kind})")
    cutoff = int(np.median(np.asarray(want, dtype=np.int64)))
    thr = _np(a.threshold_queries(cutoff, 5, block_rows=5))
    assert Q.threshold_lists_equal(thr, Q.threshold_queries(want, 130, cutoff, smallest, 5), 5)
    conv = B.align_top_queries(q, s, 3, algo=algo, block_rows=7, **kw)
    assert_top_equal(conv, got, "(align_top_queries)")


def test_ragged_lists_come_back_in_the_callers_order(torch_gpu):
    from test_ragged_gpu import LENS_150, by_class, make_bucket
    q, subjects, _ = make_bucket(0x9A17_0003, 6, 150, [LENS_150[(5 * i) % 16] for i in range(130)])
    want = by_class(O.dp_edit, q, subjects)
    assert_not_degenerate(want, 2, False)
    got = B.align_top_queries_ragged(q, subjects, 2, block_rows=4)
    assert_top_equal(got, Q.top_queries(want, 130, 2, False), "(ragged)")


def test_pairs_of_the_lists_align_as_the_listed_pairs(torch_gpu):
    q, s = global_case()
    q = q[:2]                                               # nq < K: unused slots exist
    a = _aligner(q, s)
    hit_scores, hit_queries = a.top_queries(3)
    ids = hit_queries.cpu().numpy()
    assert (ids[:, 2] == -1).all() and (ids[:, :2] >= 0).all()
    pq, ps = a.query_hits_as_pairs(hit_queries, subject_base=0)
    assert pq.dtype == torch_gpu.int32 and ps.dtype == torch_gpu.int64 and pq.numel() == ps.numel() == 130 * 3
    assert (ps.view(130, 3)[:, 2] == -1).all() and (pq.view(130, 3)[:, 2] == 0).all()
    distance, n_ops, cigar = _np(a.align_pairs(pq, ps))
    a.check_faults()                                        # the unused slots raised no BGSA_HIP_FAULT_PAIR
    distance, n_ops, cigar = distance.reshape(130, 3), n_ops.reshape(130, 3), cigar.reshape(130, 3, -1)
    assert (distance[:, 2] == -1).all() and (n_ops[:, 2] == 0).all()
    listed_q = ids[:, :2].reshape(-1)
    listed_s = np.repeat(np.arange(130), 2)
    d2, n2, c2 = _np(a.align_pairs(listed_q, listed_s))
    assert np.array_equal(distance[:, :2].reshape(-1), d2) and np.array_equal(n_ops[:, :2].reshape(-1), n2)
    assert np.array_equal(cigar[:, :2].reshape(260, -1), c2)
    assert np.array_equal(distance[:, :2], -hit_scores.cpu().numpy()[:, :2])
    # with a subject_base the ids move with it
    pq3, ps3 = a.query_hits_as_pairs(hit_queries, subject_base=700)
    assert np.array_equal(ps3.cpu().numpy().reshape(130, 3)[:, 0], 700 + np.arange(130)) and (ps3.view(130, 3)[:, 2] == -1).all()


def test_read_placement_windows_as_queries_reads_as_subjects(torch_gpu):
    windows = np.concatenate([np.frombuffer(b"TTGACCATGCAAGTCCGATTACGGATCCTA", np.uint8)[None, :], O.gen_reads(0x9A17_0004, 5, 30)])
    reads = np.stack([np.frombuffer(b"AGTCCGTTTACG", np.uint8),          # window 0 [11:23] with one base changed
                      windows[2, 0:12],                                    # at the window's start, exact
                      windows[3, 18:30],                                   # at the window's end, exact
                      np.concatenate([windows[4, 5:11], windows[4, 12:18]]),        # one base of the window skipped
                      np.concatenate([windows[5, 9:15], [ord("A") if windows[5, 14] != ord("A") else ord("C")], windows[5, 15:20]]),
                      windows[1, 3:15]]).astype(np.uint8)
    k = 2
    scores, ids, spans, cigars = B.trace_top_queries(windows, reads, k, B.ALGO_MYERS, semi_global=True)
    assert scores.shape == (6, k) and ids.shape == (6, k) and spans.shape == (6, k, 4)
    want = O.dp_edit_semiglobal(windows, reads)
    assert_top_equal((scores, ids), Q.top_queries(want, 6, k, False), "(placement)")
    assert ids[:, 0].tolist() == [0, 2, 3, 4, 5, 1]
    # the INTEGRATION example
    assert scores[0, 0] == -1 and spans[0, 0].tolist() == [11, 23, 0, 12] and cigars[0][0] == "6=1X5="
    assert spans[1, 0].tolist() == [0, 12, 0, 12] and cigars[1][0] == "12=" and spans[2, 0].tolist() == [18, 30, 0, 12]
    # every listed pair against the reference walk, and against trace_pairs on the same pairs
    canon = T.canonical(windows[ids.reshape(-1)], reads[np.repeat(np.arange(6), k)], T.FREE_QUERY, T.UNIT)
    for p, (score, span, runs) in enumerate(canon):
        c, r = divmod(p, k)
        assert (scores[c, r], tuple(spans[c, r].tolist()), cigars[c][r]) == (score, span, A.to_string(runs)), (c, r)
    a = _aligner(windows, reads, semi_global=True)
    sc, sp, n_ops, cigar = a.trace_pairs(ids.reshape(-1), np.repeat(np.arange(6), k))
    a.check_faults()
    assert np.array_equal(sc.cpu().numpy().reshape(6, k), scores) and np.array_equal(sp.cpu().numpy().reshape(6, k, 4), spans)
    assert B.cigar_strings(n_ops, cigar) == [cigars[c][r] for c in range(6) for r in range(k)]
    # fewer windows than K: the unused slot has no script and no span
    scores1, ids1, spans1, cigars1 = B.trace_top_queries(windows[:1], reads[:1], 2, B.ALGO_MYERS, semi_global=True)
    assert ids1.tolist() == [[0, -1]] and cigars1[0] == ["6=1X5=", None] and spans1[0, 1].tolist() == [-1, -1, -1, -1]
    assert scores1[0, 1] == Q.INT32_MIN


def test_the_documented_read_placement_example(torch_gpu):
    windows = np.stack([np.frombuffer(b"TTGACCATGCAAGTCCGATTACGGATCCTA", np.uint8), np.frombuffer(b"GGCATTCGAGCTTAACGTGCCAATGGTCAT", np.uint8)])
    reads = np.stack([np.frombuffer(b"AGTCCGTTTACG", np.uint8), np.frombuffer(b"TTAACGTGCCAA", np.uint8)])
    scores, queries, spans, cigars = B.trace_top_queries(windows, reads, 1, B.ALGO_MYERS, semi_global=True)
    assert queries[:, 0].tolist() == [0, 1] and scores[:, 0].tolist() == [-1, 0]
    assert spans[:, 0].tolist() == [[11, 23, 0, 12], [11, 23, 0, 12]] and cigars == [["6=1X5="], ["12="]]

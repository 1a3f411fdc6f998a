"""Hit selection on the MI355X: bgsa_hip_top_hits_dev / bgsa_hip_threshold_hits_dev on synthetic tiles, and
DeviceAligner.top_hits / threshold_hits end to end — everything bit for bit against tests/hits_reference.py."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import hits_reference as H  # noqa: E402

pytestmark = pytest.mark.gpu

EUNSUPPORTED = -2
DTYPES = {2: np.int16, 1: np.int8}


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def _stream(torch):
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def run_top(torch, tile, valid, k, smallest, base=0, into=None, own_workspace=True, expect=0):
    """tile: numpy [nq, stride] int16 / int8 (or a device tensor) -> numpy (scores, subjects)."""
    L = B.lib()
    d_tile = tile if torch.is_tensor(tile) else torch.from_numpy(np.ascontiguousarray(tile)).cuda()
    nq, stride = d_tile.shape
    if into is None:
        sc = torch.full((nq, max(k, 1)), 12345, dtype=torch.int32, device="cuda")
        sj = torch.full((nq, max(k, 1)), 12345, dtype=torch.int64, device="cuda")
    else:
        sc, sj = torch.from_numpy(into[0]).cuda(), torch.from_numpy(into[1]).cuda()
    ws, ws_bytes = None, 0
    if own_workspace:
        ws_bytes = int(L.bgsa_hip_hits_workspace_bytes(nq, stride, d_tile.element_size(), min(max(k, 1), 64)))
        work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        ws = work.data_ptr()
    rc = L.bgsa_hip_top_hits_dev(d_tile.data_ptr(), d_tile.element_size(), nq, stride, valid, base, k, int(smallest),
                                 int(into is not None), sc.data_ptr(), sj.data_ptr(), ws, ws_bytes, _stream(torch))
    assert rc == expect, L.bgsa_hip_last_error()
    torch.cuda.synchronize()
    return sc.cpu().numpy(), sj.cpu().numpy()


def run_threshold(torch, tile, valid, cutoff, smallest, cap, base=0, into=None, own_workspace=True):
    L = B.lib()
    d_tile = tile if torch.is_tensor(tile) else torch.from_numpy(np.ascontiguousarray(tile)).cuda()
    nq, stride = d_tile.shape
    if into is None:
        cnt = torch.full((nq,), 777, dtype=torch.int32, device="cuda")
        sc = torch.full((nq, cap), 12345, dtype=torch.int32, device="cuda")
        sj = torch.full((nq, cap), 12345, dtype=torch.int64, device="cuda")
    else:
        cnt, sc, sj = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in into)
    ws, ws_bytes = None, 0
    if own_workspace:
        ws_bytes = int(L.bgsa_hip_hits_workspace_bytes(nq, stride, d_tile.element_size(), 1))
        work = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
        ws = work.data_ptr()
    B.check(L.bgsa_hip_threshold_hits_dev(d_tile.data_ptr(), d_tile.element_size(), nq, stride, valid, base, cutoff, int(smallest),
                                          int(into is not None), cap, cnt.data_ptr(), sc.data_ptr(), sj.data_ptr(), ws, ws_bytes,
                                          _stream(torch)), "threshold_hits_dev")
    torch.cuda.synchronize()
    return cnt.cpu().numpy(), sc.cpu().numpy(), sj.cpu().numpy()


def assert_top_equal(got, want, what=""):
    assert np.array_equal(got[0], want[0]), f"scores differ {what}"
    assert np.array_equal(got[1], want[1]), f"subjects differ {what}"


# ---- synthetic tiles straight into the C ABI --------------------------------------------------------------------------
def synthetic_tiles(elem):
    """name -> (tile [nq, stride], valid_count).  The columns behind valid_count hold the best possible score of BOTH
    directions alternately (and the extremes of the type), so a kernel that reads them shows it."""
    dt = DTYPES[elem]
    lo, hi = np.iinfo(dt).min, np.iinfo(dt).max
    rng = np.random.default_rng(100 + elem)
    out = {}

    def padded(body, stride):
        nq, valid = body.shape
        tile = np.empty((nq, stride), dtype=dt)
        tile[:, :valid] = body
        pad = np.where(np.arange(stride - valid) % 2 == 0, hi, lo).astype(dt)
        tile[:, valid:] = pad
        return tile, valid

    out["all_equal"] = padded(np.full((3, 1000), 7, dtype=dt), 1024)
    span = hi - lo + 1
    asc = (lo + np.arange(span)).astype(dt)[None, :].repeat(2, axis=0)       # strictly ascending over the whole type
    if elem == 2:
        out["ascending"] = padded(asc[:, 20000:20000 + 9001], 9024)
        out["descending"] = padded(asc[:, ::-1][:, 1000:1000 + 9001].copy(), 9024)
    else:
        out["ascending"] = padded(asc[:, 3:250], 256)
        out["descending"] = padded(asc[:, ::-1][:, 3:250].copy(), 256)
    out["two_values"] = padded(rng.integers(0, 2, (5, 2999)).astype(dt) * 3 - 1, 3008)
    ext = rng.integers(-20, 20, (4, 1237)).astype(dt)
    ext[0, 17], ext[0, 900], ext[1, 5], ext[2, 1236], ext[2, 0], ext[3, 64] = lo, hi, hi, lo, hi, lo
    ext[3, 65] = lo
    out["extremes"] = padded(ext, 1280)
    out["ragged_valid"] = padded(rng.integers(-9, 9, (7, 64 * 3 + 37)).astype(dt), 64 * 4)          # valid % 64 != 0
    out["wide_stride"] = padded(rng.integers(-9, 9, (3, 500)).astype(dt), 4096)                      # row_stride >> valid
    out["odd_stride"] = padded(rng.integers(-9, 9, (3, 1001)).astype(dt), 1003)                      # rows off the 16-byte grid
    out["many_segments"] = padded(rng.integers(-50, 50, (2, 70_000)).astype(dt), 70_016)             # several segments per row
    return out


@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("smallest", [False, True])
def test_top_hits_on_synthetic_tiles(torch_gpu, elem, smallest):
    for name, (tile, valid) in synthetic_tiles(elem).items():
        for k in (1, 5, 64):
            got = run_top(torch_gpu, tile, valid, k, smallest, base=1000)
            assert_top_equal(got, H.top_hits(tile, valid, k, smallest, 1000), f"({name}, K={k})")
            assert (got[1] < 1000 + valid).all(), f"a padding column appeared ({name}, K={k})"


@pytest.mark.parametrize("elem", [2, 1])
def test_top_hits_sentinel_slots_when_k_exceeds_valid_count(torch_gpu, elem):
    rng = np.random.default_rng(1)
    tile = rng.integers(-5, 5, (3, 64)).astype(DTYPES[elem])
    tile[:, 9:] = np.iinfo(DTYPES[elem]).max
    for smallest in (False, True):
        tile[:, 9:] = np.iinfo(DTYPES[elem]).min if smallest else np.iinfo(DTYPES[elem]).max
        got = run_top(torch_gpu, tile, 9, 64, smallest)
        assert_top_equal(got, H.top_hits(tile, 9, 64, smallest))
        assert (got[1][:, 9:] == -1).all() and (got[0][:, 9:] == H.worst(smallest)).all()
        assert (got[1][:, :9] >= 0).all()


def test_top_hits_k_65_is_unsupported_and_touches_nothing(torch_gpu):
    tile = np.zeros((2, 128), dtype=np.int16)
    sc, sj = run_top(torch_gpu, tile, 100, 65, False, expect=EUNSUPPORTED)
    assert (sc == 12345).all() and (sj == 12345).all()
    assert b"1..64" in B.lib().bgsa_hip_last_error()


@pytest.mark.parametrize("elem", [2, 1])
@pytest.mark.parametrize("smallest", [False, True])
def test_threshold_hits_on_synthetic_tiles(torch_gpu, elem, smallest):
    for name, (tile, valid) in synthetic_tiles(elem).items():
        body = tile[:, :valid].astype(np.int64)
        for cutoff in (int(np.median(body)), int(body.max()) if not smallest else int(body.min())):
            for cap in (valid, 3):
                got = run_threshold(torch_gpu, tile, valid, cutoff, smallest, cap, base=50)
                want = H.threshold_hits(tile, valid, cutoff, smallest, cap, 50)
                assert H.threshold_lists_equal(got, want, cap), (name, cutoff, cap)
                # slots behind a row's hits are left as they were
                for r in range(tile.shape[0]):
                    assert (got[2][r, min(int(want[0][r]), cap):] == 12345).all(), (name, cutoff, cap)


def test_library_scratch_equals_caller_workspace(torch_gpu):
    tile, valid = synthetic_tiles(2)["many_segments"]
    assert_top_equal(run_top(torch_gpu, tile, valid, 10, False, own_workspace=False), H.top_hits(tile, valid, 10, False))
    got = run_threshold(torch_gpu, tile, valid, 45, False, 100, own_workspace=False)
    assert H.threshold_lists_equal(got, H.threshold_hits(tile, valid, 45, False, 100), 100)


def test_selection_is_safe_inside_a_stream_capture(torch_gpu):
    torch = torch_gpu
    tile, valid = synthetic_tiles(2)["many_segments"]
    L = B.lib()
    d_tile = torch.from_numpy(tile).cuda()
    nq, stride = d_tile.shape
    work = torch.empty(int(L.bgsa_hip_hits_workspace_bytes(nq, stride, 2, 10)), dtype=torch.uint8, device="cuda")
    sc = torch.zeros((nq, 10), dtype=torch.int32, device="cuda")
    sj = torch.zeros((nq, 10), dtype=torch.int64, device="cuda")
    cnt = torch.zeros((nq,), dtype=torch.int32, device="cuda")
    tsc = torch.zeros((nq, 50), dtype=torch.int32, device="cuda")
    tsj = torch.zeros((nq, 50), dtype=torch.int64, device="cuda")
    work2 = torch.empty_like(work)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        s = _stream(torch)
        B.check(L.bgsa_hip_top_hits_dev(d_tile.data_ptr(), 2, nq, stride, valid, 0, 10, 0, 0, sc.data_ptr(), sj.data_ptr(),
                                        work.data_ptr(), work.numel(), s), "top_hits_dev (capture)")
        B.check(L.bgsa_hip_threshold_hits_dev(d_tile.data_ptr(), 2, nq, stride, valid, 0, 45, 0, 0, 50, cnt.data_ptr(), tsc.data_ptr(),
                                              tsj.data_ptr(), work2.data_ptr(), work2.numel(), s), "threshold_hits_dev (capture)")
    g.replay()
    torch.cuda.synchronize()
    assert_top_equal((sc.cpu().numpy(), sj.cpu().numpy()), H.top_hits(tile, valid, 10, False))
    assert H.threshold_lists_equal((cnt.cpu().numpy(), tsc.cpu().numpy(), tsj.cpu().numpy()), H.threshold_hits(tile, valid, 45, False, 50), 50)


# ---- the size case: 16 x 1,000,000 int16 --------------------------------------------------------------------------------
def _size_tile(torch):
    gen = torch.Generator(device="cpu")
    gen.manual_seed(0xB65A)
    tile = torch.randint(-150, 1, (16, 1_000_064), dtype=torch.int16, generator=gen)
    tile[:, 1_000_000:] = 32767                # the padding columns: the best possible score
    return tile


def test_size_case_top_k_and_threshold_are_exact_and_deterministic(torch_gpu):
    torch = torch_gpu
    host = _size_tile(torch)
    tile = host.numpy()
    d_tile = host.cuda()
    valid = 1_000_000
    before = d_tile.clone()
    runs = [run_top(torch, d_tile, valid, 64, False, base=5_000_000_000) for _ in range(2)]
    assert runs[0][0].tobytes() == runs[1][0].tobytes() and runs[0][1].tobytes() == runs[1][1].tobytes()
    assert_top_equal(runs[0], H.top_hits(tile, valid, 64, False, 5_000_000_000), "(size case, largest)")
    assert_top_equal(run_top(torch, d_tile, valid, 64, True), H.top_hits(tile, valid, 64, True), "(size case, smallest)")
    cap = 64
    thr = [run_threshold(torch, d_tile, valid, -1, False, cap, base=7) for _ in range(2)]      # ~1.3 % of the columns
    assert all(a.tobytes() == b.tobytes() for a, b in zip(thr[0], thr[1]))
    want = H.threshold_hits(tile, valid, -1, False, cap, 7)
    assert H.threshold_lists_equal(thr[0], want, cap) and (want[0] > cap).all()               # every row overflows: true counts
    cap = 20_000
    got = run_threshold(torch, d_tile, valid, -149, True, cap)
    assert H.threshold_lists_equal(got, H.threshold_hits(tile, valid, -149, True, cap), cap)
    assert torch.equal(d_tile, before)         # selection only reads the tile


# ---- end to end: 32 queries x 20,000 random subjects, eight planted mutants per query at 0..7 edits ---------------------
NQ, NS, PLANT = 32, 20_000, 8


@pytest.fixture(scope="module")
def planted(oracle):
    q = oracle.gen_reads(0xB175_0001, NQ, 150)
    s = oracle.gen_reads(0xB175_1001, NS, 150)
    where = {}
    rng = np.random.default_rng(77)
    slots = rng.permutation(NS)[: NQ * PLANT].reshape(NQ, PLANT)
    for i in range(NQ):
        s[slots[i]] = oracle.mutate(np.repeat(q[i: i + 1], PLANT, axis=0), np.arange(PLANT), 1000 + i)
        where[i] = sorted(int(x) for x in slots[i])
    return q, s, where


def _aligner(q, s, algo=B.ALGO_MYERS, **kw):
    a = B.DeviceAligner(algo, "cuda:0", **kw)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _np(tensors):
    return tuple(t.cpu().numpy() for t in tensors)


@pytest.mark.parametrize("mode", ["global", "semi_global", "plus_distance"])
def test_myers_top_hits_end_to_end(torch_gpu, oracle, planted, mode):
    q, s, where = planted
    if mode == "global":
        a, want_scores, smallest = _aligner(q, s), oracle.myers64(q, s), False
    elif mode == "semi_global":
        a, want_scores, smallest = _aligner(q, s, semi_global=True), oracle.dp_edit_semiglobal(q, s), False
    else:
        a, want_scores, smallest = _aligner(q, s, scores=(0, 1, 1)), -oracle.myers64(q, s).astype(np.int16), True
    got = _np(a.top_hits(10))
    a.check_faults()
    assert got[0].dtype == np.int32 and got[1].dtype == np.int64
    assert_top_equal(got, H.top_hits(want_scores, NS, 10, smallest), f"({mode})")
    if mode != "semi_global":
        for i in range(NQ):     # the eight planted mutants (at most 7 edits) beat every random read
            assert sorted(got[1][i, :PLANT].tolist()) == where[i]
    ns_padded = a.ns
    assert ns_padded % 64 == 0 and (got[1] < NS).all()


def test_bitpal_top_hits_end_to_end(torch_gpu, oracle, planted):
    q, s, _ = planted
    a = _aligner(q, s, B.ALGO_BITPAL, scores=(2, -3, -5))
    got = _np(a.top_hits(10))
    a.check_faults()
    assert_top_equal(got, H.top_hits(oracle.bitpal(q, s), NS, 10, False), "(BitPAl 2/-3/-5)")


def test_banded_threshold_hits_end_to_end(torch_gpu, oracle, planted):
    q, s, where = planted
    a = _aligner(q, s, B.ALGO_BANDED, k=8)
    cap = 32
    got = _np(a.threshold_hits(8, cap))
    a.check_faults()
    want = H.threshold_hits(oracle.banded64(q, s, 8), NS, 8, True, cap)
    assert H.threshold_lists_equal(got, want, cap)
    dist = oracle.banded64(q, s, 8)
    for i in range(NQ):
        n = int(got[0][i])
        found = got[2][i, :n].tolist()
        # exactly the planted pairs, ascending, and no random read.  mutate() keeps the length: after e edits with i
        # insertions and d deletions it cuts or pads |i - d| <= e characters at the end, so a mutant lies within
        # e + |i - d| <= 2e of its query.  The mutants at 0..4 edits are therefore always within k = 8 (at least 5 per
        # query); one at 5..7 edits may lie beyond it, and then the oracle's filter rejects it too.
        assert found == sorted(found) and found == [j for j in where[i] if dist[i, j] <= 8]
        assert 5 <= n <= PLANT and set(found) <= set(where[i])
        assert (got[1][i, :n] <= 8).all() and got[1][i, :n].min() == 0
    # and the filter's own top-K: smallest distance first
    assert_top_equal(_np(a.top_hits(10)), H.top_hits(oracle.banded64(q, s, 8), NS, 10, True), "(banded top-K)")


def test_query_blocks_equal_one_block(torch_gpu, planted):
    q, s, _ = planted
    a = _aligner(q, s)
    one = _np(a.top_hits(10, block_rows=1000))
    five = _np(a.top_hits(10, block_rows=5))         # 32 queries: six blocks of 5 and a last one of 2
    assert_top_equal(five, one)
    t1 = _np(a.threshold_hits(-60, 16, block_rows=1000))
    t5 = _np(a.threshold_hits(-60, 16, block_rows=5))
    assert H.threshold_lists_equal(t5, t1, 16) and (t1[0] >= PLANT).all()


def test_subject_buckets_accumulate_to_the_whole_bucket(torch_gpu, oracle, planted):
    q, s, _ = planted
    whole = _aligner(q, s)
    want_top = _np(whole.top_hits(10))
    cap = 40
    want_thr = _np(whole.threshold_hits(-68, cap))
    scores = oracle.myers64(q, s)
    assert_top_equal(want_top, H.top_hits(scores, NS, 10, False))
    assert H.threshold_lists_equal(want_thr, H.threshold_hits(scores, NS, -68, False, cap), cap)
    top = thr = None
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0")
    a.set_queries(q)
    for lo, hi in ((0, 7_001), (7_001, 7_100), (7_100, NS)):     # three unequal buckets, none a multiple of 64
        a.set_subjects(s[lo:hi])
        top = a.top_hits(10, subject_base=lo, into=top)
        thr = a.threshold_hits(-68, cap, subject_base=lo, into=thr)
    a.check_faults()
    assert_top_equal(_np(top), want_top, "(three buckets)")
    assert H.threshold_lists_equal(_np(thr), want_thr, cap)
    with pytest.raises(B.BgsaHipError):
        a.top_hits(10, into=(top[0], top[1][:, :5]))


def test_threshold_overflow_keeps_true_counts_and_lowest_hits(torch_gpu, oracle, planted):
    q, s, _ = planted
    a = _aligner(q, s)
    scores = oracle.myers64(q, s)
    cutoff = int(np.sort(scores, axis=1)[:, -200].min())          # at least 200 hits in every row
    got = _np(a.threshold_hits(cutoff, 50))
    want = H.threshold_hits(scores, NS, cutoff, False, 50)
    assert (want[0] >= 200).all() and H.threshold_lists_equal(got, want, 50)
    full = H.threshold_hits(scores, NS, cutoff, False, NS)
    for i in range(NQ):
        assert got[2][i].tolist() == full[2][i, :50].tolist()        # the 50 lowest-indexed hits


def test_scoring_is_untouched_by_selection(torch_gpu, oracle, planted):
    q, s, _ = planted
    a = _aligner(q, s)
    tile = a.score()
    before = tile.clone()
    L = B.lib()
    sc = torch_gpu.empty((NQ, 10), dtype=torch_gpu.int32, device="cuda")
    sj = torch_gpu.empty((NQ, 10), dtype=torch_gpu.int64, device="cuda")
    B.check(L.bgsa_hip_top_hits_dev(tile.data_ptr(), 2, NQ, a.ns, a.ns_real, 0, 10, 0, 0, sc.data_ptr(), sj.data_ptr(), None, 0,
                                    _stream(torch_gpu)), "top_hits_dev")
    cnt = torch_gpu.empty((NQ,), dtype=torch_gpu.int32, device="cuda")
    B.check(L.bgsa_hip_threshold_hits_dev(tile.data_ptr(), 2, NQ, a.ns, a.ns_real, 0, -60, 0, 0, 10, cnt.data_ptr(), sc.data_ptr(),
                                          sj.data_ptr(), None, 0, _stream(torch_gpu)), "threshold_hits_dev")
    torch_gpu.cuda.synchronize()
    assert torch_gpu.equal(tile, before)
    assert np.array_equal(tile[:, :NS].cpu().numpy(), oracle.myers64(q, s))
    assert np.array_equal(a.score()[:, :NS].cpu().numpy(), oracle.myers64(q, s))      # and scoring still works afterwards
    assert L.bgsa_hip_stream_faults(1) == 0


def test_align_top_hits_convenience(torch_gpu, oracle, planted):
    q, s, _ = planted
    got = B.align_top_hits(q[:5], s[:3000], 7)
    assert_top_equal(got, H.top_hits(oracle.myers64(q[:5], s[:3000]), 3000, 7, False))

"""Hit lists per subject without a GPU: the C ABI's argument checks (they come before any HIP call), the workspace size, and
the numpy reference helper against a brute-force loop."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import query_hits_reference as Q  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
INT32_MAX = 2 ** 31 - 1
P = 0x10000   # a non-null "device pointer": every call below must fail before it is looked at


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


def _top(L, tile=P, elem=2, nq=4, stride=128, valid=100, base=0, k=10, smallest=0, acc=0, sc=P, hq=P, ws=None, ws_bytes=0):
    return L.bgsa_hip_top_queries_dev(tile, elem, nq, stride, valid, base, k, smallest, acc, sc, hq, ws, ws_bytes, None)


def _thr(L, tile=P, elem=2, nq=4, stride=128, valid=100, base=0, cutoff=0, smallest=0, acc=0, cap=8, cnt=P, sc=P, hq=P, ws=None,
         ws_bytes=0):
    return L.bgsa_hip_threshold_queries_dev(tile, elem, nq, stride, valid, base, cutoff, smallest, acc, cap, cnt, sc, hq, ws, ws_bytes, None)


def _refused(L, rc, want=EINVAL):
    """The call was refused with `want` and said why."""
    return rc == want and len(L.bgsa_hip_last_error()) > 0


def test_symbols_are_declared_and_exported(L):
    names = B.declared_symbols()
    for fn in ("bgsa_hip_query_hits_workspace_bytes", "bgsa_hip_top_queries_dev", "bgsa_hip_threshold_queries_dev"):
        assert fn in names and hasattr(L, fn)
    for method in ("top_queries", "threshold_queries", "query_hits_as_pairs"):
        assert callable(getattr(B.DeviceAligner, method))
    for fn in ("align_top_queries", "align_top_queries_ragged", "trace_top_queries"):
        assert callable(getattr(B, fn))


def test_top_queries_argument_checks_come_before_any_hip_call(L):
    assert _refused(L, _top(L, tile=None))
    assert _refused(L, _top(L, sc=None)) and _refused(L, _top(L, hq=None))
    assert _refused(L, _top(L, nq=0)) and _refused(L, _top(L, nq=-3))
    assert _refused(L, _top(L, stride=0)) and _refused(L, _top(L, stride=-128))
    assert _refused(L, _top(L, valid=129))                     # valid_count > row_stride
    assert _refused(L, _top(L, valid=-1))
    assert _refused(L, _top(L, elem=4)) and _refused(L, _top(L, elem=0))
    assert _refused(L, _top(L, base=-1))
    assert _refused(L, _top(L, base=INT32_MAX - 3))            # query_base + n_queries beyond INT32_MAX
    assert b"query ids" in L.bgsa_hip_last_error()
    assert _refused(L, _top(L, ws=P, ws_bytes=8))              # a workspace that is too small
    assert b"workspace" in L.bgsa_hip_last_error()
    for k in (0, -1, 65, 1000):
        assert _refused(L, _top(L, k=k), EUNSUPPORTED)
    assert b"1..64" in L.bgsa_hip_last_error()


def test_threshold_queries_argument_checks_come_before_any_hip_call(L):
    assert _refused(L, _thr(L, tile=None))
    assert _refused(L, _thr(L, cnt=None)) and _refused(L, _thr(L, sc=None)) and _refused(L, _thr(L, hq=None))
    assert _refused(L, _thr(L, nq=0)) and _refused(L, _thr(L, stride=-1))
    assert _refused(L, _thr(L, cap=0)) and _refused(L, _thr(L, cap=-5))
    assert _refused(L, _thr(L, valid=129)) and _refused(L, _thr(L, valid=-1))
    assert _refused(L, _thr(L, elem=3))
    assert _refused(L, _thr(L, base=-1)) and _refused(L, _thr(L, base=INT32_MAX - 3))
    assert _refused(L, _thr(L, ws=P, ws_bytes=8))


def test_workspace_bytes_never_shrinks_when_an_argument_grows(L):
    f = L.bgsa_hip_query_hits_workspace_bytes
    assert f(0, 100, 2, 10) == 0 and f(4, 0, 2, 10) == 0 and f(4, 100, 3, 10) == 0 and f(4, 100, 0, 10) == 0 and f(4, 100, 2, 0) == 0
    nqs = [1, 2, 3, 7, 16, 31, 32, 33, 100, 999, 1000, 1001, 4096, 32768, 100_000, 1_000_000]
    strides = [1, 63, 64, 1000, 8191, 8192, 8193, 20_032, 100_000, 1_000_064, 10_000_000, (1 << 31) - 1]
    for elem in (1, 2):
        table = np.array([[f(nq, st, elem, 10) for st in strides] for nq in nqs], dtype=np.float64)
        assert (table > 0).all()
        assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    for nq, st in ((16, 1_000_064), (1000, 1_000_064), (5, 100)):
        assert f(nq, st, 1, 10) <= f(nq, st, 2, 10)
        sizes = [f(nq, st, 2, k) for k in range(1, 66)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the headline block: 1,000 x 1M int16 = 2 GB of scores needs well under 1 % of that
    assert f(1000, 1_000_064, 2, 64) < 20 * 1024 * 1024


def test_reference_helper_agrees_with_a_brute_force_loop():
    rng = np.random.default_rng(15)
    for trial in range(40):
        nq, ns = int(rng.integers(1, 9)), int(rng.integers(1, 6))
        valid = int(rng.integers(1, ns + 1))
        tile = rng.integers(-2, 2, (nq, ns)).astype(np.int16)       # four distinct values: ties everywhere
        for k in (1, 3, nq, nq + 2):
            for smallest in (False, True):
                base = int(rng.integers(0, 1000))
                got = Q.top_queries(tile, valid, k, smallest, base)
                want = Q.brute_top_queries(tile, valid, k, smallest, base)
                assert got[1].dtype == np.int32 and got[0].shape == (valid, k)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, k, smallest)
                # accumulate: a second tile with ids BELOW the stored ones — equal scores then go to the newcomer
                more = rng.integers(-2, 2, (3, ns)).astype(np.int16)
                low = max(0, base - 3)
                got2 = Q.top_queries(more, valid, k, smallest, low, into=got)
                want2 = Q.brute_top_queries(more, valid, k, smallest, low, into=want)
                assert np.array_equal(got2[0], want2[0]) and np.array_equal(got2[1], want2[1]), (trial, k, smallest, "accumulate")
    # ties go to the smaller query id; padding columns never appear; unused slots are (-1, worst)
    tile = np.array([[5, 9], [7, 9], [7, 9], [5, 9]], dtype=np.int16)
    s, q = Q.top_queries(tile, 1, 5, False, query_base=100)
    assert q.tolist() == [[101, 102, 100, 103, -1]] and s.tolist() == [[7, 7, 5, 5, Q.INT32_MIN]]
    s, q = Q.top_queries(tile, 1, 2, True)
    assert q.tolist() == [[0, 3]] and s.tolist() == [[5, 5]]


def test_reference_threshold_lists_overflow_and_append():
    tile = np.array([3, 1, 4, 1, 5, 9, 2, 6], dtype=np.int8).reshape(8, 1).repeat(2, axis=1)
    tile[:, 1] = 100                                                # a padding column: never listed
    c, s, q = Q.threshold_queries(tile, 1, 2, True, 4, query_base=10)
    assert c.tolist() == [3] and s[0, :3].tolist() == [1, 1, 2] and q[0, :3].tolist() == [11, 13, 16] and q.dtype == np.int32
    c, s, q = Q.threshold_queries(tile, 1, 4, False, 2)             # overflow: true count, the lowest-indexed hits
    assert c.tolist() == [4] and q.tolist() == [[2, 4]] and s.tolist() == [[4, 5]]
    # append: a second query set lands behind the first one's count, and what lies beyond the cap is only counted
    first = Q.threshold_queries(tile, 1, 5, False, 4)
    assert first[0].tolist() == [3] and first[2].tolist() == [[4, 5, 7, -1]]
    c, s, q = Q.threshold_queries(tile, 1, 5, False, 4, query_base=1000, into=first)
    assert c.tolist() == [6] and q.tolist() == [[4, 5, 7, 1004]] and s.tolist() == [[5, 9, 6, 5]]
    # three query blocks accumulated = the whole tile at once, for both selections
    rng = np.random.default_rng(19)
    whole = rng.integers(-3, 3, (50, 3)).astype(np.int16)
    top = thr = None
    for lo, hi in ((0, 17), (17, 18), (18, 50)):
        top = Q.top_queries(whole[lo:hi], 3, 6, False, query_base=lo, into=top)
        thr = Q.threshold_queries(whole[lo:hi], 3, 1, False, 50, query_base=lo, into=thr)
    want = Q.top_queries(whole, 3, 6, False)
    assert np.array_equal(top[0], want[0]) and np.array_equal(top[1], want[1])
    assert Q.threshold_lists_equal(thr, Q.threshold_queries(whole, 3, 1, False, 50), 50)

"""Hit selection without a GPU: the C ABI's argument checks (they come before any HIP call), the workspace size, the
numpy reference helper against a brute-force loop, and ShardedAligner.run_hits under gloo with the oracle as hits_fn."""
import ctypes
import os
import socket
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import hits_reference as H  # noqa: E402
from bgsa_amd.multi_gpu import ShardedAligner, merge_hits, plan_shards  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must fail before it is looked at


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


def _top(L, tile=P, elem=2, nq=4, stride=128, valid=100, base=0, k=10, smallest=0, acc=0, sc=P, sj=P, ws=None, ws_bytes=0):
    return L.bgsa_hip_top_hits_dev(tile, elem, nq, stride, valid, base, k, smallest, acc, sc, sj, ws, ws_bytes, None)


def _thr(L, tile=P, elem=2, nq=4, stride=128, valid=100, base=0, cutoff=0, smallest=0, acc=0, cap=8, cnt=P, sc=P, sj=P, ws=None,
         ws_bytes=0):
    return L.bgsa_hip_threshold_hits_dev(tile, elem, nq, stride, valid, base, cutoff, smallest, acc, cap, cnt, sc, sj, ws, ws_bytes, None)


def test_symbols_are_declared_and_exported(L):
    names = B.declared_symbols()
    for fn in ("bgsa_hip_hits_workspace_bytes", "bgsa_hip_top_hits_dev", "bgsa_hip_threshold_hits_dev"):
        assert fn in names and hasattr(L, fn)


def test_top_hits_argument_checks_come_before_any_hip_call(L):
    assert _top(L, tile=None) == EINVAL
    assert _top(L, sc=None) == EINVAL and _top(L, sj=None) == EINVAL
    assert _top(L, nq=0) == EINVAL and _top(L, nq=-3) == EINVAL
    assert _top(L, stride=0) == EINVAL
    assert _top(L, valid=129) == EINVAL                       # valid_count > row_stride
    assert _top(L, valid=-1) == EINVAL
    assert _top(L, stride=1 << 31, valid=1 << 31) == EINVAL   # valid_count >= 2^31
    assert _top(L, elem=4) == EINVAL and _top(L, elem=0) == EINVAL
    assert _top(L, base=-1) == EINVAL and _top(L, base=1 << 46) == EINVAL
    assert _top(L, ws=P, ws_bytes=8) == EINVAL                # a workspace that is too small
    assert b"workspace" in L.bgsa_hip_last_error()
    for k in (0, -1, 65, 1000):
        assert _top(L, k=k) == EUNSUPPORTED
    assert b"1..64" in L.bgsa_hip_last_error()


def test_threshold_hits_argument_checks_come_before_any_hip_call(L):
    assert _thr(L, tile=None) == EINVAL
    assert _thr(L, cnt=None) == EINVAL and _thr(L, sc=None) == EINVAL and _thr(L, sj=None) == EINVAL
    assert _thr(L, nq=0) == EINVAL and _thr(L, stride=-1) == EINVAL
    assert _thr(L, cap=0) == EINVAL and _thr(L, cap=-5) == EINVAL
    assert _thr(L, valid=129) == EINVAL
    assert _thr(L, stride=(1 << 31) + 64, valid=1 << 31) == EINVAL
    assert _thr(L, elem=3) == EINVAL
    assert _thr(L, ws=P, ws_bytes=8) == EINVAL


def test_workspace_bytes_never_shrinks_when_an_argument_grows(L):
    f = L.bgsa_hip_hits_workspace_bytes
    assert f(0, 100, 2, 10) == 0 and f(4, 0, 2, 10) == 0 and f(4, 100, 3, 10) == 0 and f(4, 100, 2, 0) == 0
    nqs = [1, 2, 3, 7, 16, 31, 32, 33, 100, 999, 1000, 1001, 4096, 8191, 8192, 32767, 32768, 32769, 100_000, 1_000_000]
    strides = [1, 63, 64, 1000, 8191, 8192, 8193, 20_032, 100_000, 1_000_064, 10_000_000, (1 << 31) - 1]
    table = np.array([[f(nq, st, 2, 10) for st in strides] for nq in nqs], dtype=np.float64)
    assert (table > 0).all()
    assert (np.diff(table, axis=0) >= 0).all() and (np.diff(table, axis=1) >= 0).all()
    for nq, st in ((16, 1_000_064), (1000, 1_000_064), (5, 100)):
        assert f(nq, st, 1, 10) <= f(nq, st, 2, 10)
        sizes = [f(nq, st, 2, k) for k in range(1, 65)]
        assert all(b >= a for a, b in zip(sizes, sizes[1:]))
    # the headline block: 1,000 x 1M int16 = 2 GB of scores needs well under 1 % of that
    assert f(1000, 1_000_064, 2, 64) < 20 * 1024 * 1024


def test_reference_helper_agrees_with_a_brute_force_loop():
    rng = np.random.default_rng(5)
    for trial in range(40):
        nq, ns = int(rng.integers(1, 4)), int(rng.integers(1, 12))
        valid = int(rng.integers(1, ns + 1))
        tile = rng.integers(-2, 2, (nq, ns)).astype(np.int16)       # four distinct values: ties everywhere
        for k in (1, 3, valid, valid + 2):
            for smallest in (False, True):
                base = int(rng.integers(0, 1000))
                got = H.top_hits(tile, valid, k, smallest, base)
                want = H.brute_top_hits(tile, valid, k, smallest, base)
                assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (trial, k, smallest)
    # ties go to the smaller subject id; padding columns never appear; unused slots are (-1, worst)
    tile = np.array([[5, 7, 7, 5, 9, 9]], dtype=np.int16)
    s, j = H.top_hits(tile, 4, 5, False, subject_base=100)
    assert j.tolist() == [[101, 102, 100, 103, -1]] and s.tolist() == [[7, 7, 5, 5, H.INT32_MIN]]
    s, j = H.top_hits(tile, 4, 2, True)
    assert j.tolist() == [[0, 3]] and s.tolist() == [[5, 5]]


def test_reference_threshold_lists_and_accumulate():
    tile = np.array([[3, 1, 4, 1, 5, 9, 2, 6]], dtype=np.int8)
    c, s, j = H.threshold_hits(tile, 7, 2, True, 4, subject_base=10)
    assert c.tolist() == [3] and s[0, :3].tolist() == [1, 1, 2] and j[0, :3].tolist() == [11, 13, 16]
    c, s, j = H.threshold_hits(tile, 8, 4, False, 2)             # overflow: true count, the lowest-indexed hits
    assert c.tolist() == [4] and j.tolist() == [[2, 4]] and s.tolist() == [[4, 5]]
    # three buckets accumulated = the whole bucket at once, for both selections
    rng = np.random.default_rng(9)
    whole = rng.integers(-3, 3, (3, 50)).astype(np.int16)
    cuts = [(0, 17), (17, 18), (18, 50)]
    top = thr = None
    for lo, hi in cuts:
        top = H.top_hits(whole[:, lo:hi], hi - lo, 6, False, subject_base=lo, into=top)
        thr = H.threshold_hits(whole[:, lo:hi], hi - lo, 1, False, 50, subject_base=lo, into=thr)
    want = H.top_hits(whole, 50, 6, False)
    assert np.array_equal(top[0], want[0]) and np.array_equal(top[1], want[1])
    assert H.threshold_lists_equal(thr, H.threshold_hits(whole, 50, 1, False, 50), 50)


def test_merge_hits_is_the_helpers_merge():
    rng = np.random.default_rng(3)
    for smallest in (False, True):
        sc = rng.integers(-4, 1, (5, 24)).astype(np.int32)
        sj = np.stack([rng.permutation(1000)[:24] for _ in range(5)]).astype(np.int64)
        sj[:, 20:] = -1                                            # unused slots of a short shard
        sc[:, 20:] = H.worst(smallest)
        got = merge_hits(torch, torch.from_numpy(sc), torch.from_numpy(sj), 8, smallest)
        want = H.merge(sc.astype(np.int64), sj, 8, smallest)
        assert np.array_equal(got[0].numpy(), want[0]) and np.array_equal(got[1].numpy(), want[1])
    got = merge_hits(torch, torch.from_numpy(sc[:, 20:]), torch.from_numpy(sj[:, 20:]), 6, True)    # nothing but unused slots
    assert (got[1].numpy() == -1).all() and (got[0].numpy() == H.INT32_MAX).all()


# ---- run_hits: the exchange and the merge under gloo, the oracle + the helper as the compute hook -----------------------
NQ, NS, K_BEST = 6, 333, 10


def _reads(O):
    q = O.gen_reads(31, NQ, 150)
    s = O.gen_reads(32, NS, 150)      # random 150 bp reads: distances cluster in a few values, ties cross every shard border
    return q, s


def _oracle_hits_fn(O, seen=None):
    def hits_fn(queries, subjects, k_best, smallest, subject_base):
        if seen is not None:
            seen.append((queries.shape, subjects.shape, subject_base))
        if subjects.shape[0] == 0:
            return H.merge(np.zeros((queries.shape[0], 0), np.int64), np.zeros((queries.shape[0], 0), np.int64), k_best, smallest)
        return H.top_hits(O.myers64(queries, subjects), subjects.shape[0], k_best, smallest, subject_base)
    return hits_fn


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    import oracle as O

    q, s = _reads(O)
    seen = []
    sa = ShardedAligner(dist=dist)
    result, shards = sa.run_hits(q if rank == 0 else None, s, K_BEST, hits_fn=_oracle_hits_fn(O, seen))
    assert seen == [((NQ, 150), (shards[rank].count, 150), shards[rank].start)]     # all queries, own slice, its base
    if rank == 0:
        np.savez(out_path, scores=result[0].numpy(), subjects=result[1].numpy())
    else:
        assert result is None
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_run_hits_under_gloo_equals_the_whole_bucket(tmp_path, oracle, world):
    out = tmp_path / "hits.npz"
    mp.spawn(_worker, args=(world, _free_port(), str(out)), nprocs=world, join=True)
    got = np.load(out)
    q, s = _reads(oracle)
    want = H.top_hits(oracle.myers64(q, s), NS, K_BEST, False)
    assert got["scores"].dtype == np.int32 and got["subjects"].dtype == np.int64
    assert np.array_equal(got["scores"], want[0]) and np.array_equal(got["subjects"], want[1])
    # the case is a real one: some query's K-th and (K+1)-th candidates tie, and its list spans more than one shard
    full = oracle.myers64(q, s)
    ranked = -np.sort(-full.astype(np.int64), axis=1)
    assert (ranked[:, K_BEST - 1] == ranked[:, K_BEST]).any()
    border = plan_shards(NS, world)[1].start
    assert ((want[1] < border).any(axis=1) & (want[1] >= border).any(axis=1)).any()


def test_run_hits_single_rank_needs_no_process_group(oracle):
    q, s = _reads(oracle)
    for smallest in (False, True):
        sa = ShardedAligner(dist=None)
        (sc, sj), shards = sa.run_hits(q, s, K_BEST, smallest=smallest, hits_fn=_oracle_hits_fn(oracle))
        want = H.top_hits(oracle.myers64(q, s), NS, K_BEST, smallest)
        assert len(shards) == 1 and np.array_equal(sc.numpy(), want[0]) and np.array_equal(sj.numpy(), want[1])


def test_run_hits_direction_follows_the_aligner():
    assert B.default_smallest(B.ALGO_BANDED) and B.default_smallest(B.ALGO_MYERS, (0, 1, 1))
    assert not B.default_smallest(B.ALGO_MYERS) and not B.default_smallest(B.ALGO_BITPAL, (2, -3, -5))
    assert not B.default_smallest(B.ALGO_MYERS, (0, -1, -1))

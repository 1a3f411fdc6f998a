"""Subject buckets of mixed read lengths on the GPU: scores, hit lists and edit scripts of DeviceAligner.set_subjects_ragged and
the binned drivers, bit for bit against the pinned oracle called once per length class on subject[:len], and against this
library's own equal-length path on each length class alone.

Subjects are a mutated query prefix cut to their length (small, varied distances) with every fourth one a random read."""
import ctypes
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import hits_reference as H  # noqa: E402
import oracle as O  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# one wave holds lanes that end in different words, at both edges of every word
LENS_150 = [1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 149, 150]


def make_bucket(seed, nq, qlen, lens, width=None):
    """(queries[nq, qlen], subjects: list of 1-D arrays of the given lengths, tails[ns, width]: for every subject the bytes its
    source goes on with behind the subject's end — the query's own continuation, the worst thing a pad can hold)."""
    lens = [int(n) for n in lens]
    width = max(max(lens), qlen) if width is None else width
    q = O.gen_reads(seed, nq, qlen)
    ns = len(lens)
    src = q[np.arange(ns) % nq]
    full = np.concatenate([O.mutate(src, np.arange(ns) % 7, seed + 1), O.gen_reads(seed + 2, ns, width)], axis=1)
    clean = np.concatenate([src, O.gen_reads(seed + 2, ns, width)], axis=1)
    rnd = O.gen_reads(seed + 3, ns, width + qlen)
    full[3::4] = rnd[3::4]
    subjects = [full[i, :n].copy() for i, n in enumerate(lens)]
    tails = np.stack([np.concatenate([clean[i, n:], rnd[i]])[:width] for i, n in enumerate(lens)])
    return q, subjects, tails


def by_class(fn, q, subjects):
    """fn(q, rows) -> [nq, n] once per length class on the unpadded subjects; columns in the subjects' order."""
    lens = np.array([s.size for s in subjects])
    out = np.empty((q.shape[0], len(subjects)), dtype=np.int64)
    for n in np.unique(lens):
        cols = np.flatnonzero(lens == n)
        out[:, cols] = fn(q, np.stack([subjects[c] for c in cols]))
    return out


def equal_length_path(q, subjects, algo, scores=None):
    """This library's equal-length launches, one per length class."""
    a = B.DeviceAligner(algo, DEV, 0, scores)
    a.set_queries(q)

    def run(_, rows):
        a.set_subjects(rows)
        assert a.d_lens is None
        return a.score()[:, : a.ns_real].cpu().numpy()
    out = by_class(run, q, subjects)
    a.check_faults()
    return out


def ragged_aligner(q, subjects, algo=B.ALGO_MYERS, scores=None):
    a = B.DeviceAligner(algo, DEV, 0, scores)
    a.set_queries(q)
    a.set_subjects_ragged(subjects)
    return a


def ragged_scores(q, subjects, algo=B.ALGO_MYERS, scores=None):
    a = ragged_aligner(q, subjects, algo, scores)
    assert a.d_lens is not None and a.d_lens.numel() == a.ns and a.ns % 64 == 0
    assert a.slen == max(s.size for s in subjects)
    assert a.d_lens[a.ns_real:].cpu().tolist() == [a.slen] * a.extra      # pad columns get the longest length
    out = a.score()
    a.check_faults()
    return out[:, : a.ns_real].cpu().numpy()


def set_padded_rows(a, subjects, pad_rows_behind):
    """The bucket with chosen bytes behind every subject's end (set_subjects_ragged writes 'N' there)."""
    import torch
    rows, lens = B.pad_ragged(subjects)
    for i, n in enumerate(lens):
        rows[i, n:] = pad_rows_behind[i][: rows.shape[1] - n]
    padded, extra = B.pad_rows(rows)
    lens = np.concatenate([lens, np.full(extra, rows.shape[1], dtype=np.int32)])
    a.ns_real, a.extra = rows.shape[0], extra
    a.set_subject_rows_device(torch.from_numpy(B.rows_to_buffer(padded)).to(a.device), padded.shape[0], padded.shape[1], None,
                              d_lens=torch.from_numpy(lens).to(a.device))


@functools.lru_cache(maxsize=None)
def case1():
    """Myers, 5 words: qlen 150, 130 subjects = three groups and 62 padding columns.  Shared and never modified."""
    q, subjects, tails = make_bucket(0xA661, 6, 150, [LENS_150[i % 16] for i in range(130)])
    want = by_class(O.dp_edit, q, subjects)
    assert np.array_equal(want, by_class(O.myers64, q, subjects))      # the two oracles agree on every class
    assert len(np.unique(-want)) > 40 and (-want[:, ::4] < 40).any()   # varied, not saturated
    return q, subjects, tails, want


def _stats():
    out = (ctypes.c_ulonglong * 2)()
    assert B.lib().bgsa_hip_myers_band_stats(out, 0) == 0
    return int(out[0]), int(out[1])


# ---- 1. Myers, 5 words, one group per wave ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores,sign", [(None, 1), ((0, 1, 1), -1)], ids=["-distance", "+distance"])
def test_myers_five_words(scores, sign):
    q, subjects, _, want = case1()
    got = ragged_scores(q, subjects, B.ALGO_MYERS, scores)
    assert got.dtype == np.int16 and np.array_equal(got, sign * want)
    assert np.array_equal(got, equal_length_path(q, subjects, B.ALGO_MYERS, scores))


# ---- 2. Myers <= 2 words: two rows per token, two groups per wave or one --------------------------------------------------------
@pytest.mark.parametrize("ns,top", [(200, 64), (64, 64), (130, 32)], ids=["2 words, G=2", "2 words, one group", "1 word, G=2"])
def test_myers_pair_rows(ns, top):
    q, subjects, _ = make_bucket(0xA662 + ns, 5, 60, [i % top + 1 for i in range(ns)])
    want = by_class(O.dp_edit, q, subjects)
    got = ragged_scores(q, subjects)
    assert np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects, B.ALGO_MYERS))


# ---- 3. Myers wide: the chains-in-turns kernels (30, 32 words) and one middle width (10 words, static grid) ---------------------
WIDE = {
    "32 words": (1000, [[1, 33, 897, 960, 961, 992, 993, 1023, 1024][i % 9] for i in range(64)]),
    "30 words": (1000, [[1, 33, 897, 929, 959, 960][i % 6] for i in range(64)]),
    "10 words": (300, list(range(257, 301)) + [1, 31, 32, 33, 150, 256] * 2 + list(range(290, 301)) * 4),
}


@pytest.mark.parametrize("name", list(WIDE))
def test_myers_wide(name):
    qlen, lens = WIDE[name]
    q, subjects, _ = make_bucket(0xA663 + len(lens) + max(lens), 3, qlen, lens)
    assert B.word_num(B.ALGO_MYERS, qlen, max(lens)) == int(name.split()[0])
    want = by_class(O.dp_edit, q, subjects)
    got = ragged_scores(q, subjects)
    assert np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects, B.ALGO_MYERS))


# ---- 4. BitPAl ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scores", [(2, -3, -5), (1, -1, -2)], ids=str)
def test_bitpal(scores):
    q, subjects, _, _ = case1()
    want = by_class(lambda qq, rows: O.dp_nw(qq, rows, *scores), q, subjects)
    got = ragged_scores(q, subjects, B.ALGO_BITPAL, scores)
    assert np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects, B.ALGO_BITPAL, scores))


def test_bitpal_beyond_the_counter_widths():
    # 9 words: the static-grid instantiation of the length-aware BitPAl kernel
    q, subjects, _ = make_bucket(0xA664, 3, 280, list(range(225, 289)) + [1, 32, 33, 256, 257, 288])
    want = by_class(O.dp_nw, q, subjects)
    assert np.array_equal(ragged_scores(q, subjects, B.ALGO_BITPAL, (2, -3, -5)), want)


# ---- 5. what lies behind a subject's end never enters ----------------------------------------------------------------------------
@pytest.mark.parametrize("algo,scores", [(B.ALGO_MYERS, None), (B.ALGO_BITPAL, (2, -3, -5))], ids=["myers", "bitpal"])
def test_pad_independence(algo, scores):
    q, subjects, tails, want = case1()
    a = B.DeviceAligner(algo, DEV, 0, scores)
    a.set_queries(q)
    tiles = []
    for pad in (np.full_like(tails, ord("N")), np.full_like(tails, ord("A")), tails):   # tails: the query's own continuation
        set_padded_rows(a, subjects, pad)
        tiles.append(a.score()[:, : a.ns_real].cpu().numpy())
    a.check_faults()
    assert np.array_equal(tiles[0], tiles[1]) and np.array_equal(tiles[0], tiles[2])
    if algo == B.ALGO_MYERS:
        assert np.array_equal(tiles[0], want)
        # the pads do differ where it would show: scored at the full width the three buckets disagree
        a.d_lens = None
        full = []
        for pad in (np.full_like(tails, ord("N")), tails):
            rows, _ = B.pad_ragged(subjects)
            for i, s in enumerate(subjects):
                rows[i, s.size:] = pad[i][: rows.shape[1] - s.size]
            a.set_subjects(rows)
            full.append(a.score()[:, : a.ns_real].cpu().numpy())
        assert not np.array_equal(full[0], full[1])


# ---- 6. the certified band ------------------------------------------------------------------------------------------------------
def test_lens_launch_leaves_the_band_statistics_alone():
    q, subjects, _, want = case1()
    a = ragged_aligner(q, subjects)
    a.torch.cuda.synchronize()
    before = _stats()
    got = a.score()
    a.check_faults()
    assert _stats() == before
    assert np.array_equal(got[:, : a.ns_real].cpu().numpy(), want)


def test_null_lens_is_the_plain_call_band_included():
    import torch
    q = O.gen_reads(0xA666, 6, 150)
    s = O.mutate(q[np.arange(128) % 6], np.arange(128) % 9, 0xA667)
    a = B.DeviceAligner(B.ALGO_MYERS, DEV)
    a.set_queries(q)
    a.set_subjects_ragged(list(s))          # equal lengths: this is set_subjects
    assert a.d_lens is None
    assert B.lib().bgsa_hip_myers_band_half(150, 150) > 0
    L, p = B.lib(), a.params()
    outs, deltas = [], []
    need = int(L.bgsa_hip_workspace_bytes_ex(ctypes.byref(p), 150, 150, 6))
    work = torch.empty(need, dtype=torch.uint8, device=a.device)
    for lens_call in (False, True):
        out = torch.full((6, 128), 0x7777, dtype=torch.int16, device=a.device)
        torch.cuda.synchronize()
        before = _stats()
        if lens_call:
            rc = L.bgsa_hip_cal_align_score_lens_ex(ctypes.byref(p), a.d_content.data_ptr(), a.d_peq.data_ptr(), out.data_ptr(), None,
                                                    150, 150, 128, 0, 6, a.wn, work.data_ptr(), need, a._stream())
        else:
            rc = L.bgsa_hip_cal_align_score_ex(ctypes.byref(p), a.d_content.data_ptr(), a.d_peq.data_ptr(), out.data_ptr(),
                                               150, 150, 128, 0, 6, a.wn, work.data_ptr(), need, a._stream())
        assert rc == 0, L.bgsa_hip_last_error()
        a.check_faults()
        after = _stats()
        outs.append(out.cpu().numpy().tobytes())
        deltas.append((after[0] - before[0], after[1] - before[1]))
    assert outs[0] == outs[1]
    assert deltas[0] == deltas[1] and deltas[0][1] == 6 * 2       # every (query, wave) banded, by either call
    assert np.array_equal(np.frombuffer(outs[1], dtype=np.int16).reshape(6, 128), O.myers64(q, s))


# ---- 7. query window ------------------------------------------------------------------------------------------------------------
def test_query_window():
    q, subjects, _, want = case1()
    a = ragged_aligner(q, subjects)
    got = a.score(2, q.shape[0] - 1)
    a.check_faults()
    assert tuple(got.shape) == (q.shape[0] - 3, a.ns)
    assert np.array_equal(got[:, : a.ns_real].cpu().numpy(), want[2: q.shape[0] - 1])


# ---- 8. hit lists ---------------------------------------------------------------------------------------------------------------
def test_hits():
    q, subjects, _, want = case1()
    a = ragged_aligner(q, subjects)
    scores, ids = a.top_hits(5, block_rows=4)                 # two blocks of queries
    ws, wi = H.top_hits(want, len(subjects), 5, False)
    assert np.array_equal(scores.cpu().numpy(), ws) and np.array_equal(ids.cpu().numpy(), wi)
    assert int(ids.max()) < len(subjects)                     # padding columns never appear
    cutoff, cap = -25, len(subjects)
    got = tuple(x.cpu().numpy() for x in a.threshold_hits(cutoff, cap, block_rows=4))
    ref = H.threshold_hits(want, len(subjects), cutoff, False, cap)
    assert ref[0].sum() > 0 and H.threshold_lists_equal(got, ref, cap)
    for r in range(q.shape[0]):
        assert (got[2][r, : got[0][r]] < len(subjects)).all()
    a.check_faults()


# ---- 9. edit scripts ------------------------------------------------------------------------------------------------------------
def _consumed(runs):
    return (sum(n for n, op in runs if op != A.OP_D), sum(n for n, op in runs if op != A.OP_I))


def test_align_hits():
    q, subjects, _, want = case1()
    a = ragged_aligner(q, subjects)
    scores, ids = a.top_hits(5)
    distance, n_ops, cigar = a.align_hits(ids)
    a.check_faults()
    assert tuple(cigar.shape) == (q.shape[0], 5, 150 + 150)   # cigar_cap=None stays qlen + max_len
    assert np.array_equal(distance.cpu().numpy(), -scores.cpu().numpy())
    ids, distance, n_ops = ids.cpu().numpy(), distance.cpu().numpy(), n_ops.cpu().numpy()
    words = cigar.cpu().numpy().view(np.uint32)
    lens = np.array([s.size for s in subjects])
    pairs = [(r, k) for r in range(q.shape[0]) for k in range(5)]
    for n in np.unique(lens[ids.reshape(-1)]):      # canonical(...) once per length class
        cls = [(r, k) for r, k in pairs if lens[ids[r, k]] == n]
        ref = A.canonical(q[[r for r, _ in cls]], np.stack([subjects[ids[r, k]] for r, k in cls]))
        for (r, k), (d, runs) in zip(cls, ref):
            got = A.unpack(words[r, k, : n_ops[r, k]])
            A.validate(q[r], subjects[ids[r, k]], int(distance[r, k]), got)
            assert got == runs and d == distance[r, k] == -want[r, ids[r, k]]
            assert _consumed(got) == (150, n)


def test_align_pairs_chunked_at_the_minimum_workspace():
    q, subjects, _, want = case1()
    a = ragged_aligner(q, subjects)
    nq, ns = q.shape[0], len(subjects)
    pq, ps = np.repeat(np.arange(nq), ns), np.tile(np.arange(ns), nq)       # 780 pairs: 13 waves, one per chunk
    one_pass = [x.cpu().numpy() for x in a.align_pairs(pq, ps)]
    minimum = int(B.lib().bgsa_hip_align_pairs_min_workspace_bytes(150, 150))
    chunked = [x.cpu().numpy() for x in a.align_pairs(pq, ps, workspace_bytes=minimum)]
    a.check_faults()
    assert np.array_equal(one_pass[0].reshape(nq, ns), -want)
    for x, y in zip(one_pass, chunked):
        assert np.array_equal(x, y)
    lens = np.array([s.size for s in subjects])
    words = chunked[2].view(np.uint32)
    for p in range(0, nq * ns, 7):
        runs = A.unpack(words[p, : chunked[1][p]])
        assert _consumed(runs) == (150, lens[ps[p]])


def test_trace_hits_bitpal_global():
    q, subjects, _, _ = case1()
    scores = (2, -3, -5)
    a = ragged_aligner(q, subjects, B.ALGO_BITPAL, scores)
    tile = a.score()[:, : a.ns_real].cpu().numpy()
    hit_scores, ids = a.top_hits(4)
    score, span, n_ops, cigar = (x.cpu().numpy() for x in a.trace_hits(ids))
    a.check_faults()
    ids = ids.cpu().numpy()
    lens = np.array([s.size for s in subjects])
    words = cigar.view(np.uint32)
    for r in range(q.shape[0]):
        for k in range(4):
            n = int(lens[ids[r, k]])
            assert score[r, k] == tile[r, ids[r, k]] == hit_scores[r, k]
            assert span[r, k].tolist() == [0, 150, 0, n]
            runs = A.unpack(words[r, k, : n_ops[r, k]])
            assert _consumed(runs) == (150, n)
            value = sum(length * {A.OP_EQ: scores[0], A.OP_X: scores[1]}.get(op, scores[2]) for length, op in runs)
            assert value == score[r, k]
    # a pair with a short subject and the Myers cross-check kernel: the same script as align_pairs
    m = ragged_aligner(q, subjects)
    some = np.array([[0, 2, 16, 129]] * q.shape[0])
    d, n1, c1 = (x.cpu().numpy() for x in m.align_hits(some))
    s2, sp2, n2, c2 = (x.cpu().numpy() for x in m.trace_hits(some))
    m.check_faults()
    assert np.array_equal(-d, s2) and np.array_equal(n1, n2)
    for r in range(q.shape[0]):
        for k in range(4):
            assert np.array_equal(c1[r, k, : n1[r, k]], c2[r, k, : n2[r, k]]) and sp2[r, k, 3] == lens[some[r, k]]


# ---- 10. refusals on the device path ----------------------------------------------------------------------------------------------
def _refused(a, text):
    import torch
    out = torch.full((a.nq, a.ns), 0x7777, dtype=a.out_dtype, device=a.device) if a.out_dtype == torch.int16 else \
        torch.full((a.nq, a.ns), 0x77, dtype=a.out_dtype, device=a.device)
    with pytest.raises(B.BgsaHipError, match="rc=-2") as e:
        a.score(out=out)
    assert "per-subject lengths" in str(e.value) and text in str(e.value)
    a.check_faults()
    assert bool((out == (0x7777 if a.out_dtype == torch.int16 else 0x77)).all())


def test_refusals_leave_the_outputs_untouched():
    q, subjects, _, _ = case1()
    for algo, scores in ((B.ALGO_MYERS, None), (B.ALGO_BITPAL, (2, -3, -5))):
        a = B.DeviceAligner(algo, DEV, 0, scores, semi_global=True)
        a.set_queries(q)
        a.set_subjects_ragged(subjects)
        _refused(a, "semi-global")
    a = B.DeviceAligner(B.ALGO_BANDED, DEV, 8)
    a.set_queries(q)
    a.set_subjects_ragged(subjects[14:16] * 32)      # 149 and 150 bp
    _refused(a, "banded filter")
    a = B.DeviceAligner(B.ALGO_MYERS, DEV)
    a.set_queries(q)
    a.set_subjects_ragged([O.gen_reads(1, 1, 1056)[0], O.gen_reads(2, 1, 100)[0]])
    assert a.wn == 33
    _refused(a, "word_num > 32")
    a = B.DeviceAligner(B.ALGO_MYERS, DEV, semi_global=True)
    a.set_queries(q)
    a.set_subjects_ragged(subjects)
    with pytest.raises(B.BgsaHipError, match="rc=-2"):
        a.trace_pairs([0], [0])
    a.check_faults()


# ---- 11. the binned drivers -------------------------------------------------------------------------------------------------------
def test_binned_drivers():
    lens = [20 + (i * 37) % 281 for i in range(148)] + [300, 20]
    q, subjects, _ = make_bucket(0xA66B, 3, 150, lens)
    assert min(lens) == 20 and max(lens) == 300
    want = by_class(O.dp_edit, q, subjects)
    got = B.align_all_pairs_ragged(q, subjects, device=DEV)
    assert got.shape == (3, 150) and np.array_equal(got, want)
    got = B.align_all_pairs_ragged(q, subjects, algo=B.ALGO_BITPAL, scores=(1, -1, -2), device=DEV)
    assert np.array_equal(got, by_class(lambda qq, rows: O.dp_nw(qq, rows, 1, -1, -2), q, subjects))
    hit_scores, ids = B.align_top_hits_ragged(q, subjects, 4, device=DEV)
    assert ids.shape == (3, 4) and ids.min() >= 0 and ids.max() < 150
    for r in range(3):
        assert len(set(ids[r].tolist())) == 4
        assert np.array_equal(want[r, ids[r]], hit_scores[r])            # the ids are the caller's indices
    assert np.array_equal(hit_scores, H.top_hits(want, 150, 4, False)[0])

"""Seeded read mapping on the MI355X: the k-mer index, the candidate counts and lists, the verify kernel, the selection — each
against tests/seed_map_reference.py or against the scored tile —, and ReferenceMapper.map_reads_seeded bit for bit against the
blanked map_reads, the blanked host pipeline and the whole-reference optimum."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import reference_map_reference as M  # noqa: E402
import seed_map_reference as R  # noqa: E402
from align_reference import classes  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = -77            # what an output holds where nobody may write
FIELDS = ("scores", "windows", "strand", "ref_begin", "ref_end", "keep")


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


# ---- the 128-read case of test_reference_map_gpu.py, restated ---------------------------------------------------------------
REF_LEN, W, S, N, BOUND, Q = 3000, 96, 48, 32, 4, 6
REPEAT_AT, UNIT, COPIES = 1500, 40, 3


def make_case():
    """(reference, reads[128, 32], kinds): planted on both strands with 0..3 edits, in window overlaps, at both edges, in the
    tandem repeat, and unrelated; three N in the reference."""
    rng = np.random.default_rng(3000)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    ref[REPEAT_AT: REPEAT_AT + UNIT * COPIES] = np.tile(ACGT[rng.integers(4, size=UNIT)], COPIES)
    ref[[333, 2222, 2900]] = ord("N")
    reads, kinds = [], []

    def add(kind, strand, begin, edits=0):
        room = min(N + 3, REF_LEN - begin)
        src = _edit(rng, list(ref[begin: begin + room]), edits if room == N + 3 else 0, ACGT)
        read = np.array(src[:N], np.uint8)
        assert read.size == N
        reads.append(M.reverse_complement(read) if strand else read)
        kinds.append(kind)

    clear = [x for x in rng.permutation(REF_LEN - N - 3) if not REPEAT_AT - N - 3 < x < REPEAT_AT + UNIT * COPIES]
    for i in range(40):
        add("planted", 0, int(clear[i]), i % 4)
    for i in range(40):
        add("planted", 1, int(clear[40 + i]), i % 4)
    for i, m in enumerate((3, 7, 11, 19, 23, 40, 47, 55)):
        add("overlap", 0, m * S - 16, i % 3)
        add("overlap", 1, (m + 1) * S - 16, i % 3)
    for strand in (0, 1):
        add("edge", strand, 0)
        add("edge", strand, REF_LEN - N)
    for i in range(12):
        add("repeat", 0, REPEAT_AT + 3 * i)
        add("repeat", 1, REPEAT_AT + 3 * i + 1)
    for _ in range(4):
        reads.append(ACGT[rng.integers(4, size=N)])
        kinds.append("unrelated")
    assert len(reads) == 128
    return ref, np.stack(reads), kinds


def whole_reference_optimum(ref, reads):
    """min over i of D[i][n] with D[0][j] = j, D[i][0] = 0, unit costs over the classes: one row step per reference base."""
    rc, sc = classes(ref), classes(reads)
    n = sc.shape[1]
    ramp = np.arange(n + 1, dtype=np.int32)
    d = np.tile(ramp, (sc.shape[0], 1))
    best = d[:, n].copy()
    for c in rc:
        t = np.empty_like(d)
        t[:, 0] = 0
        np.minimum(d[:, 1:] + 1, d[:, :-1] + (sc != c), out=t[:, 1:])
        d = np.minimum.accumulate(t - ramp, axis=1) + ramp
        np.minimum(best, d[:, n], out=best)
    return best


def assert_same_hits(got, want, what=""):
    for name in FIELDS:
        g, w = getattr(got, name), (want[name] if isinstance(want, dict) else getattr(want, name))
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"{name} differs {what}: {np.argwhere(g != w)[:5].tolist()}"
    assert got.cigars == (want["cigars"] if isinstance(want, dict) else want.cigars), f"the cigars differ {what}"


@pytest.fixture(scope="module")
def case(torch_gpu):
    """The case, what the helper says about it (host only, asserted before the GPU is touched), and the exhaustive results."""
    ref, reads, kinds = make_case()
    offsets, positions = R.index(classes(ref), Q)
    lookup = R.lookup_of(offsets, positions)
    flagged = np.array([R.has_n_piece(r, BOUND, Q) for r in reads])
    cands = [R.candidates(lookup, REF_LEN, W, S, r, BOUND, Q) for r in reads]
    assert flagged.sum() <= 8, "too many reads with an N in a piece: the case would test the exhaustive path"
    n_ids = 2 * M.window_count(REF_LEN, W, S)
    assert max(len(c) for c in cands) <= max(n_ids // 8, 256)             # the default cap sends nobody to the exhaustive path
    assert B.max_stride(W, N, BOUND) == 61 >= S and B.seed_plan(N, BOUND) == (BOUND, Q, Q)
    mapper = B.ReferenceMapper(ref, W, S)
    full = {k: mapper.map_reads(reads, k_best=k, max_distance=BOUND) for k in (1, 3)}
    host = M.map_reads_host(ref, W, S, reads, k_best=3, max_distance=BOUND)
    return dict(ref=ref, reads=reads, kinds=kinds, offsets=offsets, positions=positions, flagged=flagged, cands=cands, mapper=mapper,
                full=full, host=host)


def upload_reads(torch, reads):
    return torch.from_numpy(B.rows_to_buffer(B.pad_rows(reads)[0])).cuda()


# ---- 1. the index -----------------------------------------------------------------------------------------------------------
def check_index(mapper, ref, q):
    offsets, positions = mapper.seed_index(q)
    mapper.aligner.torch.cuda.synchronize()
    want_offsets, want_positions = R.index(classes(ref), q)
    got_offsets = offsets.cpu().numpy()
    assert got_offsets.dtype == np.int32 and got_offsets.size == 4 ** q + 1
    assert np.array_equal(got_offsets, want_offsets)
    total = int(want_offsets[-1])
    assert np.array_equal(R.sorted_buckets(got_offsets, positions.cpu().numpy()[:total]), want_positions)
    return total, want_offsets


@pytest.mark.parametrize("q", [1, 5, 6, 12])
def test_index_equals_the_helper(case, q):
    total, offsets = check_index(B.ReferenceMapper(case["ref"], W, S), case["ref"], q)
    assert total == REF_LEN - q + 1 - sum(min(q, at + 1, REF_LEN - at) for at in (333, 2222, 2900))     # the k-mers over an N
    assert np.diff(offsets).max() >= COPIES        # the tandem repeat: a k-mer of the unit occurs once per copy


def test_index_edge_cases(torch_gpu):
    rng = np.random.default_rng(12)
    q = 5
    short = ACGT[rng.integers(4, size=q - 1)]
    assert check_index(B.ReferenceMapper(short, q - 1, 1), short, q)[0] == 0                 # L = q - 1: an empty index
    exact = ACGT[rng.integers(4, size=q)]
    assert check_index(B.ReferenceMapper(exact, q, 1), exact, q)[0] == 1                     # L = q: one k-mer
    all_n = np.full(300, ord("N"), np.uint8)
    assert check_index(B.ReferenceMapper(all_n, 64, 40), all_n, q)[0] == 0
    odd = ACGT[rng.integers(4, size=700)].copy()
    odd[[5, 99, 100, 640]] = [ord("x"), ord("-"), ord("n"), 200]                           # outside the alphabet: class 0, indexed as 'A'
    assert check_index(B.ReferenceMapper(odd, 64, 40), odd, q)[0] == 700 - q + 1
    assert check_index(B.ReferenceMapper(odd, 64, 40), odd, 1)[0] == 700


# ---- 2. counts, flags and candidates ----------------------------------------------------------------------------------------
def run_count_emit(torch, mapper, reads, bound, q, cap, both=True):
    L = B.lib()
    offsets, positions = mapper.seed_index(q)
    ns, n = reads.shape
    d_rows = upload_reads(torch, reads)
    counts = torch.full((ns + 3,), SENT, dtype=torch.int32, device="cuda")
    shape = (mapper.ref_len, mapper.window_len, mapper.stride, offsets.data_ptr(), positions.data_ptr(), q)
    B.check(L.bgsa_hip_seed_count_candidates_dev(*shape, d_rows.data_ptr(), n, ns, bound, int(both), cap, counts.data_ptr(), None), "count")
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert (got[ns:] == SENT).all()
    got = got[:ns]
    sizes = np.maximum(got, 0).astype(np.int64)
    prefix = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    out_read = torch.full((total + 5,), SENT, dtype=torch.int32, device="cuda")
    out_window = torch.full((total + 5,), SENT, dtype=torch.int32, device="cuda")
    B.check(L.bgsa_hip_seed_emit_candidates_dev(*shape, d_rows.data_ptr(), n, ns, bound, int(both), counts.data_ptr(),
                                                torch.from_numpy(prefix).cuda().data_ptr(), 1000, out_read.data_ptr(),
                                                out_window.data_ptr(), None), "emit")
    torch.cuda.synchronize()
    out_read, out_window = out_read.cpu().numpy(), out_window.cpu().numpy()
    assert (out_read[total:] == SENT).all() and (out_window[total:] == SENT).all()
    lists = []
    for c in range(ns):
        mine = slice(int(prefix[c]), int(prefix[c] + sizes[c]))
        assert (out_read[mine] == 1000 + c).all()                                        # read_base + r
        lists.append(sorted(out_window[mine].tolist()))
    return got, lists


def test_counts_and_candidates_equal_the_helper(torch_gpu, case):
    reads, cands, flagged = case["reads"], case["cands"], case["flagged"]
    got, lists = run_count_emit(torch_gpu, case["mapper"], reads, BOUND, Q, 10 ** 6)
    want = np.array([R.count_or_flag(c, f, 10 ** 6) for c, f in zip(cands, flagged)])
    assert np.array_equal(got, want)
    for c in range(128):
        assert lists[c] == ([] if flagged[c] else sorted(cands[c])), c
    assert (got > 0).sum() >= 120 and sum(len(set(x)) < len(x) for x in lists) >= 60          # repetitions do occur


def test_flags_with_a_cap_of_8(torch_gpu, case):
    got, lists = run_count_emit(torch_gpu, case["mapper"], case["reads"], BOUND, Q, 8)
    want = np.array([R.count_or_flag(c, f, 8) for c, f in zip(case["cands"], case["flagged"])])
    assert np.array_equal(got, want)
    assert (want == -2).sum() >= 24 and (want == -1).sum() == case["flagged"].sum() and (want >= 0).sum() >= 1
    assert all(len(lists[c]) == max(want[c], 0) for c in range(128))
    exact = np.array([len(c) for c in case["cands"]])
    got, _ = run_count_emit(torch_gpu, case["mapper"], case["reads"][:64], BOUND, Q, int(exact[:64].max()))   # count == cap is not above it
    assert not (got == -2).any()


def test_counts_forward_strand_only_and_other_seeds(torch_gpu, case):
    forward = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    for q in (3, 6):
        offsets, positions = R.index(classes(case["ref"]), q)
        lookup = R.lookup_of(offsets, positions)
        reads = case["reads"][::4]
        got, lists = run_count_emit(torch_gpu, forward, reads, BOUND, q, 10 ** 6, both=False)
        for c, read in enumerate(reads):
            if R.has_n_piece(read, BOUND, q, both_strands=False):
                assert got[c] == -1
            else:
                assert lists[c] == sorted(R.candidates(lookup, REF_LEN, W, S, read, BOUND, q, both_strands=False)), (q, c)


# ---- 3. the verify kernel against the scored tile -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [32, 33, 150, 512, 513, 1024])
def test_verify_equals_the_scored_tile(torch_gpu, n):
    torch = torch_gpu
    rng = np.random.default_rng(n)
    ref_len, w_len, stride, ns, spare = 3000, n + 48, 37, 70, 8          # spare bases, so that a read with 8 deletions is still all reference
    ref = ACGT[rng.integers(4, size=ref_len)].copy()
    ref[rng.integers(ref_len, size=12)] = ord("N")
    reads, begins = [], []
    for c in range(ns):
        begin = int(rng.integers(0, ref_len - n - spare))
        if c % 7 == 6:
            begin = ref_len - n - spare                                                   # in the anchored last window
        read = np.array(_edit(rng, list(ref[begin: begin + n + spare]), int(rng.integers(0, spare + 1)), ACGT)[:n], np.uint8)
        assert read.size == n
        reads.append(ACGT[rng.integers(4, size=n)] if c % 5 == 4 else M.reverse_complement(read) if c % 2 else read)
        begins.append(begin)
    reads = np.stack(reads)
    mapper = B.ReferenceMapper(ref, w_len, stride)
    a, n_windows = mapper.aligner, mapper.n_windows
    assert mapper.starts[-1] % stride != 0
    a.set_subjects(reads, qlen=w_len)
    assert a.wn == (n + 31) // 32
    mapper._build_rows(None, 0, 2 * n_windows)
    tile = a.score().cpu().numpy().astype(np.int64)                                        # [2 n_windows, 128]

    n_pairs = 333                                                                          # no multiple of 64
    windows = rng.integers(0, 2 * n_windows, size=n_pairs).astype(np.int32)
    subjects = rng.integers(0, ns, size=n_pairs).astype(np.int64)
    windows[:4] = [n_windows - 1, 2 * n_windows - 1, 0, n_windows]                         # the anchored window on both strands
    for p, c in enumerate(range(ns), start=30):       # every read once in a window that holds its source whole: W - S >= n + spare
        home = min(begins[c] // stride, n_windows - 1)
        subjects[p], windows[p] = c, home + (n_windows if c % 2 and c % 5 != 4 else 0)
    nobody = {10: -1, 11: 128, 12: -5}                                                     # the unused slot, the next bucket, below the base
    no_window = {20: -1, 21: 2 * n_windows, 22: 2 ** 31 - 1, 23: -2 ** 31}
    for p, s in nobody.items():
        subjects[p] = s
    for p, g in no_window.items():
        windows[p] = g
    base = 1 << 33                                                                         # a nonzero subject_base
    d_subjects = torch.from_numpy(np.where(subjects == -1, -1, subjects + base)).cuda()
    d_windows = torch.from_numpy(windows).cuda()
    distance = torch.full((n_pairs + 64,), SENT, dtype=torch.int32, device="cuda")
    need = int(B.lib().bgsa_hip_reference_verify_workspace_bytes(w_len, n, n_pairs))
    assert (need > 0) == (n > 512)
    work = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

    def run(out, work_bytes):
        B.check(B.lib().bgsa_hip_reference_verify_pairs_dev(mapper.d_reference.data_ptr(), ref_len, w_len, stride, a.d_peq.data_ptr(), n, a.ns,
                                                            a.wn, d_windows.data_ptr(), d_subjects.data_ptr(), n_pairs, base, out.data_ptr(),
                                                            work.data_ptr() if need else None, work_bytes, None), "verify")
    run(distance, need)
    a.check_faults()
    got = distance.cpu().numpy()
    assert (got[n_pairs:] == SENT).all()
    owned = np.array([p not in nobody and p not in no_window for p in range(n_pairs)])
    assert (got[:n_pairs][~owned] == SENT).all(), "a pair nobody owns, or one without a window, was written"
    want = -tile[windows[owned], subjects[owned]]
    assert np.array_equal(got[:n_pairs][owned], want)
    assert (want <= 8).sum() >= 50 and (windows[owned] >= n_windows).sum() >= 100
    if need:                                                                               # one wave's workspace: the list in chunks
        again = torch.full((n_pairs + 64,), SENT, dtype=torch.int32, device="cuda")
        run(again, int(B.lib().bgsa_hip_reference_verify_workspace_bytes(w_len, n, 0)))
        a.check_faults()
        assert torch.equal(again, distance)


# ---- 4. selection -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 9, 64])
def test_select_equals_the_helper(torch_gpu, k):
    torch = torch_gpu
    rng = np.random.default_rng(k)
    bound = 5
    lengths = [0, 1, k - 1, k, k + 1, 0, 200, 3, 64, 65, 0] + [int(x) for x in rng.integers(0, 3 * k + 2, size=20)]
    lengths = [max(x, 0) for x in lengths]
    ids, dist, segments = [], [], [0]
    for length in lengths:
        ids += sorted(rng.choice(5000, size=length, replace=False).tolist())
        dist += rng.integers(-1, bound + 4, size=length).tolist()                            # few values: ties; -1 and beyond the bound
        segments.append(len(ids))
    n_reads = len(lengths)
    d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
    d_dist = torch.tensor(dist, dtype=torch.int32, device="cuda")
    d_seg = torch.tensor(segments, dtype=torch.int64, device="cuda")
    scores = torch.full((n_reads + 2, k), SENT, dtype=torch.int32, device="cuda")
    hits = torch.full((n_reads + 2, k), SENT, dtype=torch.int32, device="cuda")
    B.check(B.lib().bgsa_hip_seed_select_dev(d_ids.data_ptr(), d_dist.data_ptr(), d_seg.data_ptr(), n_reads, bound, k, scores.data_ptr(),
                                             hits.data_ptr(), None), "select")
    torch.cuda.synchronize()
    scores, hits = scores.cpu().numpy(), hits.cpu().numpy()
    assert (scores[n_reads:] == SENT).all() and (hits[n_reads:] == SENT).all()
    tied = 0
    for r in range(n_reads):
        mine = slice(segments[r], segments[r + 1])
        want_scores, want_hits = R.select(ids[mine], dist[mine], bound, k)
        assert np.array_equal(scores[r], want_scores) and np.array_equal(hits[r], want_hits), r
        tied += int((np.diff(want_scores[want_hits >= 0]) == 0).sum())
    assert k == 1 or tied >= 10


def test_the_four_steps_compose_to_select_seeded(torch_gpu, case):
    torch, mapper, reads = torch_gpu, case["mapper"], case["reads"]
    ns, k_sel = reads.shape[0], mapper.k_selected(3)
    cap = max(mapper.n_ids // 8, 256)
    d_rows, d_lens = mapper.aligner._set_bucket(reads, qlen=W)
    assert d_lens is None
    want_scores, want_ids, want_counts, _ = mapper.select_seeded(d_rows, ns, N, BOUND, Q, k_sel, cap, block_rows=ns)
    job = mapper.seed_bucket(d_rows, N, BOUND, Q)
    scores = torch.full((ns, k_sel), SENT, dtype=torch.int32, device="cuda")
    ids, counts = torch.full_like(scores, SENT), torch.full((ns,), SENT, dtype=torch.int32, device="cuda")
    cand_read, cand_window = mapper.seed_candidates(job, 0, ns, cap, counts)
    pair_read, pair_window = mapper.seed_dedupe(cand_read, cand_window)
    distance = mapper.seed_verify(job, 0, pair_read, pair_window)
    mapper.seed_select(job, 0, ns, pair_read, pair_window, distance, k_sel, scores, ids)
    mapper.aligner.check_faults()
    seeded = ~case["flagged"]
    assert cand_read.numel() == sum(len(c) for c, f in zip(case["cands"], case["flagged"]) if not f)
    assert pair_read.numel() == sum(len(set(c)) for c, f in zip(case["cands"], case["flagged"]) if not f) == distance.numel()
    for got, want in ((scores, want_scores), (ids, want_ids), (counts, want_counts)):
        assert got.dtype == want.dtype and torch.equal(got, want)
    assert np.array_equal(ids.cpu().numpy()[seeded], R.blank(case["full"][3], BOUND)["windows"][seeded])     # and to map_reads' lists


# ---- 5. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_best", [1, 3])
def test_map_reads_seeded_equals_the_blanked_map_reads_and_host_pipeline(case, k_best):
    mapper = case["mapper"]
    got = mapper.map_reads_seeded(case["reads"], k_best=k_best, max_distance=BOUND)
    stats = mapper.last_seed_stats
    assert stats["reads_fallback_cap"] == 0 and stats["reads_fallback_n"] == int(case["flagged"].sum()) <= 8
    assert stats["reads_seeded"] == 128 - stats["reads_fallback_n"] and stats["seed_len"] == Q
    seeded = ~case["flagged"]
    assert stats["candidates_emitted"] == sum(len(c) for c, f in zip(case["cands"], case["flagged"]) if not f)
    assert stats["candidates_unique"] == sum(len(set(c)) for c, f in zip(case["cands"], case["flagged"]) if not f)
    k_sel = mapper.k_selected(k_best)
    assert got.scores.shape == (128, k_sel)
    assert_same_hits(got, R.blank(case["full"][k_best], BOUND), "against the blanked map_reads")
    assert_same_hits(got, B.blank_beyond(case["full"][k_best], BOUND), "against blank_beyond")
    host = dict(case["host"])                       # k_best = 3; slot r of a list depends on the slots in front of it only
    for name in FIELDS:
        host[name] = host[name][:, :k_sel]
    host["cigars"] = [row[:k_sel] for row in host["cigars"]]
    assert_same_hits(got, R.blank(host, BOUND), "against the blanked host pipeline")
    within = (case["full"][k_best].windows >= 0) & (-case["full"][k_best].scores.astype(np.int64) <= BOUND)
    assert stats["candidates_within_bound"] >= within[seeded].sum() and (~within).sum() > 100       # blanking did something
    assert got.keep.sum() >= 124 and ((got.strand == 1) & (got.keep == 1)).sum() >= 50


def test_the_cap_never_changes_a_result(case):
    mapper, want = case["mapper"], R.blank(case["full"][3], BOUND)
    counts = np.array([R.count_or_flag(c, f, 8) for c, f in zip(case["cands"], case["flagged"])])
    got = mapper.map_reads_seeded(case["reads"], k_best=3, max_distance=BOUND, max_candidates=8)
    assert_same_hits(got, want, "with max_candidates = 8")
    stats = mapper.last_seed_stats
    assert stats["reads_fallback_cap"] == (counts == -2).sum() and stats["reads_fallback_n"] == (counts == -1).sum()
    repeats = np.array([k == "repeat" for k in case["kinds"]])
    assert (counts[repeats & ~case["flagged"]] == -2).all()                              # the repeat reads fall back
    got = mapper.map_reads_seeded(case["reads"], k_best=3, max_distance=BOUND, max_candidates=0)
    assert_same_hits(got, want, "with max_candidates = 0")
    stats = mapper.last_seed_stats
    nothing = sum(1 for c, f in zip(case["cands"], case["flagged"]) if not f and not c)
    assert stats["reads_seeded"] == nothing <= 4 and stats["candidates_emitted"] == 0


@pytest.mark.parametrize("block_rows", [1, 7, 1000])
def test_blocks_do_not_change_a_result(case, block_rows):
    got = case["mapper"].map_reads_seeded(case["reads"], k_best=3, max_distance=BOUND, block_rows=block_rows)
    assert_same_hits(got, R.blank(case["full"][3], BOUND), f"with blocks of {block_rows} reads")


@pytest.mark.parametrize("seed_len", [3, 6])
def test_seed_lengths_do_not_change_a_result(case, seed_len):
    got = case["mapper"].map_reads_seeded(case["reads"], k_best=3, max_distance=BOUND, seed_len=seed_len, max_candidates=10 ** 6)
    assert_same_hits(got, R.blank(case["full"][3], BOUND), f"with seeds of {seed_len} bp")
    assert case["mapper"].last_seed_stats["seed_len"] == seed_len and case["mapper"].last_seed_stats["reads_fallback_cap"] == 0
    assert {Q, seed_len} <= set(case["mapper"].seed_indexes)                                # the index is kept per seed_len


def test_forward_strand_only(case):
    mapper = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    got = mapper.map_reads_seeded(case["reads"], k_best=3, max_distance=BOUND)
    assert_same_hits(got, R.blank(mapper.map_reads(case["reads"], k_best=3, max_distance=BOUND), BOUND), "on the forward strand")
    assert got.windows.max() < mapper.n_windows and not (got.strand == 1).any()
    assert mapper.last_seed_stats["reads_fallback_n"] == sum(R.has_n_piece(r, BOUND, Q, both_strands=False) for r in case["reads"])


# ---- 6. bound and optimum ---------------------------------------------------------------------------------------------------
def test_reads_within_the_bound_lead_with_their_optimum(case):
    ref, reads = case["ref"], case["reads"]
    got = case["mapper"].map_reads_seeded(reads, k_best=1, max_distance=BOUND)
    optimum = np.minimum(whole_reference_optimum(ref, reads), whole_reference_optimum(ref, np.stack([M.reverse_complement(r) for r in reads])))
    within = optimum <= BOUND
    planted = np.array([k != "unrelated" for k in case["kinds"]])
    assert within[planted].all() and not within[~planted].any(), "the case is broken"
    assert np.array_equal(-got.scores[within, 0], optimum[within]) and (got.keep[within, 0] == 1).all()
    assert (got.ref_begin[within, 0] >= 0).all() and all(got.cigars[c][0] for c in np.flatnonzero(within))
    for c in np.flatnonzero(~within):             # an unrelated read has only unused slots
        assert (got.scores[c] == R.INT32_MIN).all() and (got.windows[c] == -1).all() and (got.strand[c] == -1).all()
        assert (got.ref_begin[c] == -1).all() and (got.ref_end[c] == -1).all() and (got.keep[c] == 0).all()
        assert all(t is None for t in got.cigars[c])


# ---- 7. the workload's geometry on a small reference ------------------------------------------------------------------------
def test_workload_geometry_on_a_small_reference(torch_gpu):
    ref_len, w_len, stride, n, bound, q = 200_000, 400, 239, 150, 12, 11
    rng = np.random.default_rng(150)
    ref = ACGT[rng.integers(4, size=ref_len)]
    reads = []
    for c in range(496):
        begin = int(rng.integers(0, ref_len - n - 12))
        read = np.array(_edit(rng, list(ref[begin: begin + n + 12]), c % 13, ACGT)[:n], np.uint8)          # 0..12 edits, indels among them
        reads.append(M.reverse_complement(read) if c % 2 else read)
    reads += [ACGT[rng.integers(4, size=n)] for _ in range(16)]
    reads = np.stack(reads)
    assert B.max_stride(w_len, n, bound) == stride and B.seed_plan(n, bound) == (bound, q, q)
    mapper = B.ReferenceMapper(ref, w_len, stride)
    want = B.blank_beyond(mapper.map_reads(reads, k_best=1, max_distance=bound), bound)
    got = mapper.map_reads_seeded(reads, k_best=1, max_distance=bound)
    assert_same_hits(got, want, "on the workload's geometry")
    stats = mapper.last_seed_stats
    assert stats["reads_seeded"] == 512 and stats["max_candidates"] == max(mapper.n_ids // 8, 256)
    assert 496 <= stats["candidates_unique"] < 512 * mapper.n_ids // 100                    # the filter does not pass everything
    assert (got.keep[:496, 0] == 1).sum() >= 480 and (got.windows[496:] == -1).all()


# ---- 8. refusals before any launch ------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(torch_gpu):
    ref, reads, _ = make_case()
    mapper = B.ReferenceMapper(ref, W, S)

    def untouched():
        return not hasattr(mapper.aligner, "d_peq") and mapper.d_rows is None and not mapper.seed_indexes and mapper.last_seed_stats is None

    with pytest.raises(B.BgsaHipError, match=r"rc=-1.*seed_len 7 allows max_distance <= 3; max_distance 4 allows seed_len <= 6"):
        mapper.map_reads_seeded(reads, max_distance=BOUND, seed_len=7)
    with pytest.raises(B.BgsaHipError, match="allows no seed"):
        mapper.map_reads_seeded(reads, max_distance=N)
    with pytest.raises(B.BgsaHipError, match="max_distance is required"):
        mapper.map_reads_seeded(reads)
    with pytest.raises(B.BgsaHipError, match="1,024"):
        mapper.map_reads_seeded(np.full((2, 1025), ord("A"), np.uint8), max_distance=2)
    for k_best in (0, 65):
        with pytest.raises(B.BgsaHipError, match="k_best must lie in 1..64"):
            mapper.map_reads_seeded(reads, k_best=k_best, max_distance=BOUND)
    with pytest.raises(B.BgsaHipError, match="cigar_cap"):
        mapper.map_reads_seeded(reads, max_distance=BOUND, cigar_cap=0)
    with pytest.raises(B.BgsaHipError, match="max_candidates"):
        mapper.map_reads_seeded(reads, max_distance=BOUND, max_candidates=-1)
    assert untouched()
    wide = B.ReferenceMapper(ref, W, 62)
    with pytest.raises(B.BgsaHipError, match="rc=-1.*largest stride allowed is 61"):
        wide.map_reads_seeded(reads, max_distance=BOUND)
    assert not hasattr(wide.aligner, "d_peq") and not wide.seed_indexes
    assert untouched()

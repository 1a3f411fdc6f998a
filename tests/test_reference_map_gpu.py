"""A reference as the query set, on the MI355X: the window rows of bgsa_hip_reference_windows_dev byte for byte (range form and
id-list form, an unaligned buffer between sentinels), bgsa_amd.ReferenceMapper.map_reads bit for bit against the host pipeline of
tests/reference_map_reference.py and against the whole-reference optimum, and bgsa_hip_reference_placements_dev alone."""
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import reference_map_reference as M  # noqa: E402
import trace_reference as T  # noqa: E402
from align_reference import CHAR_OP, classes  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
GUARD = 64            # sentinel bytes on both sides of an output buffer
SENT = 0xAB


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


# ---- 1. window rows ---------------------------------------------------------------------------------------------------------
def build_rows(torch, mapper, calls, n_rows, offset):
    """Runs `calls` = [(ids | None, first_id, rows, row offset)] into one buffer of n_rows rows that starts `offset` bytes into an
    allocation, GUARD sentinel bytes on both sides; returns the rows' bytes after checking the sentinels."""
    W = mapper.window_len
    total = n_rows * (W + 1)
    whole = torch.full((offset + total + GUARD,), SENT, dtype=torch.uint8, device="cuda")
    assert offset >= GUARD and whole.data_ptr() % 4 == 0
    for ids, first, rows, at in calls:
        d_ids = None if ids is None else torch.tensor(ids, dtype=torch.int32, device="cuda")
        B.check(B.lib().bgsa_hip_reference_windows_dev(mapper.d_reference.data_ptr(), mapper.ref_len, W, mapper.stride,
                                                       None if d_ids is None else d_ids.data_ptr(), first, rows,
                                                       whole.data_ptr() + offset + at * (W + 1), None), "reference_windows_dev")
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert (got[:offset] == SENT).all() and (got[offset + total:] == SENT).all(), "a byte outside the rows was written"
    return got[offset: offset + total]


def reference_1000():
    rng = np.random.default_rng(1000)
    ref = np.frombuffer(b"ACGTN", np.uint8)[rng.choice(5, size=1000, p=[0.23, 0.23, 0.23, 0.23, 0.08])].copy()
    ref[517] = ord("x")        # outside the alphabet: class 0, complements to 'T'
    return ref


@pytest.mark.parametrize("offset", [GUARD + 1, GUARD + 2, GUARD + 3, GUARD + 4])
def test_window_rows_range_form(torch_gpu, offset):
    ref = reference_1000()
    mapper = B.ReferenceMapper(ref, 64, 40)
    n = mapper.n_windows
    assert n == 25 and mapper.starts[-1] == 936 and mapper.starts[-1] % 40 != 0       # the last window is anchored
    want = M.rows_buffer(M.window_rows(classes(ref), 64, 40, range(2 * n)))
    one = build_rows(torch_gpu, mapper, [(None, 0, 2 * n, 0)], 2 * n, offset)
    assert np.array_equal(one, want)
    two = build_rows(torch_gpu, mapper, [(None, 0, 13, 0), (None, 13, 2 * n - 13, 13)], 2 * n, offset)
    assert np.array_equal(two, want)
    rows = want.reshape(2 * n, 65)
    assert (rows[:, 64] == ord("\n")).all() and rows[:, :64].max() == 4
    at = int(np.flatnonzero(mapper.starts <= 517)[-1])       # the byte outside the alphabet: 'A' forward, 'T' on the reverse strand
    col = 517 - int(mapper.starts[at])
    assert rows[at, col] == 0 and rows[n + at, 63 - col] == 3


def test_window_rows_id_list_form(torch_gpu):
    ref = reference_1000()
    mapper = B.ReferenceMapper(ref, 64, 40)
    n = mapper.n_windows
    rng = np.random.default_rng(5)
    ids = list(rng.permutation(2 * n)) + [-1, 2 * n, 7, 7, -2 ** 31, 2 ** 31 - 1]
    ids = [int(ids[i]) for i in rng.permutation(len(ids))]
    want = M.rows_buffer(M.window_rows(classes(ref), 64, 40, ids))
    got = build_rows(torch_gpu, mapper, [(ids, 12345, len(ids), 0)], len(ids), GUARD + 3)      # first_id is ignored
    assert np.array_equal(got, want)
    for r, g in enumerate(ids):
        if not 0 <= g < 2 * n:
            assert (want.reshape(-1, 65)[r, :64] == 4).all()


@pytest.mark.parametrize("shape", [(64, 64, 1), (1000, 33, 1), (1000, 1, 1)])
def test_window_rows_other_shapes(torch_gpu, shape):
    ref_len, W, S = shape
    ref = reference_1000()[:ref_len]
    mapper = B.ReferenceMapper(ref, W, S)
    n = mapper.n_windows
    want = M.rows_buffer(M.window_rows(classes(ref), W, S, range(2 * n)))
    assert np.array_equal(build_rows(torch_gpu, mapper, [(None, 0, 2 * n, 0)], 2 * n, GUARD + 1), want)
    ids = [2 * n - 1, -1, 0, n, n - 1]
    want = M.rows_buffer(M.window_rows(classes(ref), W, S, ids))
    assert np.array_equal(build_rows(torch_gpu, mapper, [(ids, 0, len(ids), 0)], len(ids), GUARD + 2), want)


def test_a_newline_in_the_reference_raises(torch_gpu):
    with pytest.raises(B.BgsaHipError, match="newline"):
        B.ReferenceMapper(b"ACGT\nACGT", 4, 2)


# ---- 2. end to end ------------------------------------------------------------------------------------------------------------
REF_LEN, W, S, N, BOUND, K_BEST = 3000, 96, 48, 32, 4, 3
REPEAT_AT, UNIT, COPIES = 1500, 40, 3


def make_case():
    """(reference, reads[128, 32], kinds, loci): kinds[c] names how read c was made, loci[c] = (strand, begin) of its source or None."""
    rng = np.random.default_rng(3000)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    ref[REPEAT_AT: REPEAT_AT + UNIT * COPIES] = np.tile(ACGT[rng.integers(4, size=UNIT)], COPIES)
    ref[[333, 2222, 2900]] = ord("N")
    reads, kinds, loci = [], [], []

    def add(kind, strand, begin, edits=0):
        room = min(N + 3, REF_LEN - begin)                   # three spare bases, so that a read with deletions is still all reference
        src = _edit(rng, list(ref[begin: begin + room]), edits if room == N + 3 else 0, ACGT)
        read = np.array(src[:N], np.uint8)
        assert read.size == N
        reads.append(M.reverse_complement(read) if strand else read)
        kinds.append(kind)
        loci.append((strand, begin))

    clear = [x for x in rng.permutation(REF_LEN - N - 3) if not REPEAT_AT - N - 3 < x < REPEAT_AT + UNIT * COPIES]
    for i in range(40):
        add("planted", 0, int(clear[i]), i % 4)
    for i in range(40):
        add("planted", 1, int(clear[40 + i]), i % 4)
    for i, m in enumerate((3, 7, 11, 19, 23, 40, 47, 55)):    # 16 bp before a multiple of the stride: whole in one window, clipped next door
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
        loci.append(None)
    assert len(reads) == 128
    return ref, np.stack(reads), kinds, loci


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


@pytest.fixture(scope="module")
def case(torch_gpu):
    ref, reads, kinds, loci = make_case()
    assert B.max_stride(W, N, BOUND) == 61 >= S
    mapper = B.ReferenceMapper(ref, W, S)
    got = mapper.map_reads(reads, k_best=K_BEST, max_distance=BOUND)
    want = M.map_reads_host(ref, W, S, reads, k_best=K_BEST, max_distance=BOUND)
    return dict(ref=ref, reads=reads, kinds=kinds, loci=loci, mapper=mapper, got=got, want=want)


def assert_same_hits(got, want, what=""):
    for name in ("scores", "windows", "strand", "ref_begin", "ref_end", "keep"):
        g, w = getattr(got, name), (want[name] if isinstance(want, dict) else getattr(want, name))
        assert g.shape == w.shape and np.array_equal(g, w), f"{name} differs {what}: {np.argwhere(g != w)[:5].tolist()}"
    assert got.cigars == (want["cigars"] if isinstance(want, dict) else want.cigars), f"the cigars differ {what}"


def test_map_reads_equals_the_host_pipeline(case):
    got = case["got"]
    assert got.scores.shape == (128, 9) and got.scores.dtype == np.int32 and got.ref_begin.dtype == np.int64
    assert_same_hits(got, case["want"])
    assert got.keep.sum() > 128 and (got.keep.sum(axis=1) >= 2).sum() >= 20          # several loci per read do occur (the repeat)
    assert ((got.strand == 1) & (got.keep == 1)).sum() >= 50


def test_best_window_is_the_optimum_over_the_whole_reference(case):
    ref, reads, got = case["ref"], case["reads"], case["got"]
    forward = whole_reference_optimum(ref, reads)
    reverse = whole_reference_optimum(ref, np.stack([M.reverse_complement(r) for r in reads]))
    optimum = np.minimum(forward, reverse)
    planted = np.array([k != "unrelated" for k in case["kinds"]])
    assert (optimum[planted] <= BOUND).all(), "a planted read is beyond the bound: the case is broken"
    assert (optimum[~planted] > BOUND).all()
    within = optimum <= BOUND
    assert np.array_equal(-got.scores[within, 0], optimum[within])
    for c in np.flatnonzero(planted):
        strand, begin = case["loci"][c]
        assert (forward[c] if strand == 0 else reverse[c]) == optimum[c] or case["kinds"][c] == "repeat"


def test_kept_hits_validate_on_the_forward_reference(case):
    ref, reads, got = case["ref"], case["reads"], case["got"]
    checked = 0
    for c, r in zip(*np.nonzero(got.keep)):
        begin, end = int(got.ref_begin[c, r]), int(got.ref_end[c, r])
        assert 0 <= begin <= end <= REF_LEN and got.strand[c, r] in (0, 1)
        runs = [(int(length), CHAR_OP[op]) for length, op in re.findall(r"(\d+)([=XID])", got.cigars[c][r])]
        read = M.reverse_complement(reads[c]) if got.strand[c, r] else reads[c]
        T.validate(ref[begin:end], read, T.FREE_QUERY, T.UNIT, int(got.scores[c, r]), (0, end - begin, 0, N), runs)
        checked += 1
    assert checked > 128
    assert all(t is None for c in range(128) for r, t in enumerate(got.cigars[c]) if not got.keep[c, r])


def test_a_planted_read_has_exactly_one_kept_hit_at_its_locus(case):
    got = case["got"]
    for c, (kind, locus) in enumerate(zip(case["kinds"], case["loci"])):
        if kind in ("unrelated", "repeat"):
            continue
        strand, begin = locus
        at_locus = (got.keep[c] == 1) & (got.strand[c] == strand) & (got.ref_begin[c] < begin + N) & (begin < got.ref_end[c])
        assert at_locus.sum() == 1, (c, kind, locus)
        if kind == "overlap":       # its best view is the hit that leads the list
            assert at_locus[0]
    views = 0
    for c, kind in enumerate(case["kinds"]):      # and a locus seen through two windows did lose its second view
        views += int(((got.keep[c] == 0) & (got.ref_begin[c] >= 0)).sum())
    assert views >= 40


def test_repeat_reads_report_several_copies(case):
    """A window reports ONE placement, so a copy shows only where some window's own best placement is that copy: every read
    from the repeat reports a copy, most report two or three, all an exact number of units apart."""
    got = case["got"]
    several = 0
    for c, kind in enumerate(case["kinds"]):
        if kind != "repeat":
            continue
        kept = np.flatnonzero((got.keep[c] == 1) & (got.scores[c] == 0))
        assert 1 <= kept.size <= COPIES, c
        several += kept.size >= 2
        begins = np.sort(got.ref_begin[c, kept])
        assert ((np.diff(begins) % UNIT) == 0).all() and (np.diff(begins) > 0).all()
        picked = B.ReferenceMapper.placements_of(got, K_BEST)[c]
        assert len(picked) <= K_BEST and picked[0].distance == 0 and picked[0].cigar == "32="
    assert several >= 12


# ---- 3. segments and blocks never change a result -----------------------------------------------------------------------------
def test_segments_and_blocks_do_not_change_a_result(case):
    small = B.ReferenceMapper(case["ref"], W, S, segment_windows=7)
    assert_same_hits(small.map_reads(case["reads"], k_best=K_BEST, max_distance=BOUND), case["got"], "with segments of 7 windows")
    assert_same_hits(case["mapper"].map_reads(case["reads"], k_best=K_BEST, max_distance=BOUND, block_rows=5), case["got"],
                     "with blocks of 5 reads")
    assert_same_hits(small.map_reads(case["reads"], k_best=K_BEST, max_distance=BOUND, block_rows=5), case["got"], "with both")


def test_max_distance_none_places_every_selected_hit(case):
    got = case["mapper"].map_reads(case["reads"][:40], k_best=1)
    want = M.map_reads_host(case["ref"], W, S, case["reads"][:40], k_best=1)
    assert_same_hits(got, want, "with max_distance=None")
    assert ((got.windows >= 0) == (got.ref_begin >= 0)).all()


def test_map_reads_takes_reads_beyond_1024_bp(torch_gpu):
    """33 words: the three other entry points refuse such a read, map_reads does not."""
    ref_len, w_len, stride, n, bound, edits = 3000, 1200, 100, 1056, 8, 3
    rng = np.random.default_rng(1056)
    ref = ACGT[rng.integers(4, size=ref_len)].copy()
    begins = (700, 1500)
    exact = ref[begins[0]: begins[0] + n].copy()
    edited = np.array(_edit(rng, list(ref[begins[1]: begins[1] + n + edits]), edits, ACGT)[:n], np.uint8)
    reads = np.stack([exact, M.reverse_complement(edited)])
    assert B.max_stride(w_len, n, bound) >= stride
    got = B.ReferenceMapper(ref, w_len, stride).map_reads(reads, k_best=1, max_distance=bound)
    for c, (strand, planted) in enumerate(((0, 0), (1, edits))):
        assert got.keep[c, 0] == 1 and got.strand[c, 0] == strand, c
        begin, end = int(got.ref_begin[c, 0]), int(got.ref_end[c, 0])
        assert 0 <= begin <= begins[c] + planted and begins[c] + n - planted <= end <= ref_len, (c, begin, end)
        assert -int(got.scores[c, 0]) <= planted and (planted or got.cigars[c][0] == f"{n}=")
        runs = [(int(length), CHAR_OP[op]) for length, op in re.findall(r"(\d+)([=XID])", got.cigars[c][0])]
        read = M.reverse_complement(reads[c]) if strand else reads[c]
        T.validate(ref[begin:end], read, T.FREE_QUERY, T.UNIT, int(got.scores[c, 0]), (0, end - begin, 0, n), runs)


# ---- 4. one strand ----------------------------------------------------------------------------------------------------------
def test_forward_strand_only(case):
    both = case["got"]
    mapper = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    got = mapper.map_reads(case["reads"], k_best=K_BEST, max_distance=BOUND)
    assert got.windows.max() < mapper.n_windows and not (got.strand == 1).any()
    worse = 0
    for c, (kind, locus) in enumerate(zip(case["kinds"], case["loci"])):
        if kind in ("planted", "overlap", "edge"):
            if locus[0] == 1:
                assert got.scores[c, 0] < both.scores[c, 0], c
                worse += 1
            else:
                assert got.scores[c, 0] == both.scores[c, 0], c
    assert worse >= 40
    assert_same_hits(got, M.map_reads_host(case["ref"], W, S, case["reads"], k_best=K_BEST, max_distance=BOUND, both_strands=False))


# ---- 5. a stride too large is refused before anything is launched --------------------------------------------------------------
def test_stride_beyond_max_stride_raises_before_any_launch(case):
    mapper = B.ReferenceMapper(case["ref"], W, 62)
    with pytest.raises(B.BgsaHipError, match="rc=-1.*largest stride allowed is 61"):
        mapper.map_reads(case["reads"], k_best=K_BEST, max_distance=BOUND)
    assert not hasattr(mapper.aligner, "d_peq") and mapper.d_rows is None         # no subjects preprocessed, no rows built
    exact = B.ReferenceMapper(case["ref"], W, 61)
    first = exact.map_reads(case["reads"][:16], k_best=1, max_distance=BOUND)
    saved = [np.array(x) for x in first[:5]] + [[list(row) for row in first.cigars]]
    peq = exact.aligner.d_peq
    with pytest.raises(B.BgsaHipError, match="largest stride allowed is 60"):
        exact.map_reads(case["reads"], k_best=1, max_distance=BOUND + 1)
    assert exact.aligner.d_peq is peq
    for before, after in zip(saved[:5], first[:5]):
        assert np.array_equal(before, after)
    assert saved[5] == first.cigars
    with pytest.raises(B.BgsaHipError, match="no stride"):
        B.ReferenceMapper(case["ref"], 40, 8).map_reads(case["reads"], max_distance=20)


# ---- 6. the placements call alone -----------------------------------------------------------------------------------------------
def test_placements_call_alone(torch_gpu):
    torch = torch_gpu
    ref_len, w_len, stride, k, n_reads, cap = 1000, 64, 40, 64, 65, 4
    n = M.window_count(ref_len, w_len, stride)
    rng = np.random.default_rng(6)
    hits = rng.integers(0, 2 * n, size=(n_reads, k)).astype(np.int32)
    hits[rng.random((n_reads, k)) < 0.15] = -1                   # unused slots
    hits[3, 5], hits[64, 63], hits[0, 0] = 2 * n, 2 ** 31 - 1, -7  # ids that are no window
    qb = rng.integers(0, 40, size=n_reads * k)
    qe = qb + rng.integers(0, 25, size=n_reads * k)
    qb[rng.random(n_reads * k) < 0.2] = -1                       # beyond the bound
    span = np.stack([qb, qe, np.zeros_like(qb), np.full_like(qb, 20)], axis=1).astype(np.int32)
    n_ops = rng.integers(0, 7, size=n_reads * k).astype(np.int32)      # 5 and 6 overflow a row of 4
    cigar = rng.integers(1, 2 ** 20, size=(n_reads * k, cap)).astype(np.int32)
    want = M.placements(ref_len, w_len, stride, hits, span, n_ops, cigar, cap)

    dev = [torch.from_numpy(x).cuda() for x in (hits, span, n_ops, cigar)]
    outs = [torch.full((n_reads, k), 99, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int64, torch.int32)]
    B.check(B.lib().bgsa_hip_reference_placements_dev(ref_len, w_len, stride, dev[0].data_ptr(), n_reads, k, dev[1].data_ptr(),
                                                      dev[2].data_ptr(), dev[3].data_ptr(), cap, *(t.data_ptr() for t in outs), None),
            "reference_placements_dev")
    torch.cuda.synchronize()
    for name, got, exp in zip(("strand", "ref_begin", "ref_end", "keep"), outs, want[:4]):
        assert np.array_equal(got.cpu().numpy(), exp), name
    got_cigar = dev[3].cpu().numpy()
    assert np.array_equal(got_cigar, want[4])
    reverse_placed = (hits.reshape(-1) >= n) & (hits.reshape(-1) < 2 * n) & (qb >= 0)
    over = reverse_placed & (n_ops > cap)
    flipped = reverse_placed & (n_ops >= 2) & (n_ops <= cap)
    assert over.sum() >= 100 and np.array_equal(got_cigar[over], cigar[over])          # an overflowing row's runs are untouched
    assert flipped.sum() >= 100 and not np.array_equal(got_cigar[flipped], cigar[flipped])
    assert np.array_equal(got_cigar[~reverse_placed], cigar[~reverse_placed])
    assert np.array_equal(dev[1].cpu().numpy(), span) and np.array_equal(dev[2].cpu().numpy(), n_ops)
    keep = want[3]
    assert 0 < keep.sum() < (want[1] >= 0).sum()                 # some placed hits were hidden by a better view

    # without runs: the same coordinates, nothing to reverse
    outs2 = [torch.full((n_reads, k), 99, dtype=dt, device="cuda") for dt in (torch.int32, torch.int64, torch.int64, torch.int32)]
    B.check(B.lib().bgsa_hip_reference_placements_dev(ref_len, w_len, stride, dev[0].data_ptr(), n_reads, k, dev[1].data_ptr(),
                                                      None, None, 0, *(t.data_ptr() for t in outs2), None), "reference_placements_dev")
    torch.cuda.synchronize()
    for a, b in zip(outs, outs2):
        assert torch.equal(a, b)

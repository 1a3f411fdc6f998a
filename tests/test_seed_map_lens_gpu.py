"""Seeded read mapping for reads of mixed lengths on the MI355X: the per-read candidate counts and lists against
tests/seed_map_reference.py, the per-lane verify kernel against the tile bgsa_hip_myers_place_score_lens_dev scores (every instance
of the ladder, both sides of the column-block switch), the lens calls against the equal-length calls where every length is the
width, and ReferenceMapper.map_reads_seeded_ragged bit for bit against the blanked map_reads_ragged and the whole-reference optimum."""
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
from test_seed_map_gpu import assert_same_hits  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = -77            # what an output holds where nobody may write
REF_LEN, W, S, BOUND = 3000, 160, 48, 4
REPEAT_AT, UNIT, COPIES = 1500, 40, 3
N_IDS = 2 * M.window_count(REF_LEN, W, S)
DEFAULT_CAP = max(N_IDS // 8, 256)


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def make_case():
    """(reference, reads: 128 arrays of 30..80 bp in shuffled order, kinds): planted on both strands with 0..3 edits, in window
    overlaps, at both edges, in the tandem repeat, and unrelated; three N in the reference.  Host only."""
    rng = np.random.default_rng(3001)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    ref[REPEAT_AT: REPEAT_AT + UNIT * COPIES] = np.tile(ACGT[rng.integers(4, size=UNIT)], COPIES)
    ref[[333, 2222, 2900]] = ord("N")
    lens = np.array([30, 32, 33, 64, 65, 80] + rng.integers(30, 81, size=122).tolist())
    rng.shuffle(lens)
    reads, kinds = [], []

    def add(kind, strand, begin, edits=0):
        n = int(lens[len(reads)])
        begin = min(begin, REF_LEN - n)
        room = min(n + 3, REF_LEN - begin)
        src = _edit(rng, list(ref[begin: begin + room]), edits if room == n + 3 else 0, ACGT)
        read = np.array(src[:n], np.uint8)
        assert read.size == n
        reads.append(M.reverse_complement(read) if strand else read)
        kinds.append(kind)

    clear = [x for x in rng.permutation(REF_LEN - 83) if not REPEAT_AT - 83 < x < REPEAT_AT + UNIT * COPIES]
    for i in range(96):
        add("planted", (i // 4) % 2, int(clear[i]), i % 4)
    for i, m in enumerate((3, 7, 11, 19, 23, 40, 47, 55)):
        add("overlap", 0, m * S - 16, i % 3)
        add("overlap", 1, (m + 1) * S - 16, i % 3)
    for strand in (0, 1):
        add("edge", strand, 0)
        add("edge", strand, REF_LEN)                     # clamped to REF_LEN - n: the read ends with the reference
    for i in range(4):
        add("repeat", 0, REPEAT_AT + 3 * i)
        add("repeat", 1, REPEAT_AT + 3 * i + 1)
    while len(reads) < 128:
        reads.append(ACGT[rng.integers(4, size=int(lens[len(reads)]))])
        kinds.append("unrelated")
    assert len(reads) == 128 and [r.size for r in reads] == lens.tolist()
    return ref, reads, kinds


def helper_counts(ref, reads, bound, q, cap, both=True, lookup=None):
    """(counts or flags, candidate lists) of tests/seed_map_reference.py for reads of one bin, every read at its own length."""
    if lookup is None:
        lookup = R.lookup_of(*R.index(classes(ref), q))
    L_, counts, lists = len(ref), [], []
    for read in reads:
        n = read.size
        b_r = min(bound, n)
        if n // (b_r + 1) < q:
            counts.append(-3)
            lists.append([])
        elif R.has_n_piece(read, b_r, q, both):
            counts.append(-1)
            lists.append([])
        else:
            cands = R.candidates(lookup, L_, W, S, read, b_r, q, both)
            counts.append(R.count_or_flag(cands, False, cap))
            lists.append(sorted(cands) if counts[-1] >= 0 else [])
    return np.array(counts), lists


def whole_reference_optimum_ragged(ref, reads):
    """min over i of D[i][n_r] with D[0][j] = j, D[i][0] = 0, unit costs over the classes, every read at its own length: one row step
    per reference base on rows padded with a class nothing matches (column n_r depends on the columns in front of it only)."""
    rc = classes(ref)
    lens = np.array([r.size for r in reads])
    sc = np.full((len(reads), int(lens.max())), 9, dtype=np.int64)
    for i, r in enumerate(reads):
        sc[i, : r.size] = classes(r)
    ramp = np.arange(sc.shape[1] + 1, dtype=np.int64)
    d = np.tile(ramp, (sc.shape[0], 1))
    rows = np.arange(len(reads))
    best = d[rows, lens].copy()
    for c in rc:
        t = np.empty_like(d)
        t[:, 0] = 0
        np.minimum(d[:, 1:] + 1, d[:, :-1] + (sc != c), out=t[:, 1:])
        d = np.minimum.accumulate(t - ramp, axis=1) + ramp
        np.minimum(best, d[rows, lens], out=best)
    return best


@pytest.fixture(scope="module")
def case(torch_gpu):
    """The case, what the helper says about it (host only, asserted before the GPU is touched), and the exhaustive results."""
    ref, reads, kinds = make_case()
    lens = [r.size for r in reads]
    assert {30, 32, 33, 64, 65, 80} <= set(lens) and min(lens) == 30 and max(lens) == 80
    plan = B.seed_plan_ragged(lens, BOUND)
    assert [((max(lens[i] for i in idx) + 31) // 32, q) for idx, q in plan] == [(1, 6), (2, 6), (3, 12)]
    flags = np.zeros(128, dtype=np.int64)
    cands = [None] * 128
    for idx, q in plan:
        counts, lists = helper_counts(ref, [reads[i] for i in idx], BOUND, q, DEFAULT_CAP)
        flags[idx] = counts
        for i, one in zip(idx.tolist(), lists):
            cands[i] = one
    assert (flags < 0).sum() <= 16, "too many flagged reads: the case would test the exhaustive path"
    assert B.max_stride(W, 80, BOUND) == 77 >= S
    mapper = B.ReferenceMapper(ref, W, S)
    full = {k: mapper.map_reads_ragged(reads, k_best=k, max_distance=BOUND) for k in (1, 3)}
    return dict(ref=ref, reads=reads, lens=lens, kinds=kinds, plan=plan, flags=flags, cands=cands, mapper=mapper, full=full)


def upload_ragged(torch, reads):
    """(device rows, device lengths with the pad columns at the width, width) as set_reads_ragged packs a bucket."""
    rows, lens = B.pad_ragged(reads)
    padded, extra = B.pad_rows(rows)
    lens = np.concatenate([lens, np.full(extra, rows.shape[1], dtype=np.int32)]).astype(np.int32)
    return torch.from_numpy(B.rows_to_buffer(padded)).cuda(), torch.from_numpy(lens).cuda(), rows.shape[1]


# ---- 1. counts, flags and candidates ----------------------------------------------------------------------------------------
def run_count_emit_lens(torch, mapper, reads, bound, q, cap, both=True, d_lens=None, equal_length=False):
    """Count and emit for one bucket of reads; returns (counts, the sorted list per read, the raw emit arrays)."""
    L = B.lib()
    offsets, positions = mapper.seed_index(q)
    d_rows, lens, width = upload_ragged(torch, reads)
    lens = lens if d_lens is None else d_lens
    ns = len(reads)
    counts = torch.full((ns + 3,), SENT, dtype=torch.int32, device="cuda")
    shape = (mapper.ref_len, mapper.window_len, mapper.stride, offsets.data_ptr(), positions.data_ptr(), q)
    if equal_length:
        B.check(L.bgsa_hip_seed_count_candidates_dev(*shape, d_rows.data_ptr(), width, ns, bound, int(both), cap, counts.data_ptr(), None), "count")
    else:
        B.check(L.bgsa_hip_seed_count_candidates_lens_dev(*shape, d_rows.data_ptr(), lens.data_ptr(), width, ns, bound, int(both), cap,
                                                          counts.data_ptr(), None), "count lens")
    torch.cuda.synchronize()
    got = counts.cpu().numpy()
    assert (got[ns:] == SENT).all()
    got = got[:ns]
    sizes = np.maximum(got, 0).astype(np.int64)
    prefix = np.cumsum(sizes) - sizes
    total = int(sizes.sum())
    out_read = torch.full((total + 5,), SENT, dtype=torch.int32, device="cuda")
    out_window = torch.full((total + 5,), SENT, dtype=torch.int32, device="cuda")
    d_prefix = torch.from_numpy(prefix).cuda()
    if equal_length:
        B.check(L.bgsa_hip_seed_emit_candidates_dev(*shape, d_rows.data_ptr(), width, ns, bound, int(both), counts.data_ptr(),
                                                    d_prefix.data_ptr(), 1000, out_read.data_ptr(), out_window.data_ptr(), None), "emit")
    else:
        B.check(L.bgsa_hip_seed_emit_candidates_lens_dev(*shape, d_rows.data_ptr(), lens.data_ptr(), width, ns, bound, int(both),
                                                         counts.data_ptr(), d_prefix.data_ptr(), 1000, out_read.data_ptr(),
                                                         out_window.data_ptr(), None), "emit lens")
    torch.cuda.synchronize()
    out_read, out_window = out_read.cpu().numpy(), out_window.cpu().numpy()
    assert (out_read[total:] == SENT).all() and (out_window[total:] == SENT).all()     # a flagged read writes no slot
    lists = []
    for c in range(ns):
        mine = slice(int(prefix[c]), int(prefix[c] + sizes[c]))
        assert (out_read[mine] == 1000 + c).all()                                        # read_base + r
        lists.append(sorted(out_window[mine].tolist()))
    return got, lists, (out_read, out_window)


def test_counts_flags_and_candidates_equal_the_helper_per_bin(torch_gpu, case):
    seeded = 0
    for idx, q in case["plan"]:
        reads = [case["reads"][i] for i in idx]
        got, lists, _ = run_count_emit_lens(torch_gpu, case["mapper"], reads, BOUND, q, DEFAULT_CAP)
        assert np.array_equal(got, case["flags"][idx]), q
        for c, i in enumerate(idx.tolist()):
            assert lists[c] == case["cands"][i], (q, i)
        seeded += int((got > 0).sum())
    assert seeded >= 108 and (case["flags"] == -3).sum() == 0


def test_a_cap_of_8_flags_the_reads_above_it(torch_gpu, case):
    above = exact = 0
    for idx, q in case["plan"]:
        reads = [case["reads"][i] for i in idx]
        want, want_lists = helper_counts(case["ref"], reads, BOUND, q, 8)
        got, lists, _ = run_count_emit_lens(torch_gpu, case["mapper"], reads, BOUND, q, 8)
        assert np.array_equal(got, want) and lists == want_lists
        above += int((want == -2).sum())
        exact += int((want >= 0).sum())
    assert above >= 24 and exact >= 1


def test_a_seed_of_8_flags_exactly_the_reads_too_short_for_it(torch_gpu, case):
    short = 0
    for idx, _ in case["plan"]:
        reads = [case["reads"][i] for i in idx]
        want, want_lists = helper_counts(case["ref"], reads, BOUND, 8, 10 ** 6)
        got, lists, _ = run_count_emit_lens(torch_gpu, case["mapper"], reads, BOUND, 8, 10 ** 6)
        assert np.array_equal(got, want) and lists == want_lists
        too_short = np.array([r.size // (min(BOUND, r.size) + 1) < 8 for r in reads])
        assert np.array_equal(got == -3, too_short)
        short += int(too_short.sum())
    assert short >= 5 and all(n >= 40 or n // 5 < 8 for n in case["lens"])       # 30 .. 39 bp: step 6 or 7


def test_counts_on_the_forward_strand_only(torch_gpu, case):
    forward = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    for idx, q in case["plan"]:
        reads = [case["reads"][i] for i in idx[::3]]
        want, want_lists = helper_counts(case["ref"], reads, BOUND, q, 10 ** 6, both=False)
        got, lists, _ = run_count_emit_lens(torch_gpu, forward, reads, BOUND, q, 10 ** 6, both=False)
        assert np.array_equal(got, want) and lists == want_lists
        assert all(g < forward.n_windows for one in lists for g in one)


def test_lengths_outside_the_row_are_clamped(torch_gpu, case):
    """A length above the width counts as the width, a negative one as 0 (flag -3): neither forms an index outside the row."""
    reads = [case["reads"][i] for i in case["plan"][0][0][:64]]
    d_rows, lens, width = upload_ragged(torch_gpu, reads)
    odd = lens.clone()
    odd[0], odd[1], odd[2] = 10 ** 6, -5, 0
    got, lists, _ = run_count_emit_lens(torch_gpu, case["mapper"], reads, BOUND, 6, 10 ** 6, d_lens=odd)
    padded = np.concatenate([reads[0], np.full(width - reads[0].size, ord("N"), np.uint8)])     # the row at its full width
    want, want_lists = helper_counts(case["ref"], [padded] + reads[1:], BOUND, 6, 10 ** 6)
    want[1:3] = -3
    want_lists[1] = want_lists[2] = []
    assert np.array_equal(got, want) and lists == want_lists


# ---- 2. the verify kernel against the scored tile -----------------------------------------------------------------------------
def ragged_lengths(rng, width, count):
    """1, 31, 32, 33, width - 1, width and both sides of every multiple of 32 the width allows, filled up at random."""
    want = {1, 31, 32, 33, width - 1, width}
    for k in range(32, width + 32, 32):
        want |= {k - 1, k + 1}
    want = sorted(x for x in want if 1 <= x <= width)
    assert len(want) <= count
    return want + [int(x) for x in rng.integers(1, width + 1, size=count - len(want))]


@pytest.mark.parametrize("width", [32, 33, 64, 96, 128, 150, 192, 256, 384, 512, 513, 1024])
def test_verify_lens_equals_the_scored_tile(torch_gpu, width):
    torch = torch_gpu
    rng = np.random.default_rng(width)
    ref_len, w_len, stride, ns, spare = 3000, width + 48, 37, 70, 8
    ref = ACGT[rng.integers(4, size=ref_len)].copy()
    ref[rng.integers(ref_len, size=12)] = ord("N")
    lens = ragged_lengths(rng, width, ns)
    reads, begins = [], []
    for c, n in enumerate(lens):
        begin = int(rng.integers(0, ref_len - n - spare))
        if c % 7 == 6:
            begin = ref_len - n - spare                                                   # in the anchored last window
        read = np.array(_edit(rng, list(ref[begin: begin + n + spare]), int(rng.integers(0, spare + 1)), ACGT)[:n], np.uint8)
        assert read.size == n
        reads.append(ACGT[rng.integers(4, size=n)] if c % 5 == 4 else M.reverse_complement(read) if c % 2 else read)
        begins.append(begin)
    mapper = B.ReferenceMapper(ref, w_len, stride)
    a, n_windows = mapper.aligner, mapper.n_windows
    a.set_reads_ragged(reads, qlen=w_len)                                                  # ONE bucket, not binned
    assert a.reads_ragged and a.slen == width and a.wn == (width + 31) // 32 and a.ns == 128
    assert a.d_lens.cpu().numpy().tolist() == lens + [width] * 58
    mapper._build_rows(None, 0, 2 * n_windows)
    tile = a.score().cpu().numpy().astype(np.int64)                                        # [2 n_windows, 128], every read at its own length

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
    need = int(B.lib().bgsa_hip_reference_verify_workspace_bytes(w_len, width, n_pairs))
    assert (need > 0) == (width > 512)
    work = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

    def run(out, work_bytes):
        B.check(B.lib().bgsa_hip_reference_verify_pairs_lens_dev(mapper.d_reference.data_ptr(), ref_len, w_len, stride, a.d_peq.data_ptr(),
                                                                 a.d_lens.data_ptr(), width, a.ns, a.wn, d_windows.data_ptr(),
                                                                 d_subjects.data_ptr(), n_pairs, base, out.data_ptr(),
                                                                 work.data_ptr() if need else None, work_bytes, None), "verify lens")
    run(distance, need)
    a.check_faults()
    got = distance.cpu().numpy()
    assert (got[n_pairs:] == SENT).all()
    owned = np.array([p not in nobody and p not in no_window for p in range(n_pairs)])
    assert (got[:n_pairs][~owned] == SENT).all(), "a pair nobody owns, or one without a window, was written"
    want = -tile[windows[owned], subjects[owned]]
    assert np.array_equal(got[:n_pairs][owned], want), np.flatnonzero(got[:n_pairs][owned] != want)[:10].tolist()
    assert (want <= np.array(lens)[subjects[owned]]).all()                                 # a distance never exceeds the read's own length
    assert (want <= 8).sum() >= 50 and (windows[owned] >= n_windows).sum() >= 100
    if need:                                                                               # one wave's workspace: the list in chunks
        again = torch.full((n_pairs + 64,), SENT, dtype=torch.int32, device="cuda")
        run(again, int(B.lib().bgsa_hip_reference_verify_workspace_bytes(w_len, width, 0)))
        a.check_faults()
        assert torch.equal(again, distance)


def test_verify_lens_of_length_zero_is_distance_zero(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(5)
    ref = ACGT[rng.integers(4, size=500)]
    mapper = B.ReferenceMapper(ref, 96, 40)
    a = mapper.aligner
    a.set_subjects(np.stack([ref[100:140], ref[200:240]]), qlen=96)
    d_lens = torch.full((a.ns,), 40, dtype=torch.int32, device="cuda")
    d_lens[0], d_lens[1] = 0, -9                                                           # clamped to [0, read_len]
    windows = torch.tensor([2, 5, 0], dtype=torch.int32, device="cuda")
    subjects = torch.tensor([0, 1, 1], dtype=torch.int64, device="cuda")
    distance = torch.full((5,), SENT, dtype=torch.int32, device="cuda")
    B.check(B.lib().bgsa_hip_reference_verify_pairs_lens_dev(mapper.d_reference.data_ptr(), 500, 96, 40, a.d_peq.data_ptr(), d_lens.data_ptr(), 40,
                                                             a.ns, a.wn, windows.data_ptr(), subjects.data_ptr(), 3, 0, distance.data_ptr(), None, 0,
                                                             None), "verify lens")
    assert distance.cpu().numpy().tolist() == [0, 0, 0, SENT, SENT]


# ---- 3. every length equal to the width: the lens calls write what the equal-length calls write -----------------------------
def test_lens_calls_equal_the_equal_length_calls_when_every_length_is_the_width(torch_gpu):
    torch = torch_gpu
    rng = np.random.default_rng(33)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    ref[[500, 1500]] = ord("N")
    for n, w_len, stride, bound, q in ((40, 96, 40, 3, 6), (150, 200, 30, 5, 11), (600, 660, 50, 6, 12)):
        mapper = B.ReferenceMapper(ref, w_len, stride)
        begins = rng.integers(0, REF_LEN - n - 8, size=70)
        reads = [np.array(_edit(rng, list(ref[b: b + n + 8]), int(rng.integers(0, 7)), ACGT)[:n], np.uint8) for b in begins]
        reads = [M.reverse_complement(r) if c % 2 else r for c, r in enumerate(reads)]
        same = run_count_emit_lens(torch, mapper, reads, bound, q, 300)
        plain = run_count_emit_lens(torch, mapper, reads, bound, q, 300, equal_length=True)
        assert np.array_equal(same[0], plain[0]) and (same[0] >= 0).sum() >= 40
        assert np.array_equal(same[2][0], plain[2][0]) and np.array_equal(same[2][1], plain[2][1])     # the raw arrays, order included

        a = mapper.aligner
        a.set_subjects(np.stack(reads), qlen=w_len)
        d_lens = torch.full((a.ns,), n, dtype=torch.int32, device="cuda")
        n_pairs = 200
        windows = torch.from_numpy(rng.integers(0, 2 * mapper.n_windows, size=n_pairs).astype(np.int32)).cuda()
        subjects = torch.from_numpy(rng.integers(0, 70, size=n_pairs).astype(np.int64)).cuda()
        need = int(B.lib().bgsa_hip_reference_verify_workspace_bytes(w_len, n, n_pairs))
        work = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")
        tail = (n, a.ns, a.wn, windows.data_ptr(), subjects.data_ptr(), n_pairs, 0)
        head = (mapper.d_reference.data_ptr(), REF_LEN, w_len, stride, a.d_peq.data_ptr())
        out = [torch.full((n_pairs + 3,), SENT, dtype=torch.int32, device="cuda") for _ in range(2)]
        B.check(B.lib().bgsa_hip_reference_verify_pairs_dev(*head, *tail, out[0].data_ptr(), work.data_ptr() if need else None, need, None), "verify")
        B.check(B.lib().bgsa_hip_reference_verify_pairs_lens_dev(*head, d_lens.data_ptr(), *tail, out[1].data_ptr(),
                                                                 work.data_ptr() if need else None, need, None), "verify lens")
        assert torch.equal(out[0], out[1]) and (out[0][:n_pairs] >= 0).all() and (out[0][n_pairs:] == SENT).all()


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k_best", [1, 3])
def test_map_reads_seeded_ragged_equals_the_blanked_map_reads_ragged(case, k_best):
    mapper, flags = case["mapper"], case["flags"]
    got = mapper.map_reads_seeded_ragged(case["reads"], k_best=k_best, max_distance=BOUND)
    stats = mapper.last_seed_stats
    assert stats["reads_fallback_n"] == (flags == -1).sum() and stats["reads_fallback_cap"] == (flags == -2).sum()
    assert stats["reads_fallback_short"] == 0 and stats["reads_seeded"] == (flags >= 0).sum() >= 112
    assert [(b["words"], b["q"]) for b in stats["bins"]] == [(1, 6), (2, 6), (3, 12)]
    assert [b["reads"] for b in stats["bins"]] == [idx.size for idx, _ in case["plan"]]
    for b, (idx, _) in zip(stats["bins"], case["plan"]):
        assert b["emitted"] == sum(len(case["cands"][i]) for i in idx) and b["unique"] == sum(len(set(case["cands"][i])) for i in idx)
    assert stats["candidates_emitted"] == sum(b["emitted"] for b in stats["bins"]) > 0
    assert stats["candidates_unique"] == sum(b["unique"] for b in stats["bins"])
    k_sel = mapper.k_selected(k_best)
    assert got.scores.shape == (128, k_sel)
    want = B.blank_beyond(case["full"][k_best], BOUND)
    assert_same_hits(got, want, "against the blanked map_reads_ragged")
    assert_same_hits(got, R.blank(case["full"][k_best], BOUND), "against the helper's blanking")
    assert got.keep.sum() >= 120 and ((got.strand == 1) & (got.keep == 1)).sum() >= 40


def test_reads_within_the_bound_lead_with_their_optimum(case):
    ref, reads = case["ref"], case["reads"]
    got = case["mapper"].map_reads_seeded_ragged(reads, k_best=1, max_distance=BOUND)
    optimum = np.minimum(whole_reference_optimum_ragged(ref, reads),
                         whole_reference_optimum_ragged(ref, [M.reverse_complement(r) for r in reads]))
    within = optimum <= BOUND
    planted = np.array([k != "unrelated" for k in case["kinds"]])
    assert within[planted].all() and not within[~planted].any(), "the case is broken"
    assert np.array_equal(-got.scores[within, 0], optimum[within]) and (got.keep[within, 0] == 1).all()
    assert (got.ref_begin[within, 0] >= 0).all() and all(got.cigars[c][0] for c in np.flatnonzero(within))
    for c in np.flatnonzero(~within):             # an unrelated read has only unused slots
        assert (got.scores[c] == R.INT32_MIN).all() and (got.windows[c] == -1).all() and (got.keep[c] == 0).all()
        assert all(t is None for t in got.cigars[c])


# ---- 5. what never changes a result -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_candidates", [0, 8, None])
def test_the_cap_never_changes_a_result(case, max_candidates):
    mapper = case["mapper"]
    got = mapper.map_reads_seeded_ragged(case["reads"], k_best=3, max_distance=BOUND, max_candidates=max_candidates)
    assert_same_hits(got, B.blank_beyond(case["full"][3], BOUND), f"with max_candidates = {max_candidates}")
    stats = mapper.last_seed_stats
    if max_candidates == 0:        # everyone with a candidate takes the exhaustive path
        assert stats["candidates_emitted"] == 0 and stats["reads_seeded"] <= 8 and stats["reads_fallback_cap"] >= 108
    elif max_candidates == 8:
        assert stats["reads_fallback_cap"] >= 24 and stats["reads_seeded"] >= 1
    else:
        assert stats["max_candidates"] == DEFAULT_CAP and stats["reads_fallback_cap"] == (case["flags"] == -2).sum()


@pytest.mark.parametrize("block_rows", [1, 7, 1000])
def test_blocks_do_not_change_a_result(case, block_rows):
    got = case["mapper"].map_reads_seeded_ragged(case["reads"], k_best=3, max_distance=BOUND, block_rows=block_rows)
    assert_same_hits(got, B.blank_beyond(case["full"][3], BOUND), f"with blocks of {block_rows} reads")


@pytest.mark.parametrize("seed_len", [3, 6])
def test_seed_lengths_do_not_change_a_result(case, seed_len):
    mapper = case["mapper"]
    got = mapper.map_reads_seeded_ragged(case["reads"], k_best=3, max_distance=BOUND, seed_len=seed_len, max_candidates=10 ** 6)
    assert_same_hits(got, B.blank_beyond(case["full"][3], BOUND), f"with seeds of {seed_len} bp")
    stats = mapper.last_seed_stats
    assert stats["seed_len"] == seed_len and [b["q"] for b in stats["bins"]] == [seed_len] * 3
    assert stats["reads_fallback_cap"] == 0 and stats["reads_fallback_short"] == 0


def test_a_seed_too_long_for_some_reads_sends_them_through_the_exhaustive_path(case):
    mapper = case["mapper"]
    got = mapper.map_reads_seeded_ragged(case["reads"], k_best=3, max_distance=BOUND, seed_len=8)
    assert_same_hits(got, B.blank_beyond(case["full"][3], BOUND), "with seeds of 8 bp")
    assert mapper.last_seed_stats["reads_fallback_short"] == sum(n // 5 < 8 for n in case["lens"]) >= 5


def test_forward_strand_only(case):
    mapper = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    got = mapper.map_reads_seeded_ragged(case["reads"], k_best=3, max_distance=BOUND)
    assert_same_hits(got, B.blank_beyond(mapper.map_reads_ragged(case["reads"], k_best=3, max_distance=BOUND), BOUND), "on the forward strand")
    assert got.windows.max() < mapper.n_windows and not (got.strand == 1).any()
    assert mapper.last_seed_stats["reads_seeded"] >= 112


# ---- 6. one length: map_reads_seeded's own result ----------------------------------------------------------------------------
def test_a_list_of_one_length_equals_map_reads_seeded(case):
    rng = np.random.default_rng(64)
    ref, mapper = case["ref"], case["mapper"]
    begins = rng.integers(0, REF_LEN - 70, size=70)
    reads = np.stack([np.array(_edit(rng, list(ref[b: b + 67]), int(rng.integers(0, 4)), ACGT)[:64], np.uint8) for b in begins])
    reads[1::2] = np.stack([M.reverse_complement(r) for r in reads[1::2]])
    for k_best in (1, 3):
        want = mapper.map_reads_seeded(reads, k_best=k_best, max_distance=BOUND)
        want_stats = dict(mapper.last_seed_stats)
        got = mapper.map_reads_seeded_ragged(list(reads), k_best=k_best, max_distance=BOUND)
        assert_same_hits(got, want, "against map_reads_seeded")
        stats = mapper.last_seed_stats
        for name in ("reads_seeded", "reads_fallback_n", "reads_fallback_cap", "candidates_emitted", "candidates_unique", "candidates_within_bound"):
            assert stats[name] == want_stats[name], name
        assert [(b["words"], b["q"]) for b in stats["bins"]] == [(2, 12)] and want_stats["seed_len"] == 12
        assert (got.keep[:, 0] == 1).sum() >= 60


# ---- 7. refusals before any launch ------------------------------------------------------------------------------------------
def test_refusals_come_before_any_launch(torch_gpu):
    ref, reads, _ = make_case()
    mapper = B.ReferenceMapper(ref, W, S)

    def untouched(m=mapper):
        return not hasattr(m.aligner, "d_peq") and m.d_rows is None and not m.seed_indexes and m.last_seed_stats is None

    with pytest.raises(B.BgsaHipError, match="max_distance is required"):
        mapper.map_reads_seeded_ragged(reads)
    with pytest.raises(B.BgsaHipError, match="max_distance is required"):
        mapper.map_reads_seeded_ragged(reads, max_distance=None)
    with pytest.raises(B.BgsaHipError, match="1,024"):
        mapper.map_reads_seeded_ragged(reads + [np.full(1025, ord("A"), np.uint8)], max_distance=2)
    for k_best in (0, 65):
        with pytest.raises(B.BgsaHipError, match="k_best must lie in 1..64"):
            mapper.map_reads_seeded_ragged(reads, k_best=k_best, max_distance=BOUND)
    with pytest.raises(B.BgsaHipError, match="cigar_cap"):
        mapper.map_reads_seeded_ragged(reads, max_distance=BOUND, cigar_cap=0)
    with pytest.raises(B.BgsaHipError, match="max_candidates"):
        mapper.map_reads_seeded_ragged(reads, max_distance=BOUND, max_candidates=-1)
    with pytest.raises(B.BgsaHipError, match="1..13"):
        mapper.map_reads_seeded_ragged(reads, max_distance=BOUND, seed_len=14)
    with pytest.raises(B.BgsaHipError, match="negative"):
        mapper.map_reads_seeded_ragged(reads, max_distance=-1)
    assert untouched()
    wide = B.ReferenceMapper(ref, W, 78)
    with pytest.raises(B.BgsaHipError, match=r"rc=-1.*longest read \(80 bp\).*largest stride allowed is 77"):
        wide.map_reads_seeded_ragged(reads, max_distance=BOUND)
    assert untouched(wide) and untouched()

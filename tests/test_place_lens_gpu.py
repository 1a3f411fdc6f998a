"""Read placement on buckets of mixed read lengths, on the GPU: DeviceAligner.set_reads_ragged (Myers semi-global, every lane
right-aligned by its own length), its scores, hit lists and edit scripts, and ReferenceMapper.map_reads_ragged.

Expected scores come from the pinned oracle (oracle.dp_edit_semiglobal) called once per length class on the unpadded reads, and
the same tile is compared with this library's own equal-length path run on each length class alone.  The bytes behind every
read's end are adversarial — the source's own continuation (make_bucket's tails) — wherever a bucket is built by hand."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import oracle as O  # noqa: E402
import query_hits_reference as QH  # noqa: E402
import reference_map_reference as M  # noqa: E402
import trace_reference as T  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402
from test_ragged_gpu import LENS_150, by_class, make_bucket, set_padded_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ACGT = np.frombuffer(b"ACGT", np.uint8)
PEQ_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 18, 20, 22, 24, 25, 26, 28, 30, 32]   # myers_global.hip: PeqWidths
NEXT_WIDTH_UP = [9, 11, 23, 27, 31]                                                          # word counts that run at NW > word_num


def placer(q):
    a = B.DeviceAligner(B.ALGO_MYERS, DEV, semi_global=True)
    a.set_queries(q)
    return a


def adversarial_bucket(q, subjects, tails):
    """The bucket with the source's continuation behind every read's end, marked as set_reads_ragged marks it."""
    a = placer(q)
    set_padded_rows(a, subjects, tails)
    a.mark_reads_ragged()
    assert a.reads_ragged and a.d_lens is not None and a.ns % 64 == 0
    return a


def equal_length_path(q, subjects):
    """This library's equal-length semi-global launches, one per length class."""
    a = placer(q)

    def run(_, rows):
        a.set_subjects(rows)
        assert a.d_lens is None and not a.reads_ragged
        return a.score()[:, : a.ns_real].cpu().numpy()
    out = by_class(run, q, subjects)
    a.check_faults()
    return out


def scores_of(a):
    out = a.score()
    a.check_faults()
    return out[:, : a.ns_real].cpu().numpy()


@functools.lru_cache(maxsize=None)
def case1(ns=130):
    """5 words: qlen 200, 130 reads = three groups (not a multiple of a workgroup's four waves) and 62 pad columns; lengths of
    1..5 words in every wave.  Shared and never modified."""
    q, subjects, tails = make_bucket(0x91A0 + ns, 6, 200, [LENS_150[i % 16] for i in range(ns)])
    want = by_class(O.dp_edit_semiglobal, q, subjects)
    assert len(np.unique(want)) > 12                     # varied distances
    return q, subjects, tails, want


# ---- 1. five words, mixed word counts in one wave ------------------------------------------------------------------------------
def test_five_words_mixed_word_counts_in_one_wave():
    q, subjects, tails, want = case1()
    a = adversarial_bucket(q, subjects, tails)
    assert (a.ns, a.ns_real, a.extra, a.wn, a.slen) == (192, 130, 62, 5, 150)
    got = scores_of(a)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects))
    part = a.score(2, 5)                                 # a query sub-window: the same rows of the full call
    a.check_faults()
    assert np.array_equal(part[:, :130].cpu().numpy(), want[2:5])
    # the pad matters: the same rows scored at the full width differ somewhere
    b = placer(q)
    rows, _ = B.pad_ragged(subjects)
    for i, s in enumerate(subjects):
        rows[i, s.size:] = tails[i][: rows.shape[1] - s.size]
    b.set_subjects(rows)
    assert not np.array_equal(b.score()[:, :130].cpu().numpy(), want)


def test_five_words_through_set_reads_ragged():
    q, subjects, _, want = case1()
    a = placer(q)
    a.set_reads_ragged(subjects)
    assert a.reads_ragged and a.d_lens[a.ns_real:].cpu().tolist() == [a.slen] * a.extra      # pad columns get the longest length
    assert np.array_equal(scores_of(a), want)


def test_five_groups():
    q, subjects, tails, want = case1(320)
    a = adversarial_bucket(q, subjects, tails)
    assert a.ns == 320
    got = scores_of(a)
    assert np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects))


# ---- 2. every width ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", PEQ_WIDTHS + NEXT_WIDTH_UP, ids=lambda w: f"{w} words")
def test_every_width(w):
    base = [32 * (w - 1) + 1, 32 * w - 1, 32 * w, 1, 33, max(1, 32 * (w - 2) + 5)]
    pool = sorted({n for n in base if 1 <= n <= 32 * w})
    lens = [pool[i % len(pool)] for i in range(64)]
    q, subjects, tails = make_bucket(0x91B0 + w, 2, 32 * w + 40, lens)
    a = adversarial_bucket(q, subjects, tails)
    assert a.wn == w and a.slen == 32 * w and a.ns == 64
    got = scores_of(a)
    want = by_class(O.dp_edit_semiglobal, q, subjects)
    assert np.array_equal(got, want)
    assert np.array_equal(got, equal_length_path(q, subjects))


# ---- 3. all lengths equal, passed as a tensor ----------------------------------------------------------------------------------
def test_equal_lengths_as_a_tensor_is_the_equal_length_kernel():
    import torch
    q = O.gen_reads(0x91C0, 6, 200)
    s = O.mutate(np.tile(q[:, 20:170], (22, 1))[:128], np.arange(128) % 9, 0x91C1)
    a = placer(q)
    a.set_subjects(s)
    plain = a.score().cpu().numpy()
    a.set_subject_rows_device(torch.from_numpy(B.rows_to_buffer(s)).to(a.device), 128, 150,
                              d_lens=torch.full((128,), 150, dtype=torch.int32, device=a.device))
    a.mark_reads_ragged()
    a.ns_real, a.extra = 128, 0
    got = a.score().cpu().numpy()
    a.check_faults()
    assert np.array_equal(got, plain) and np.array_equal(got, O.dp_edit_semiglobal(q, s))


# ---- 4. traces -----------------------------------------------------------------------------------------------------------------
def cigar_runs(n_ops, row):
    return [(int(w) >> 4, int(w) & 15) for w in row[: int(n_ops)].view(np.uint32).tolist()]


def test_traces_are_the_length_class_own():
    q, subjects, tails, want = case1()
    a = adversarial_bucket(q, subjects, tails)
    cols = np.arange(48)                                   # every length three times, mutated and random reads
    pq = (cols * 5 + cols // 16) % 6
    score, span, n_ops, cigar = (t.cpu().numpy() for t in a.trace_pairs(pq, cols))
    a.check_faults()
    lens = np.array([subjects[c].size for c in cols])
    assert np.array_equal(score, want[pq, cols]) and np.array_equal(span[:, 3], lens) and (span[:, 2] == 0).all()
    b = placer(q)
    for n in np.unique(lens):
        mine = np.flatnonzero(lens == n)
        b.set_subjects(np.stack([subjects[cols[p]] for p in mine]))
        e_score, e_span, e_n_ops, e_cigar = (t.cpu().numpy() for t in b.trace_pairs(pq[mine], np.arange(mine.size)))
        assert np.array_equal(score[mine], e_score) and np.array_equal(span[mine], e_span) and np.array_equal(n_ops[mine], e_n_ops)
        for k, p in enumerate(mine):
            assert cigar_runs(n_ops[p], cigar[p]) == cigar_runs(e_n_ops[k], e_cigar[k])
    b.check_faults()
    for p, c in enumerate(cols):                           # every script against its unpadded read, on the host
        T.validate(q[pq[p]], subjects[c], T.FREE_QUERY, T.UNIT, int(score[p]), span[p], cigar_runs(n_ops[p], cigar[p]))
    # trace_hits goes the same way
    hit = np.stack([cols[:6], cols[6:12]], axis=1)
    h_score = a.trace_hits(hit)[0].cpu().numpy()
    assert np.array_equal(h_score, want[np.arange(6)[:, None], hit])


# ---- 5. hit lists --------------------------------------------------------------------------------------------------------------
def test_hit_lists_per_read():
    q, subjects, tails, want = case1()
    a = adversarial_bucket(q, subjects, tails)
    s, i = (t.cpu().numpy() for t in a.top_queries(3, block_rows=4))
    ws, wi = QH.top_queries(want, 130, 3, False)
    assert np.array_equal(s, ws) and np.array_equal(i, wi)
    cutoff = int(np.median(want))
    got = tuple(t.cpu().numpy() for t in a.threshold_queries(cutoff, 4, block_rows=4))
    assert QH.threshold_lists_equal(got, QH.threshold_queries(want, 130, cutoff, False, 4), 4)
    assert got[0].sum() > 0 and got[0].min() < 6          # the cutoff separates
    hs, hi = (t.cpu().numpy() for t in a.top_hits(2))
    assert np.array_equal(hs[:, 0], want.max(axis=1))
    a.check_faults()


# ---- 6. refusals ---------------------------------------------------------------------------------------------------------------
def test_refusals_leave_outputs_untouched():
    import torch
    q, subjects, tails, _ = case1()
    for a in (B.DeviceAligner(B.ALGO_MYERS, DEV, scores=(0, 1, 1), semi_global=True), B.DeviceAligner(B.ALGO_BITPAL, DEV, semi_global=True),
              B.DeviceAligner(B.ALGO_MYERS, DEV), B.DeviceAligner(B.ALGO_BITPAL, DEV, scores=(0, -1, -1))):
        a.set_queries(q)
        with pytest.raises(B.BgsaHipError, match="rc=-2"):
            a.set_reads_ragged(subjects)
        assert not hasattr(a, "d_peq") and a.d_lens is None and not a.reads_ragged       # before any allocation
        with pytest.raises(B.BgsaHipError, match="rc=-2"):
            a.mark_reads_ragged()
    # 33 words: set_reads_ragged refuses; a bucket marked by hand is refused by the scoring call, its output untouched
    long_reads = [O.gen_reads(0x91D0, 1, 1056)[0], O.gen_reads(0x91D1, 1, 700)[0]]
    a = placer(q)
    with pytest.raises(B.BgsaHipError, match="rc=-2.*1,024"):
        a.set_reads_ragged(long_reads)
    rows, lens = B.pad_ragged(long_reads)
    padded, extra = B.pad_rows(rows)
    lens = np.concatenate([lens, np.full(extra, 1056, np.int32)])
    a.ns_real, a.extra = 2, extra
    a.set_subject_rows_device(torch.from_numpy(B.rows_to_buffer(padded)).to(a.device), 64, 1056, d_lens=torch.from_numpy(lens).to(a.device))
    a.mark_reads_ragged()
    assert a.wn == 33
    out = torch.full((6, 64), 12345, dtype=torch.int16, device=a.device)
    with pytest.raises(B.BgsaHipError, match="rc=-2.*word_num > 32"):
        a.score(out=out)
    assert (out == 12345).all().item()
    # place_pairs_banded keeps refusing a mixed-length bucket; set_subjects_ragged on a semi-global aligner keeps raising at the
    # first scoring call
    a = adversarial_bucket(q, subjects, tails)
    with pytest.raises(B.BgsaHipError, match="rc=-2.*mixed read lengths"):
        a.place_pairs_banded([0], [0], 5)
    a.set_subjects_ragged(subjects)
    assert not a.reads_ragged
    out = torch.full((6, a.ns), 12345, dtype=torch.int16, device=a.device)
    with pytest.raises(B.BgsaHipError, match="rc=-2.*per-subject lengths"):
        a.score(out=out)
    assert (out == 12345).all().item()
    # equal lengths through set_reads_ragged IS set_subjects
    a.set_reads_ragged([s[:1].repeat(40) for s in subjects[:5]])
    assert a.d_lens is None and not a.reads_ragged and a.slen == 40


# ---- 7. the mapper -------------------------------------------------------------------------------------------------------------
REF_LEN, W, S, BOUND = 3000, 200, 30, 8


@functools.lru_cache(maxsize=None)
def mapper_case():
    rng = np.random.default_rng(0x91E0)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    reads, loci = [], []
    for i in range(130):
        n = int(rng.integers(33, 151))
        if i % 16 == 15:                                   # a few pure random reads
            reads.append(ACGT[rng.integers(4, size=n)].copy())
            loci.append(None)
            continue
        begin = int(rng.integers(0, REF_LEN - n - 3))
        src = _edit(rng, list(ref[begin: begin + n + 3]), i % 4, ACGT)      # three spare bases: a read with deletions is still all reference
        read = np.array(src[:n], np.uint8)
        strand = i % 2
        reads.append(M.reverse_complement(read) if strand else read)
        loci.append((strand, begin))
    return ref, reads, loci


def test_map_reads_ragged_equals_map_reads_per_length():
    ref, reads, loci = mapper_case()
    mapper = B.ReferenceMapper(ref, W, S, DEV)
    got = mapper.map_reads_ragged(reads, k_best=1, max_distance=BOUND)
    ns, k_sel = len(reads), mapper.k_selected(1)
    assert got.scores.shape == (ns, k_sel) and len(got.cigars) == ns
    lens = np.array([r.size for r in reads])
    assert len(B.bin_by_words(lens)) == 4 and len(np.unique(lens)) > 40
    for n in np.unique(lens):
        mine = np.flatnonzero(lens == n)
        one = mapper.map_reads(np.stack([reads[c] for c in mine]), k_best=1, max_distance=BOUND)
        for name in ("scores", "strand", "ref_begin", "ref_end", "keep", "windows"):
            assert np.array_equal(getattr(got, name)[mine], getattr(one, name)), (name, int(n))
        assert [got.cigars[c] for c in mine] == one.cigars, int(n)
    placed = 0
    for c, locus in enumerate(loci):                       # every planted read leads with its own locus and strand
        if locus is None:
            continue
        strand, begin = locus
        assert got.keep[c, 0] == 1 and got.strand[c, 0] == strand and -got.scores[c, 0] <= 3, c
        assert abs(int(got.ref_begin[c, 0]) - begin) <= 3 and got.cigars[c][0] is not None, (c, got.ref_begin[c, 0], begin)
        placed += 1
    assert placed == 122
    unplaced = (got.windows >= 0) & (-got.scores.astype(np.int64) > BOUND)
    assert unplaced.any() and (got.ref_begin[unplaced] == -1).all() and (got.keep[unplaced] == 0).all()
    assert all(got.cigars[c][r] is None for c, r in zip(*np.nonzero(unplaced)))


@pytest.mark.parametrize("max_distance", [2, None])      # None: the bin's worst selected distance, one scalar read back
def test_a_list_of_one_length_equals_map_reads(max_distance):
    ref, _, _ = mapper_case()
    rng = np.random.default_rng(64)
    begins = rng.integers(0, REF_LEN - 70, size=70)
    reads = np.stack([np.array(_edit(rng, list(ref[b: b + 67]), int(rng.integers(0, 4)), ACGT)[:64], np.uint8) for b in begins])
    reads[1::2] = np.stack([M.reverse_complement(r) for r in reads[1::2]])
    mapper = B.ReferenceMapper(ref, W, S, DEV)
    want = mapper.map_reads(reads, k_best=2, max_distance=max_distance)
    got = mapper.map_reads_ragged(list(reads), k_best=2, max_distance=max_distance)
    for name in ("scores", "strand", "ref_begin", "ref_end", "keep", "windows"):
        g, w = getattr(got, name), getattr(want, name)
        assert g.shape == w.shape == (70, mapper.k_selected(2)) and g.dtype == w.dtype and np.array_equal(g, w), name
    assert got.cigars == want.cigars
    if max_distance is None:      # every selected hit is placed
        assert (got.ref_begin[got.windows >= 0] >= 0).all() and (got.keep[:, 0] == 1).all()
    else:
        assert ((got.windows >= 0) & (got.ref_begin < 0)).any()


def test_map_reads_ragged_refuses_a_stride_the_longest_read_rules_out():
    ref, reads, _ = mapper_case()
    longest = max(r.size for r in reads)
    stride = B.max_stride(W, longest, BOUND) + 1
    mapper = B.ReferenceMapper(ref, W, stride, DEV)
    with pytest.raises(B.BgsaHipError, match="rc=-1.*longest read"):
        mapper.map_reads_ragged(reads, k_best=1, max_distance=BOUND)
    assert mapper.d_rows is None and not hasattr(mapper.aligner, "d_peq")        # before any launch
    # shorter reads alone pass the same mapper's rule
    short = [r for r in reads if r.size <= longest - 1][:3]
    mapper.map_reads_ragged(short, k_best=1, max_distance=BOUND)

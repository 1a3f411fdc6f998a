"""Paired reads on the MI355X: the rescue-windows kernel and the pair-selection kernel against tests/pair_reference.py, and
ReferenceMapper.map_pairs against the host pipeline field by field — seeded and exhaustive, in blocks of 1000 and of 7 pairs —
on a case whose repeat and far pairs no join of the two single-end lists can pair."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import pair_reference as P  # noqa: E402
import reference_map_reference as M  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = -77            # what an output holds where nobody may write

# ---- the case: the geometry of test_seed_map_gpu.py, 96 pairs of 32 bp ends ----------------------------------------------------
REF_LEN, W, S, N = 3000, 96, 48, 32
MAX_DISTANCE, RESCUE_DISTANCE, INSERT_MIN, INSERT_MAX = 2, 6, 60, 200
COPIES, UNIT = (300, 700, 1100, 1500, 1900, 2300), 40      # one 40 bp segment at six distant loci
KINDS = ("planted", "repeat", "far", "wrong-way", "too-wide", "edge", "unrelated")


def make_case(seed: int = 96):
    """(reference, reads1[96, 32], reads2[96, 32], kinds, planted): planted[c] = ((strand, begin, end) of end 1, of end 2) where
    the pair was taken from the reference, or None for an end that was not."""
    rng = np.random.default_rng(seed)
    ref = ACGT[rng.integers(4, size=REF_LEN)].copy()
    unit = ACGT[rng.integers(4, size=UNIT)]
    for at in COPIES:
        ref[at: at + UNIT] = unit
    ref[[1000, 2222, 2750]] = ord("N")
    reads1, reads2, kinds, planted = [], [], [], []

    def taken(strand, begin, edits=0, substitutions=0):
        """A 32 bp end whose source is ref[begin, begin + 32) on `strand`, with `edits` random edits or exact substitutions."""
        room = min(N + 3, REF_LEN - begin)
        src = _edit(rng, list(ref[begin: begin + room]), edits if room == N + 3 else 0, ACGT)
        read = np.array(src[:N], np.uint8)
        for at in rng.choice(N, size=substitutions, replace=False):
            read[at] = ACGT[(int(np.flatnonzero(ACGT == read[at])[0]) + 1 + int(rng.integers(3))) % 4] if read[at] in ACGT else ACGT[0]
        assert read.size == N
        return M.reverse_complement(read) if strand else read

    def add(kind, first_is_forward, begin, insert, strands=(0, 1), edits=(0, 0), substitutions=0, end2=None):
        """The fragment [begin, begin + insert): its upstream end on strands[0], its downstream end on strands[1]; the forward
        (upstream) end is end 1 when first_is_forward, else end 2.  substitutions and end2 (a replacement) apply to end 2."""
        up, down = (strands[0], begin, begin + N), (strands[1], begin + insert - N, begin + insert)
        one, two = (up, down) if first_is_forward else (down, up)
        reads1.append(taken(one[0], one[1], edits[0]))
        reads2.append(taken(two[0], two[1], edits[1], substitutions) if end2 is None else end2)
        kinds.append(kind)
        planted.append((one, two if end2 is None else None))

    def clear(insert):      # a fragment start away from the copies and the reference's ends
        while True:
            at = int(rng.integers(10, REF_LEN - insert - 10))
            if all(at + insert + 40 < c or at > c + UNIT + 40 for c in COPIES):
                return at

    for i in range(28):
        insert = int(rng.integers(INSERT_MIN + 4, INSERT_MAX - 4))
        add("planted", i % 2 == 0, clear(insert), insert, edits=(i % 3, (i // 3) % 3))
    for i in range(14):     # end 2 inside the fifth or sixth copy, end 1 unique beside it
        copy, offset, insert = COPIES[4 + i % 2], i % 8, 80 + 8 * i
        if i % 4 < 2:       # end 2 is the downstream, reverse end
            add("repeat", True, copy + offset + N - insert, insert)
        else:               # end 2 is the upstream, forward end
            add("repeat", False, copy + offset, insert)
    for i in range(14):
        insert = int(rng.integers(INSERT_MIN + 4, INSERT_MAX - 4))
        add("far", i % 2 == 0, clear(insert), insert, substitutions=4 + i % 3)
    for i in range(10):
        insert = int(rng.integers(INSERT_MIN + 4, INSERT_MAX - 4))
        add("wrong-way", i % 2 == 0, clear(insert), insert, strands=(i % 2, i % 2))
    for i in range(10):
        add("too-wide", i % 2 == 0, clear(400), 400)
    for i in range(8):
        insert = 70 + 15 * i
        add("edge", i % 2 == 0, 0 if i % 4 < 2 else REF_LEN - insert, insert)
    for i in range(12):
        insert = int(rng.integers(INSERT_MIN + 4, INSERT_MAX - 4))
        add("unrelated", i % 2 == 0, clear(insert), insert, end2=ACGT[rng.integers(4, size=N)])
    assert len(kinds) == 96
    return ref, np.stack(reads1), np.stack(reads2), np.array(kinds), planted


def only_through_rescue(host) -> np.ndarray:
    """The pairs that are proper, while the two stage A lists alone, paired by the same rule, are not."""
    alone = P.choose_all(host["single"][0], host["single"][1], INSERT_MIN, INSERT_MAX)
    return (host["proper"] == 1) & (alone["proper"] == 0)


def check_host_model(host, kinds, planted):
    """What the case must show before the GPU is touched."""
    rescued = only_through_rescue(host)
    for kind in ("repeat", "far"):
        assert (rescued & (kinds == kind)).sum() >= 8, (kind, int((rescued & (kinds == kind)).sum()))
    for kind in ("wrong-way", "too-wide", "unrelated"):
        assert not host["proper"][kinds == kind].any(), kind
    assert host["proper"][kinds == "planted"].all() and host["proper"][kinds == "edge"].all()
    for c in np.flatnonzero(rescued & np.isin(kinds, ("repeat", "far"))):      # the chosen slot of end 2 is rescued, at the planted place
        r2 = int(host["slot2"][c])
        assert host["rescued2"][c, r2] and not host["rescued1"][c, int(host["slot1"][c])]
        strand, begin, end = planted[c][1]
        assert host["end2"]["strand"][c, r2] == strand
        if kinds[c] == "repeat":
            assert (host["end2"]["ref_begin"][c, r2], host["end2"]["ref_end"][c, r2]) == (begin, end)
        else:               # substitutions at a read's ends may shift an end by as much
            assert abs(host["end2"]["ref_begin"][c, r2] - begin) <= RESCUE_DISTANCE and abs(host["end2"]["ref_end"][c, r2] - end) <= RESCUE_DISTANCE


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


@pytest.fixture(scope="module")
def case(torch_gpu):
    """The case, the host model of it (asserted before the GPU is touched), a mapper and the results the tests share."""
    ref, reads1, reads2, kinds, planted = make_case()
    assert B.max_stride(W, N, RESCUE_DISTANCE) == 59 >= S
    host = P.map_pairs_host(ref, W, S, reads1, reads2, INSERT_MIN, INSERT_MAX, 1, MAX_DISTANCE, RESCUE_DISTANCE)
    check_host_model(host, kinds, planted)
    mapper = B.ReferenceMapper(ref, W, S)
    got = mapper.map_pairs(reads1, reads2, INSERT_MIN, INSERT_MAX, k_best=1, max_distance=MAX_DISTANCE, rescue_distance=RESCUE_DISTANCE)
    return dict(ref=ref, reads=(reads1, reads2), kinds=kinds, planted=planted, host=host, mapper=mapper, got=got,
                stats=dict(mapper.last_pair_stats))


def assert_same_hits(got, want, what):
    for name in P.FIELDS:
        g, w = getattr(got, name), want[name]
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"{name} differs {what}: {np.argwhere(g != w)[:5].tolist()}"
    assert got.cigars == want["cigars"], f"the cigars differ {what}"


def assert_same_pairs(got, want, what):
    assert_same_hits(got.end1, want["end1"], f"(end 1) {what}")
    assert_same_hits(got.end2, want["end2"], f"(end 2) {what}")
    for name in ("rescued1", "rescued2") + P.OUTPUTS:
        g, w = getattr(got, name), want[name]
        assert g.shape == w.shape and g.dtype == w.dtype and np.array_equal(g, w), f"{name} differs {what}: {np.argwhere(g != w)[:5].tolist()}"


# ---- 1. the rescue-windows kernel -----------------------------------------------------------------------------------------------
def run_rescue(torch, shape, lists, n_pairs, k_anchor, insert_max):
    L = B.lib()
    slots = int(L.bgsa_hip_pair_rescue_slots(*shape, insert_max))
    assert slots == P.rescue_slots(*shape, insert_max) == B.rescue_slots(*shape, insert_max)
    strand, begin, end, keep = (torch.from_numpy(x).cuda() for x in lists)
    out = torch.full((len(lists[0]) + 2, k_anchor * slots), SENT, dtype=torch.int32, device="cuda")
    B.check(L.bgsa_hip_pair_rescue_windows_dev(*shape, strand.data_ptr(), begin.data_ptr(), end.data_ptr(), keep.data_ptr(), n_pairs,
                                               lists[0].shape[1], k_anchor, insert_max, out.data_ptr(), None), "pair_rescue_windows_dev")
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("shape,insert_max", [((3000, 96, 48), 200), ((500, 64, 40), 150), ((200, 64, 64), 1000), ((333, 50, 7), 31),
                                              ((64, 64, 1), 10), ((90, 20, 1), 15)])
def test_rescue_windows_equal_the_helper(torch_gpu, shape, insert_max):
    rng = np.random.default_rng(shape[0])
    ref_len, n_pairs, k = shape[0], 70, 5                       # 70 pairs: 18 workgroups, the last one half empty
    begin = rng.integers(0, ref_len - 20, size=(n_pairs, k)).astype(np.int64)
    end = begin + rng.integers(1, 21, size=(n_pairs, k))
    strand = rng.integers(0, 2, size=(n_pairs, k)).astype(np.int32)
    keep = (rng.random((n_pairs, k)) < 0.6).astype(np.int32)
    keep[3] = 0                                                 # a pair with no anchor
    keep[4] = 1                                                 # more kept slots than k_anchor = 1 and 3 take
    begin[5, :2], end[5, :2], keep[5, :2] = (0, ref_len - 9), (9, ref_len), 1    # clipped at both ends of the reference
    strand[5, :2] = (1, 0)
    strand[6, 0], keep[6, 0] = -1, 1                            # kept slots that are no anchors: a group of -1 each
    begin[7, 0], end[7, 0], keep[7, 0] = -1, -1, 1
    end[8, 0], keep[8, 0] = ref_len + 1, 1
    lists = (strand, begin, end, keep)
    seen = 0
    for k_anchor in (1, 3, 7):                                  # 7: more groups than a list has slots
        got = run_rescue(torch_gpu, shape, lists, n_pairs, k_anchor, insert_max)
        assert (got[n_pairs:] == SENT).all()
        want = P.rescue_table(*shape, *lists, k_anchor, insert_max)
        assert np.array_equal(got[:n_pairs], want), np.argwhere(got[:n_pairs] != want)[:5].tolist()
        assert (got[3] == -1).all() and (got[6, : got.shape[1] // k_anchor] == -1).all()
        seen = max(seen, int((want >= 0).reshape(n_pairs, k_anchor, -1).sum(axis=2).max()))
    assert seen >= min(P.rescue_slots(*shape, insert_max), 2)
    assert (run_rescue(torch_gpu, shape, lists, 0, 3, insert_max) == SENT).all()      # n_pairs = 0: nothing is launched


# ---- 2. the pair-selection kernel -----------------------------------------------------------------------------------------------
def random_lists(rng, n_pairs, k):
    begin = rng.integers(0, 260, size=(n_pairs, k)).astype(np.int64)
    lists = dict(scores=-rng.integers(0, 3, size=(n_pairs, k)).astype(np.int32), strand=rng.integers(0, 2, size=(n_pairs, k)).astype(np.int32),
                 ref_begin=begin, ref_end=begin + rng.integers(28, 37, size=(n_pairs, k)), keep=(rng.random((n_pairs, k)) < 0.7).astype(np.int32))
    gone = lists["keep"] == 0
    unused = gone & (rng.random((n_pairs, k)) < 0.5)           # a slot that is not kept: unused, or unplaced with its strand
    lists["scores"][unused], lists["strand"][unused] = P.INT32_MIN, -1
    lists["ref_begin"][gone], lists["ref_end"][gone] = -1, -1
    lists["windows"] = np.zeros((n_pairs, k), np.int32)
    return lists


def run_select(torch, one, two, n_pairs, insert_min, insert_max):
    names = ("scores", "strand", "ref_begin", "ref_end", "keep")
    d_one, d_two = [torch.from_numpy(one[f]).cuda() for f in names], [torch.from_numpy(two[f]).cuda() for f in names]
    rows = len(one["keep"]) + 3
    out = [torch.full((rows,), SENT, dtype=torch.int64 if name == "insert" else torch.int32, device="cuda") for name in P.OUTPUTS]
    B.check(B.lib().bgsa_hip_pair_select_dev(*(x.data_ptr() for x in d_one), one["keep"].shape[1], *(x.data_ptr() for x in d_two),
                                             two["keep"].shape[1], n_pairs, insert_min, insert_max, *(x.data_ptr() for x in out), None),
            "pair_select_dev")
    torch.cuda.synchronize()
    return {name: x.cpu().numpy() for name, x in zip(P.OUTPUTS, out)}


@pytest.mark.parametrize("k1,k2", [(1, 1), (3, 7), (7, 3), (64, 64), (64, 1)])
def test_select_equals_the_helper(torch_gpu, k1, k2):
    rng = np.random.default_rng(100 * k1 + k2)
    n_pairs = 150                                                # 38 workgroups, the last one half empty
    one, two = random_lists(rng, n_pairs, k1), random_lists(rng, n_pairs, k2)
    one["keep"][:6], two["keep"][3:9] = 0, 0                     # an empty list on end 1, on both ends, on end 2
    got = run_select(torch_gpu, one, two, n_pairs, 60, 200)
    want = P.choose_all(one, two, 60, 200)
    for name in P.OUTPUTS:
        assert (got[name][n_pairs:] == SENT).all(), name
        assert got[name][:n_pairs].dtype == want[name].dtype and np.array_equal(got[name][:n_pairs], want[name]), \
            (name, np.flatnonzero(got[name][:n_pairs] != want[name])[:5].tolist())
    assert (want["slot1"][:6] == -1).all() and (want["slot2"][3:9] == -1).all() and (want["cost"][3:6] == 0).all()
    if k1 * k2 >= 21:
        assert (want["n_best"] > 1).sum() >= 10 and (want["next_cost"] > 0).sum() >= 10 and 10 <= want["proper"].sum() <= n_pairs - 9
    assert all((x == SENT).all() for x in run_select(torch_gpu, one, two, 0, 60, 200).values())      # n_pairs = 0


# ---- 3. map_pairs against the host pipeline -------------------------------------------------------------------------------------
def test_map_pairs_equals_the_host_pipeline(case):
    assert_same_pairs(case["got"], case["host"], "seeded, one block")
    stats, host = case["stats"], case["host"]
    assert stats["k_pair"] == 3 + 8 == case["got"].end1.scores.shape[1] and stats["rescue_slots"] == 8 and stats["pairs"] == 96
    assert stats["slots_rescued"] == host["rescued1"].sum() + host["rescued2"].sum()
    assert stats["proper"] == host["proper"].sum() and stats["proper_through_rescue"] == only_through_rescue(host).sum() >= 16
    anchors = sum(min(int(h["keep"][c].sum()), 1) for h in host["single"] for c in range(96))
    assert stats["anchors"] == anchors and stats["rescue_windows"] >= anchors and stats["pairs_verified"] >= stats["slots_rescued"]
    assert len(stats["seed"]) == 2 and stats["seed"][0]["reads_seeded"] + stats["seed"][0]["reads_fallback_n"] == 96


@pytest.mark.parametrize("seeded,block_rows", [(True, 7), (False, 1000), (False, 7)])
def test_seeding_and_blocks_do_not_change_a_result(case, seeded, block_rows):
    reads1, reads2 = case["reads"]
    got = case["mapper"].map_pairs(reads1, reads2, INSERT_MIN, INSERT_MAX, k_best=1, max_distance=MAX_DISTANCE,
                                   rescue_distance=RESCUE_DISTANCE, seeded=seeded, block_rows=block_rows)
    assert_same_pairs(got, case["host"], f"seeded={seeded}, blocks of {block_rows}")
    stats = case["mapper"].last_pair_stats
    assert (stats["seed"] is None) == (not seeded)
    assert {k: v for k, v in stats.items() if k != "seed"} == {k: v for k, v in case["stats"].items() if k != "seed"}


def test_two_hits_per_end_and_ends_of_two_lengths(case):
    ref, (reads1, reads2) = case["ref"], case["reads"]
    some = np.arange(0, 96, 4)
    short = reads2[some, :27]                                     # end 2 five bases shorter: its own bound, cap and bucket
    want = P.map_pairs_host(ref, W, S, reads1[some], short, INSERT_MIN, INSERT_MAX, 2, MAX_DISTANCE, 4)
    got = case["mapper"].map_pairs(reads1[some], short, INSERT_MIN, INSERT_MAX, k_best=2, max_distance=MAX_DISTANCE, rescue_distance=4,
                                   block_rows=5)
    assert_same_pairs(got, want, "k_best = 2, 32 and 27 bp")
    assert got.end1.scores.shape == (24, 6 + 2 * 8) and case["mapper"].last_pair_stats["k_pair"] == 22


def test_slots_that_are_not_rescued_are_the_single_end_lists(case):
    got, mapper = case["got"], case["mapper"]
    for reads, final, rescued in ((case["reads"][0], got.end1, got.rescued1), (case["reads"][1], got.end2, got.rescued2)):
        alone = mapper.map_reads_seeded(reads, k_best=1, max_distance=MAX_DISTANCE)
        for c in range(96):
            mine = ~rescued[c] & (final.windows[c] >= 0)
            used = alone.windows[c] >= 0
            assert np.array_equal(final.windows[c][mine], alone.windows[c][used]), c
            assert np.array_equal(final.scores[c][mine], alone.scores[c][used]), c
        assert (final.windows[rescued] >= 0).all() and (final.scores[rescued] >= -RESCUE_DISTANCE).all()


def test_no_join_of_the_single_end_lists_pairs_what_map_pairs_pairs(case):
    """What the code lacked: a repeat end whose list is full of lower ids, and an end beyond max_distance, beside a unique mate."""
    got, mapper, kinds, planted = case["got"], case["mapper"], case["kinds"], case["planted"]
    alone = [mapper.map_reads_seeded(reads, k_best=1, max_distance=MAX_DISTANCE) for reads in case["reads"]]
    joined = P.choose_all(*({f: getattr(h, f) for f in P.FIELDS} for h in alone), INSERT_MIN, INSERT_MAX)
    target = np.isin(kinds, ("repeat", "far")) & (joined["proper"] == 0)
    assert (target & (kinds == "repeat")).sum() >= 8 and (target & (kinds == "far")).sum() >= 8
    assert (alone[1].windows[kinds == "far"] == -1).all()             # an end beyond the bound has no single-end hit at all
    pairs = mapper.pairs_of(got)
    for c in np.flatnonzero(target):
        assert got.proper[c] == 1 and got.rescued2[c, got.slot2[c]] and not got.rescued1[c, got.slot1[c]], c
        one, two, proper = pairs[c]
        assert proper and (one.strand, one.ref_begin, one.ref_end) == planted[c][0] and one.distance == 0
        strand, begin, end = planted[c][1]
        assert two.strand == strand and INSERT_MIN <= got.insert[c] <= INSERT_MAX and got.cost[c] == two.distance
        if kinds[c] == "repeat":
            assert (two.ref_begin, two.ref_end, two.distance, two.cigar) == (begin, end, 0, "32=")
        else:
            assert MAX_DISTANCE < two.distance <= RESCUE_DISTANCE and abs(two.ref_begin - begin) <= RESCUE_DISTANCE
    for c in np.flatnonzero(np.isin(kinds, ("wrong-way", "too-wide", "unrelated"))):
        one, two, proper = pairs[c]
        assert not proper and got.n_best[c] == 0 and got.next_cost[c] == -1 and got.insert[c] == 0
        assert one is not None and (two is None) == (kinds[c] == "unrelated")


def test_a_refused_call_leaves_the_mapper_as_it_was(case):
    mapper, (reads1, reads2) = case["mapper"], case["reads"]
    mapper.map_pairs(reads1[:9], reads2[:9], INSERT_MIN, INSERT_MAX, max_distance=MAX_DISTANCE)
    stats, seed_stats, a = dict(mapper.last_pair_stats), mapper.last_seed_stats, mapper.aligner
    bucket = (a.d_peq.data_ptr(), a.ns, a.ns_real, a.wn)
    refused = [dict(reads2=reads2[:8]), dict(insert_min=0), dict(insert_min=201), dict(max_distance=None), dict(rescue_distance=1),
               dict(rescue_distance=18), dict(insert_max=1200, k_best=3), dict(k_best=0), dict(cigar_cap=0), dict(seed_len=14)]
    for over in refused:
        args = dict(reads1=reads1[:9], reads2=reads2[:9], insert_min=INSERT_MIN, insert_max=INSERT_MAX, max_distance=MAX_DISTANCE)
        args.update(over)
        with pytest.raises(B.BgsaHipError, match="rc=-1"):
            mapper.map_pairs(**args)
        assert mapper.last_pair_stats == stats and mapper.last_seed_stats is seed_stats, over
        assert (a.d_peq.data_ptr(), a.ns, a.ns_real, a.wn) == bucket, over
    forward = B.ReferenceMapper(case["ref"], W, S, both_strands=False)
    with pytest.raises(B.BgsaHipError, match="both_strands"):
        forward.map_pairs(reads1[:9], reads2[:9], INSERT_MIN, INSERT_MAX, max_distance=MAX_DISTANCE)
    assert not hasattr(forward.aligner, "d_peq") and forward.last_pair_stats is None

"""Paired reads, without a GPU: the bound R against an enumeration over small geometries, the region's clipping, every refusal of
map_pairs and their order (check_pair_call, and map_pairs on a mapper that has no device), the pairing rule of
tests/pair_reference.py against an independent enumeration, and the three new symbols: declared, exported by both flavours,
prototyped, and refusing bad arguments before any HIP call (fake pointers do)."""
import ctypes
import itertools
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import pair_reference as P  # noqa: E402
from bgsa_amd import reference as RM  # noqa: E402

EINVAL = -1
PTR = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SYMBOLS = ("bgsa_hip_pair_rescue_slots", "bgsa_hip_pair_rescue_windows_dev", "bgsa_hip_pair_select_dev")


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- 1. the bound R -------------------------------------------------------------------------------------------------------------
def rescue_counts(ref_len, W, S, insert_max):
    """For every anchor [b, b + 3) on either strand: how many windows meet its region, and whether they are one id range."""
    starts = B.window_plan(ref_len, W, S)[1]
    counts, contiguous = [], True
    for strand in (0, 1):
        b = np.arange(0, ref_len - 2)
        regions = [P.region(strand, int(x), int(x) + 3, insert_max, ref_len) for x in b]
        lo, hi = np.array([r[0] for r in regions])[:, None], np.array([r[1] for r in regions])[:, None]
        meets = (starts[None, :] < hi) & (starts[None, :] + W > lo)
        counts.append(meets.sum(axis=1))
        edges = np.abs(np.diff(np.pad(meets.astype(np.int8), ((0, 0), (1, 1))), axis=1)).sum(axis=1)
        contiguous &= bool(((edges == 2) | (edges == 0)).all())      # one run of windows, or none
    return np.concatenate(counts), contiguous


def test_the_bound_holds_is_attained_and_the_ranges_are_contiguous(L):
    attained = total = 0
    for ref_len in range(20, 91, 7):
        for W in range(4, 21):
            for S in range(1, W + 1, 2):
                for insert_max in (1, 7, 30, 200):
                    R = B.rescue_slots(ref_len, W, S, insert_max)
                    assert R == P.rescue_slots(ref_len, W, S, insert_max) == L.bgsa_hip_pair_rescue_slots(ref_len, W, S, insert_max)
                    counts, contiguous = rescue_counts(ref_len, W, S, insert_max)
                    assert contiguous and counts.max() <= R, (ref_len, W, S, insert_max, int(counts.max()), R)
                    attained += int(counts.max() == R)
                    total += 1
    assert attained >= total // 2, (attained, total)      # attained wherever the reference is long enough to show it


def test_the_helpers_rescue_windows_are_the_enumeration():
    for ref_len, W, S, insert_max in ((90, 20, 7, 30), (64, 16, 16, 40), (47, 10, 1, 5), (500, 64, 40, 150)):
        n, starts = B.window_plan(ref_len, W, S)
        for strand, b in itertools.product((0, 1), range(0, ref_len - 5, 3)):
            lo, hi = B.rescue_region(strand, b, b + 5, insert_max, ref_len)
            want = [(1 - strand) * n + w for w in range(n) if starts[w] < hi and starts[w] + W > lo]
            assert P.rescue_windows(ref_len, W, S, strand, b, b + 5, insert_max) == want
            assert len(want) <= B.rescue_slots(ref_len, W, S, insert_max) and want == list(range(want[0], want[0] + len(want)))
    table = P.rescue_table(90, 20, 7, np.array([[0, 1, -1]]), np.array([[10, 40, 5]]), np.array([[15, 50, 9]]), np.array([[1, 0, 1]]), 3, 30)
    R = P.rescue_slots(90, 20, 7, 30)
    first = P.rescue_windows(90, 20, 7, 0, 10, 15, 30)
    assert table.shape == (1, 3 * R) and table[0, : len(first)].tolist() == first and (table[0, len(first):] == -1).all()


def test_rescue_slots_and_bad_shapes(L):
    assert B.rescue_slots(3000, 96, 48, 200) == 8 and B.rescue_slots(10_000_000, 400, 239, 600) == 6
    assert B.rescue_slots(200, 64, 64, 1000) == B.window_plan(200, 64, 64)[0] == 4      # never more than there are windows
    for shape in ((1000, 64, 0, 100), (1000, 64, 65, 100), (63, 64, 40, 100), (1000, 64, 40, 0), (1000, 64, 40, 2 ** 31)):
        assert L.bgsa_hip_pair_rescue_slots(*shape) == -1 and L.bgsa_hip_last_error()
    for shape in ((1000, 64, 0, 100), (63, 64, 40, 100), (1000, 64, 40, 0)):
        with pytest.raises(B.BgsaHipError, match="rc=-1"):
            B.rescue_slots(*shape)


# ---- 2. the region --------------------------------------------------------------------------------------------------------------
def test_the_region_is_clipped_at_both_ends_of_the_reference():
    assert B.rescue_region(0, 100, 132, 200, 3000) == (100, 300) == P.region(0, 100, 132, 200, 3000)
    assert B.rescue_region(1, 268, 300, 200, 3000) == (100, 300) == P.region(1, 268, 300, 200, 3000)
    assert B.rescue_region(0, 2900, 2932, 200, 3000) == (2900, 3000)      # clipped at L
    assert B.rescue_region(1, 50, 82, 200, 3000) == (0, 82)               # clipped at 0
    assert B.rescue_region(0, 2968, 3000, 200, 3000) == (2968, 3000) and B.rescue_region(1, 0, 32, 200, 3000) == (0, 32)
    for strand, b in itertools.product((0, 1), (0, 7, 2000, 2968)):
        assert B.rescue_region(strand, b, b + 32, 200, 3000) == P.region(strand, b, b + 32, 200, 3000)


# ---- 3. refusals and their order --------------------------------------------------------------------------------------------------
REFUSALS = {
    "strands": "map_pairs: rc=-1: the mates of a pair lie on opposite strands: the mapper needs both_strands=True",
    "rows": "map_pairs: rc=-1: row c of both arrays is pair c, got 96 and 95 rows",
    "insert": "map_pairs: rc=-1: needs 1 <= insert_min <= insert_max, got 201 and 200",
    "required": "map_pairs: rc=-1: max_distance is required: the single-end lists and the rescue bound are derived from it",
    "rescue": "map_pairs: rc=-1: rescue_distance 1 is below max_distance 2",
    "stride": "map_pairs: rc=-1: at stride 59 a placement of end 2 (33 bp) within rescue_distance 6 can lie in no window of 96 bp: "
              "the largest stride allowed is 58",
    "k_pair": "map_pairs: rc=-1: k_pair = k_sel + k_best * R = 12 + 4 * 14 = 68 slots per end exceed 64: at insert_max 500 the largest "
              "k_best is 3; at k_best 4 the largest insert_max is 481",
    "1024": "map_pairs: rc=-2: reads beyond 1,024 bp have no verify kernel (map_reads takes them)",
    "k_best": "map_pairs: rc=-1: k_best must lie in 1..64",
    "negative": "map_pairs: rc=-1: max_distance is negative",
    "seed_plan": "seed_plan: rc=-1: the 3 pieces of a 32 bp read within distance 2 start 10 bp apart, too close for seeds of 11 bp: "
                 "seed_len 11 allows max_distance <= 1; max_distance 2 allows seed_len <= 10",
    "cigar_cap": "map_pairs: rc=-1: cigar_cap is not positive",
    "max_candidates": "map_pairs: rc=-1: max_candidates is negative",
}
# what breaks each rule, in the order the rules are checked
BREAKS = [("strands", dict(both_strands=False)), ("rows", dict(shape2=(95, 32))), ("insert", dict(insert_min=201)),
          ("required", dict(max_distance=None)), ("rescue", dict(rescue_distance=1)), ("stride", dict(S=59, shape2=(96, 33))),
          ("k_pair", dict(k_best=4, insert_max=500)), ("1024", dict(shape1=(96, 1025), W=1400, S=100)), ("k_best", dict(k_best=0)),
          ("negative", dict(max_distance=-1)), ("seed_plan", dict(seed_len=11)), ("cigar_cap", dict(cigar_cap=0)),
          ("max_candidates", dict(max_candidates=-1))]


def check_pair_call(both_strands=True, shape1=(96, 32), shape2=(96, 32), insert_min=60, insert_max=200, k_best=1, max_distance=2,
                    rescue_distance=6, seeded=True, seed_len=None, max_candidates=None, cigar_cap=None, W=96, S=48, ref_len=3000):
    """check_pair_call as map_pairs calls it on the 3,000 bp case of the GPU tests."""
    n_ids = 2 * B.window_plan(ref_len, W, S)[0]
    return RM.check_pair_call(both_strands, shape1, shape2, insert_min, insert_max, k_best, max_distance, rescue_distance, seeded,
                              seed_len, max_candidates, cigar_cap, W, S, ref_len, n_ids)


def test_every_refusal_has_its_text():
    for rule, over in BREAKS:
        with pytest.raises(B.BgsaHipError) as e:
            check_pair_call(**over)
        assert str(e.value) == REFUSALS[rule], rule
    with pytest.raises(B.BgsaHipError, match="no stride is"):
        check_pair_call(W=37, S=1)
    with pytest.raises(B.BgsaHipError, match="insert_min <= insert_max, got 0 and 200"):
        check_pair_call(insert_min=0)
    with pytest.raises(B.BgsaHipError, match=r"9 \+ 3 \* 28 = 93 .*at insert_max 1200 the largest k_best is 2; at k_best 3 the largest insert_max is 721"):
        check_pair_call(k_best=3, insert_max=1200)
    with pytest.raises(B.BgsaHipError, match=r"3 \+ 1 \* 62 = 65 .*no k_best fits insert_max 3000; at k_best 1 the largest insert_max is 2785"):
        check_pair_call(insert_max=3000)
    with pytest.raises(B.BgsaHipError, match=r"64 \+ 65 \* 8 = 584 .*the largest k_best is 5; no insert_max fits k_best 65"):
        check_pair_call(k_best=65)      # beyond 64 slots before k_best is looked at on its own
    assert check_pair_call(seeded=False, seed_len=11)["k_pair"] == 11      # the exhaustive stage A has no seed plan to refuse


def test_of_two_broken_rules_the_earlier_one_is_reported():
    for i, (first, one) in enumerate(BREAKS):
        for second, two in BREAKS[i + 1:]:
            if set(one) & set(two):
                continue      # both rules are broken through the same argument: one call cannot break both
            over = {**two, **one}
            if (first, second) in (("stride", "1024"), ("insert", "k_pair"), ("rescue", "negative")):
                continue      # the second break mends the first: a longer window, a wider insert_max, a bound below rescue_distance
            with pytest.raises(B.BgsaHipError) as e:
                check_pair_call(**over)
            same = 45 if second == "1024" else None      # the window that holds a 1,025 bp read changes the figures of a text
            assert str(e.value)[:same] == REFUSALS[first][:same], (first, second)


def test_what_an_accepted_call_returns():
    assert check_pair_call() == dict(k_best=1, k_sel=3, rescue_slots=8, k_pair=11, rescue_distance=6, bounds=(6, 6), caps=(128, 128))
    got = check_pair_call(shape2=(96, 5), rescue_distance=None, k_best=2, cigar_cap=9, seeded=False)
    assert got == dict(k_best=2, k_sel=6, rescue_slots=8, k_pair=22, rescue_distance=2, bounds=(2, 2), caps=(9, 9))
    assert check_pair_call(shape2=(96, 5), rescue_distance=9, seeded=False)["bounds"] == (9, 5)      # the bound stops at the read
    assert check_pair_call(k_best=3, insert_max=721)["k_pair"] == 9 + 3 * 18 == 63
    assert check_pair_call(ref_len=10_000_000, W=400, S=239, shape1=(9, 150), shape2=(9, 150), max_distance=6, rescue_distance=12,
                           insert_min=200, insert_max=600)["k_pair"] == 3 + 6


def test_map_pairs_refuses_before_it_touches_a_device():
    mapper = object.__new__(B.ReferenceMapper)      # no aligner, no reference on a device: touching either raises AttributeError
    mapper.ref_len, mapper.window_len, mapper.stride, mapper.both_strands = 3000, 96, 48, True
    mapper.n_windows = B.window_plan(3000, 96, 48)[0]
    mapper.n_ids, mapper.last_pair_stats, mapper.last_seed_stats = 2 * mapper.n_windows, None, None
    reads = np.full((4, 32), ord("A"), np.uint8)
    for over, text in ((dict(reads2=reads[:3]), "row c of both"), (dict(insert_min=0), "insert_min"), (dict(max_distance=None), "required"),
                       (dict(rescue_distance=1), "below max_distance"), (dict(rescue_distance=18), "largest stride allowed is 47"),
                       (dict(k_best=3, insert_max=1200), "exceed 64"), (dict(k_best=0), "k_best must lie"), (dict(cigar_cap=0), "cigar_cap"),
                       (dict(seed_len=14), "seed_len must lie"), (dict(reads1=reads[0]), "reads must be")):
        args = dict(reads1=reads, reads2=reads, insert_min=60, insert_max=200, max_distance=2)
        args.update(over)
        with pytest.raises(B.BgsaHipError, match=text):
            mapper.map_pairs(**args)
        assert mapper.last_pair_stats is None and mapper.last_seed_stats is None
    mapper.both_strands = False
    with pytest.raises(B.BgsaHipError, match="both_strands=True"):
        mapper.map_pairs(reads, reads, 60, 200, max_distance=2)


# ---- 4. the pairing rule ----------------------------------------------------------------------------------------------------------
def enumerate_pair(one, two, insert_min, insert_max):
    """The seven outputs by listing every combination of slot indices as a tuple and sorting: no early exit, no running best."""
    def taking_part(end):
        return [r for r in range(len(end["keep"])) if end["keep"][r] != 0 and end["strand"][r] in (0, 1) and end["ref_begin"][r] >= 0
                and 0 <= -int(end["scores"][r]) < 2 ** 30]
    rows1, rows2 = taking_part(one), taking_part(two)
    found = []
    for r1, r2 in itertools.product(rows1, rows2):
        hits = {int(one["strand"][r1]): (int(one["ref_begin"][r1]), int(one["ref_end"][r1])),
                int(two["strand"][r2]): (int(two["ref_begin"][r2]), int(two["ref_end"][r2]))}
        if len(hits) != 2:
            continue      # the same strand twice
        (f_begin, f_end), (r_begin, r_end) = hits[0], hits[1]
        if f_begin <= r_begin and f_end <= r_end and insert_min <= r_end - f_begin <= insert_max:
            found.append((-int(one["scores"][r1]) - int(two["scores"][r2]), r1, r2, r_end - f_begin))
    if not found:
        first = [(rows[0], -int(end["scores"][rows[0]])) if rows else (-1, 0) for rows, end in ((rows1, one), (rows2, two))]
        return (0, first[0][0], first[1][0], 0, first[0][1] + first[1][1], 0, -1)
    found.sort()
    costs = sorted({f[0] for f in found})
    return (1, found[0][1], found[0][2], found[0][3], costs[0], sum(f[0] == costs[0] for f in found), costs[1] if len(costs) > 1 else -1)


def random_end(rng, k):
    begin = rng.integers(0, 200, size=k)
    end = dict(scores=-rng.integers(0, 2, size=k), strand=rng.integers(-1, 2, size=k), ref_begin=begin, ref_end=begin + rng.integers(25, 40, size=k),
               keep=(rng.random(k) < 0.7).astype(np.int32), windows=np.zeros(k, np.int32))
    end["ref_begin"] = np.where(rng.random(k) < 0.1, -1, end["ref_begin"])
    return end


def test_the_pairing_rule_equals_an_exhaustive_enumeration():
    rng = np.random.default_rng(7)
    proper = ties = seconds = empty = 0
    for trial in range(1500):
        k1, k2 = (1, 1) if trial % 7 == 0 else (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
        one, two = random_end(rng, k1), random_end(rng, k2)
        if trial % 11 == 0:
            one["keep"][:] = 0
        if trial % 13 == 0:
            two["keep"][:] = 0
        got = P.choose(one, two, 40, 120)
        assert tuple(got[name] for name in P.OUTPUTS) == enumerate_pair(one, two, 40, 120), trial
        proper, ties, seconds = proper + got["proper"], ties + (got["n_best"] > 1), seconds + (got["next_cost"] >= 0)
        empty += got["slot1"] == -1 or got["slot2"] == -1
    assert proper >= 150 and ties >= 40 and seconds >= 40 and empty >= 60


def test_the_pairing_rule_on_hand_made_pairs():
    def end(*slots):      # (strand, begin, end, distance, keep)
        s = np.array(slots)
        return dict(strand=s[:, 0], ref_begin=s[:, 1], ref_end=s[:, 2], scores=-s[:, 3], keep=s[:, 4], windows=np.zeros(len(s), np.int32))
    rule = lambda a, b: tuple(P.choose(a, b, 60, 200)[name] for name in P.OUTPUTS)      # noqa: E731
    assert rule(end((0, 100, 132, 1, 1)), end((1, 168, 200, 2, 1))) == (1, 0, 0, 100, 3, 1, -1)
    assert rule(end((1, 168, 200, 2, 1)), end((0, 100, 132, 1, 1))) == (1, 0, 0, 100, 3, 1, -1)      # either end may be the forward one
    assert rule(end((0, 100, 132, 0, 1)), end((0, 168, 200, 0, 1))) == (0, 0, 0, 0, 0, 0, -1)        # the same strand
    assert rule(end((1, 100, 132, 0, 1)), end((0, 168, 200, 0, 1))) == (0, 0, 0, 0, 0, 0, -1)        # the reverse mate upstream
    assert rule(end((0, 100, 132, 0, 1)), end((1, 100, 159, 0, 1)))[0] == 0                            # an insert of 59
    assert rule(end((0, 100, 132, 0, 1)), end((1, 128, 160, 0, 1)))[:4] == (1, 0, 0, 60)               # the mates may overlap
    assert rule(end((0, 100, 132, 0, 1)), end((1, 269, 301, 0, 1)))[0] == 0                            # an insert of 201
    assert rule(end((0, 100, 140, 0, 1)), end((1, 100, 139, 0, 1)))[0] == 0                            # F.end beyond R.end
    assert rule(end((0, 100, 132, 0, 0), (0, 100, 132, 2, 1)), end((1, 168, 200, 1, 1), (1, 170, 202, 1, 1))) == (1, 1, 0, 100, 3, 2, -1)
    assert rule(end((0, 100, 132, 1, 1), (0, 90, 122, 0, 1)), end((1, 168, 200, 0, 1), (1, 170, 202, 1, 1))) == (1, 1, 0, 110, 0, 1, 1)
    assert rule(end((0, 100, 132, 1, 1), (0, 90, 122, 1, 1)), end((1, 168, 200, 1, 1), (1, 170, 202, 1, 1))) == (1, 0, 0, 100, 2, 4, -1)
    assert rule(end((0, 100, 132, 3, 0), (1, 500, 532, 4, 1)), end((1, 168, 200, 5, 0))) == (0, 1, -1, 0, 4, 0, -1)


# ---- 5. the symbols and the C ABI's refusals ----------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared and hasattr(flavour, name), (path.name, name)
    assert L.bgsa_hip_pair_rescue_slots.restype is ctypes.c_int64 and len(L.bgsa_hip_pair_rescue_slots.argtypes) == 4
    assert len(L.bgsa_hip_pair_rescue_windows_dev.argtypes) == 13 and len(L.bgsa_hip_pair_select_dev.argtypes) == 23
    for name in ("PairedHits", "rescue_slots", "rescue_region"):
        assert hasattr(B, name)
    assert B.PairedHits._fields == ("end1", "end2", "rescued1", "rescued2", "proper", "slot1", "slot2", "insert", "cost", "n_best", "next_cost")
    assert hasattr(B.ReferenceMapper, "map_pairs") and hasattr(B.ReferenceMapper, "pairs_of")


def rescue_dev(L, ref_len=3000, W=96, S=48, lists=(PTR,) * 4, n_pairs=1, k=3, k_anchor=1, insert_max=200, out=PTR):
    return L.bgsa_hip_pair_rescue_windows_dev(ref_len, W, S, *lists, n_pairs, k, k_anchor, insert_max, out, None)


def select_dev(L, one=(PTR,) * 5, k1=3, two=(PTR,) * 5, k2=3, n_pairs=1, insert_min=60, insert_max=200, outs=(PTR,) * 7):
    return L.bgsa_hip_pair_select_dev(*one, k1, *two, k2, n_pairs, insert_min, insert_max, *outs, None)


def test_rescue_windows_call_refusals(L):
    for i in range(4):
        lists = [PTR] * 4
        lists[i] = None
        assert rescue_dev(L, lists=tuple(lists)) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert rescue_dev(L, out=None) == EINVAL
    for ref_len, W, S in ((1000, 64, 0), (1000, 64, 65), (63, 64, 40), (0, 1, 1)):
        assert rescue_dev(L, ref_len=ref_len, W=W, S=S) == EINVAL
    assert rescue_dev(L, ref_len=2 ** 30 + 10, W=1, S=1) == EINVAL and b"int32" in L.bgsa_hip_last_error()
    for k in (0, -1, 65):
        assert rescue_dev(L, k=k) == EINVAL and rescue_dev(L, k_anchor=k) == EINVAL
    for insert_max in (0, -5, 2 ** 31):
        assert rescue_dev(L, insert_max=insert_max) == EINVAL
    assert rescue_dev(L, n_pairs=-1) == EINVAL
    assert rescue_dev(L, n_pairs=0) == 0 and rescue_dev(L, n_pairs=0, k=64, k_anchor=64) == 0      # nothing to do: nothing is launched


def test_select_call_refusals(L):
    for side in ("one", "two"):
        for i in range(5):
            lists = [PTR] * 5
            lists[i] = None
            assert select_dev(L, **{side: tuple(lists)}) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    for i in range(7):
        outs = [PTR] * 7
        outs[i] = None
        assert select_dev(L, outs=tuple(outs)) == EINVAL
    for k in (0, -1, 65):
        assert select_dev(L, k1=k) == EINVAL and select_dev(L, k2=k) == EINVAL and b"1..64" in L.bgsa_hip_last_error()
    for insert_min, insert_max in ((0, 200), (201, 200), (1, 2 ** 31), (-3, -2)):
        assert select_dev(L, insert_min=insert_min, insert_max=insert_max) == EINVAL
    assert select_dev(L, n_pairs=-1) == EINVAL
    assert select_dev(L, n_pairs=0) == 0 and select_dev(L, n_pairs=0, k1=64, k2=1, insert_min=1, insert_max=1) == 0

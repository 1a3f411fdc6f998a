"""Duplicate marking without a GPU: the properties of the host model tests/markdup_reference.py on about 2,000 synthetic records and
pairs with planted groups, duplicates_of_sam against duplicates on the same records rendered as SAM lines, the worked example of
INTEGRATION.md §3t, the library's exports and the refusals of the two C calls and of the entry points."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import markdup_reference as MD  # noqa: E402
import sam_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
REF_LEN = 20_000
ACGT = np.frombuffer(b"ACGT", np.uint8)


def rec(rng, strand: int, begin: int = -1, length: int = 30, span=None) -> dict:
    """A record of `length` read bases on [begin, begin + span): span below the read is an insertion, above it a deletion."""
    span = length if span is None else span
    return dict(strand=strand, begin=begin if strand >= 0 else -1, end=begin + span if strand >= 0 else -1, read=bytes(ACGT[rng.integers(4, size=length)]))


def qual(rng, length: int) -> bytes:
    return bytes(rng.integers(33, 75, size=length, dtype=np.uint8))


def planted_singles(rng) -> tuple:
    """(records, quals, {name: indices}) of a single-end batch: random records, then the planted groups."""
    records = [rec(rng, int(rng.integers(-1, 2)), int(rng.integers(0, 2000)), int(rng.choice((1, 2, 30, 64, 65)))) for _ in range(1900)]
    quals = [qual(rng, len(r["read"])) for r in records]
    at = {}

    def plant(name, group, group_quals):
        at[name] = list(range(len(records), len(records) + len(group)))
        records.extend(group)
        quals.extend(group_quals)
    plant("tie", [rec(rng, 0, 10_000) for _ in range(3)], [b"5" * 30] * 3)
    plant("threshold", [rec(rng, 0, 10_100), rec(rng, 0, 10_100)], [b"/" * 29 + b"0", b"/" * 28 + b"00"])      # 15 against 30: only q >= 15 counts
    plant("below", [rec(rng, 0, 10_200), rec(rng, 0, 10_200)], [b"/" * 30, b"!" * 29 + b"0"])                  # 0 against 15: 30 x 14 does not count
    plant("strands", [rec(rng, 0, 10_329), rec(rng, 1, 10_300)], [b"5" * 30] * 2)                              # 5' 10,329 on both strands
    plant("reverse", [rec(rng, 1, 10_400, 30), rec(rng, 1, 10_397, 30, span=33), rec(rng, 1, 10_402, 30, span=28)], [b"5" * 30, b"6" * 30, b"4" * 30])
    plant("forward", [rec(rng, 0, 10_500, 30), rec(rng, 0, 10_500, 30, span=33), rec(rng, 0, 10_500, 64)], [b"5" * 30, b"4" * 30, b"0" * 64])
    return records, quals, at


def planted_pairs(rng) -> tuple:
    """The same for a paired batch: records 2u and 2u + 1 are pair u; at[name] lists PAIR indices."""
    records = []
    for _ in range(950):
        begin, insert = int(rng.integers(0, 3000)), int(rng.integers(60, 90))
        kind = rng.random()
        one, two = rec(rng, 0, begin), rec(rng, 1, begin + insert - 30)
        if kind < 0.1:
            two = rec(rng, -1)
        elif kind < 0.15:
            one, two = rec(rng, -1), rec(rng, -1)
        elif kind < 0.4:
            one, two = two, one
        records += [one, two]
    quals = [qual(rng, len(r["read"])) for r in records]
    at = {}

    def plant(name, pairs, pair_quals):
        at[name] = list(range(len(records) // 2, len(records) // 2 + len(pairs)))
        for (one, two), (q1, q2) in zip(pairs, pair_quals):
            records.extend((one, two))
            quals.extend((q1, q2))

    def fr(begin, insert=200):
        return rec(rng, 0, begin), rec(rng, 1, begin + insert - 30)
    plant("tie", [fr(10_000) for _ in range(3)], [(b"5" * 30, b"5" * 30)] * 3)
    plant("score over both ends", [fr(11_000), fr(11_000)], [(b"9" * 30, b"0" * 30), (b"5" * 30, b"6" * 30)])      # 24 + 15 against 20 + 21
    plant("inner end differs", [fr(12_000, 200), fr(12_000, 190)], [(b"5" * 30, b"5" * 30)] * 2)
    plant("swapped", [fr(13_000), fr(13_000)[::-1]], [(b"5" * 30, b"5" * 30), (b"4" * 30, b"4" * 30)])
    plant("fragment on a pair's end", [fr(14_000), (rec(rng, 0, 14_000), rec(rng, -1)), (rec(rng, -1), rec(rng, 1, 14_170))],
          [(b"!" * 30, b"!" * 30), (b"I" * 30, b"I" * 30), (b"I" * 30, b"I" * 30)])
    plant("fragments alone", [(rec(rng, 0, 15_000), rec(rng, -1)), (rec(rng, -1), rec(rng, 0, 15_000)), (rec(rng, 0, 15_000), rec(rng, -1))],
          [(b"5" * 30, b"I" * 30), (b"I" * 30, b"6" * 30), (b"6" * 30, b"!" * 30)])
    plant("improper", [(rec(rng, 0, 16_000), rec(rng, 0, 18_000)), (rec(rng, 0, 18_000), rec(rng, 0, 16_000))], [(b"5" * 30, b"5" * 30)] * 2)
    return records, quals, at


@pytest.fixture(scope="module")
def singles():
    records, quals, at = planted_singles(np.random.default_rng(42))
    return records, quals, at, MD.duplicates(records, 1, quals)


@pytest.fixture(scope="module")
def pairs():
    records, quals, at = planted_pairs(np.random.default_rng(43))
    return records, quals, at, MD.duplicates(records, 2, quals)


def test_exactly_one_fragment_of_every_key_stays(singles):
    records, quals, _, (flagged, stats) = singles
    groups = {}
    for i, r in enumerate(records):
        if r["strand"] >= 0:
            groups.setdefault((MD.five_prime(r), r["strand"]), []).append(i)
    assert len(records) >= 1900 and sum(len(g) > 1 for g in groups.values()) > 100
    for members in groups.values():
        stays = [i for i in members if i not in flagged]
        assert len(stays) == 1
        scores = [MD.quality_sum(quals[i]) for i in members]
        assert stays[0] == members[scores.index(max(scores))]       # the best, and of equal ones the first
    assert all(records[i]["strand"] >= 0 for i in flagged)
    mapped = sum(r["strand"] >= 0 for r in records)
    assert stats == dict(pair_units=0, fragment_units=mapped, duplicate_pair_units=0, duplicate_fragment_units=mapped - len(groups),
                         records_flagged=mapped - len(groups), records_skipped=0)
    assert MD.duplicates(records, 1, None)[0] == {i for members in groups.values() for i in members[1:]}       # without QUAL: the first stays


def test_the_planted_single_end_groups(singles):
    _, _, at, (flagged, _) = singles
    assert [i in flagged for i in at["tie"]] == [False, True, True]
    assert [i in flagged for i in at["threshold"]] == [True, False]
    assert [i in flagged for i in at["below"]] == [True, False]
    assert [i in flagged for i in at["strands"]] == [False, False]
    assert [i in flagged for i in at["reverse"]] == [True, False, True]         # three begins, one 5' end
    assert [i in flagged for i in at["forward"]] == [True, True, False]         # three ends, one 5' end; 64 x 15 = 960 beats 30 x 20 = 600


def test_the_threshold_alone_decides(singles):
    records, quals, at, _ = singles
    a, b = at["below"]                                                       # 30 x '/' against 29 x '!' and one '0'
    assert MD.quality_sum(b"/") == 0 and MD.quality_sum(b"0") == 15 and MD.quality_sum(b"/0", 14) == 29
    pair, pair_quals = [records[a], records[b]], [quals[a], quals[b]]
    assert MD.duplicates(pair, 1, pair_quals, 15)[0] == {0}                  # 0 against 15
    assert MD.duplicates(pair, 1, pair_quals, 14)[0] == {1}                  # 420 against 15
    assert MD.duplicates(pair, 1, pair_quals, 16)[0] == {1}                  # 0 against 0: the first stays


def test_one_pair_of_every_key_stays_and_pairs_beat_fragments(pairs):
    records, quals, _, (flagged, stats) = pairs
    n_pairs = len(records) // 2
    key_of = lambda i: (MD.five_prime(records[i]), records[i]["strand"])      # noqa: E731
    pair_groups, paired_keys, fragment_groups = {}, set(), {}
    for u in range(n_pairs):
        mapped = [i for i in (2 * u, 2 * u + 1) if records[i]["strand"] >= 0]
        if len(mapped) == 2:
            pair_groups.setdefault(tuple(sorted(map(key_of, mapped))), []).append(u)
            paired_keys.update(map(key_of, mapped))
        elif mapped:
            fragment_groups.setdefault(key_of(mapped[0]), []).append(mapped[0])
    assert sum(len(g) > 1 for g in pair_groups.values()) >= 5
    for units in pair_groups.values():
        stays = [u for u in units if 2 * u not in flagged]
        assert len(stays) == 1 and all((2 * u in flagged) == (2 * u + 1 in flagged) for u in units)
        scores = [MD.quality_sum(quals[2 * u]) + MD.quality_sum(quals[2 * u + 1]) for u in units]
        assert stays[0] == units[scores.index(max(scores))]
    on_a_pair = 0
    for key, members in fragment_groups.items():
        stays = [i for i in members if i not in flagged]
        assert len(stays) == (0 if key in paired_keys else 1)
        on_a_pair += key in paired_keys
    assert on_a_pair >= 3
    assert all(records[i]["strand"] >= 0 for i in flagged)                      # never an unmapped mate
    assert stats["pair_units"] == sum(map(len, pair_groups.values())) and stats["fragment_units"] == sum(map(len, fragment_groups.values()))
    assert stats["duplicate_pair_units"] == stats["pair_units"] - len(pair_groups)
    assert stats["records_flagged"] == 2 * stats["duplicate_pair_units"] + stats["duplicate_fragment_units"] == len(flagged)


def test_the_planted_pair_groups(pairs):
    records, _, at, (flagged, _) = pairs
    marked = lambda name: [(2 * u in flagged, 2 * u + 1 in flagged) for u in at[name]]      # noqa: E731
    assert marked("tie") == [(False, False), (True, True), (True, True)]
    assert marked("score over both ends") == [(True, True), (False, False)]
    assert marked("inner end differs") == [(False, False), (False, False)]
    assert marked("swapped") == [(False, False), (True, True)]
    assert marked("fragment on a pair's end") == [(False, False), (True, False), (False, True)]      # whatever their scores
    assert marked("fragments alone") == [(True, False), (False, False), (True, False)]               # 600, 630, 630: the first 630 stays
    assert marked("improper") == [(False, False), (True, True)]


def render(records, quals, ends: int) -> list:
    """The records as SAM lines (tests/sam_reference.py: line): an insertion or a deletion where the interval is not the read's length."""
    lines = []
    for i, r in enumerate(records):
        mate = records[i ^ 1] if ends == 2 else None
        flag = (4 if r["strand"] < 0 else 16 * r["strand"])
        if mate is not None:
            flag |= 1 | (8 if mate["strand"] < 0 else 32 * mate["strand"]) | (64, 128)[i % 2]
        n, span = len(r["read"]), r["end"] - r["begin"]
        head = min(n, span) // 2
        cigar = "*" if r["strand"] < 0 else f"{n}=" if span == n else f"{head}={abs(span - n)}{'D' if span > n else 'I'}{min(n, span) - head}="
        reverse = r["strand"] == 1
        lines.append(S.line(b"q%d" % (i // ends), flag, b"chr" if r["strand"] >= 0 else b"*", r["begin"] + 1 if r["strand"] >= 0 else 0, 60, cigar,
                            b"*", 0, 0, S.reverse_complement(r["read"]) if reverse else r["read"], quals[i][::-1] if reverse else quals[i]))
    return lines


def test_the_sam_form_agrees_with_the_record_form(singles, pairs):
    for (records, quals, _, want), ends in ((singles, 1), (pairs, 2)):
        lines = render(records, quals, ends)
        assert any(b"D" in x.split(b"\t")[5] for x in lines) or ends == 2
        assert MD.duplicates_of_sam(lines, ends == 2) == want
    assert MD.cigar_reference_length("3=2X4I5D1=") == 11 and MD.cigar_reference_length("*") == 0
    bare = [x.rsplit(b"\t", 1)[0] + b"\t*\n" for x in render(singles[0], singles[1], 1)]      # QUAL '*': every score 0
    assert MD.duplicates_of_sam(bare, False) == MD.duplicates(singles[0], 1, None)


# the worked example of INTEGRATION.md §3t: three pairs and a half-mapped one, 4 bp reads; record = (strand, begin, end, QUAL)
EXAMPLE = [(0, 100, 104, b"5555"), (1, 296, 300, b"5555"), (1, 290, 300, b"I/II"), (0, 100, 104, b"IIII"),
           (0, 100, 104, b"IIII"), (-1, -1, -1, b"IIII"), (0, 100, 104, b"5555"), (1, 280, 284, b"5555")]


def test_the_worked_example_of_the_integration_guide():
    records = [dict(strand=s, begin=b, end=e, read=b"ACGT") for s, b, e, _ in EXAMPLE]
    quals = [q for *_, q in EXAMPLE]
    keys = MD.keys(records, 2, quals)
    assert keys["end_key"] == [400, 1198, 1198, 400, 401, MD.INT64_MAX, 400, 1134]
    assert keys["score"] == [160, 3 * 40 + 160, 160, 160] and keys["pair_key_a"] == [200, 200, MD.INT64_MAX, 200]
    assert keys["pair_key_b"] == [599, 599, MD.INT64_MAX, 567]
    order = sorted(range(4), key=lambda u: (keys["pair_key_a"][u], keys["pair_key_b"][u], -keys["score"][u], u))
    assert order == [3, 1, 0, 2]                             # pair 1 (280) heads the group of key (200, 599): pair 0 behind it is the duplicate
    score = [keys["score"][i // 2] for i in range(8)]
    assert sorted(range(8), key=lambda i: (keys["end_key"][i], -score[i], i)) == [3, 0, 6, 4, 7, 2, 1, 5]
    flagged, stats = MD.duplicates(records, 2, quals)
    assert flagged == {0, 1, 4}
    assert stats == dict(pair_units=3, fragment_units=1, duplicate_pair_units=1, duplicate_fragment_units=1, records_flagged=3, records_skipped=0)
    guide = (ROOT / "INTEGRATION.md").read_text()
    assert "§3t" in guide and "order == [3, 1, 0, 2]" in guide and "[3, 0, 6, 4, 7, 2, 1, 5]" in guide and "flagged == {0, 1, 4}" in guide


def fake_batch() -> B.SamBatch:
    """A batch of pointers that are never read and extents that pass: every call below is refused first or launches nothing."""
    return B.SamBatch(1, None, 30, 2, 1, 1, 2, 2, 1, 1, 1, 1000, 1, 2, 4, *[1] * 14)


def test_the_library_exports_both_calls_and_they_refuse_bad_arguments_before_any_launch():
    L = B.lib()
    assert {"bgsa_hip_dup_keys_dev", "bgsa_hip_dup_mark_dev"} <= set(B.declared_symbols())
    batch = fake_batch()
    ok_keys = dict(batch=batch, n=2, ends=2, min_quality=15, end_key=1, score=1, key_a=1, key_b=1, counts=1, stream=None)
    ok_mark = dict(key_a=1, key_b=1, order=1, n=2, ends=2, flag=1, counts=1, stream=None)

    def keys(**over):
        return L.bgsa_hip_dup_keys_dev(*dict(ok_keys, **over).values())

    def mark(**over):
        return L.bgsa_hip_dup_mark_dev(*dict(ok_mark, **over).values())
    for bad in (dict(batch=None), dict(end_key=None), dict(score=None), dict(key_a=None), dict(key_b=None), dict(counts=None), dict(n=-1),
                dict(ends=0), dict(ends=3), dict(n=3), dict(n=1), dict(min_quality=-1), dict(min_quality=94)):
        assert keys(**bad) == -1 and b"dup_keys_dev" in L.bgsa_hip_last_error(), bad
    unread = fake_batch()
    unread.d_strand = None
    assert keys(batch=unread) == -1 and b"dup_keys_dev" in L.bgsa_hip_last_error()
    for bad in (dict(key_a=None), dict(key_b=None), dict(order=None), dict(flag=None), dict(counts=None), dict(n=-1), dict(ends=0), dict(ends=3),
                dict(n=3)):
        assert mark(**bad) == -1 and b"dup_mark_dev" in L.bgsa_hip_last_error(), bad
    assert mark(key_a=None, ends=1, n=3) == -1 and b"dup_mark_dev" in L.bgsa_hip_last_error()
    assert keys(n=0) == 0 and keys(n=0, ends=1, min_quality=0) == 0 and keys(n=0, min_quality=93) == 0      # nothing to do, nothing launched
    assert mark(n=0) == 0 and mark(n=0, ends=1, key_b=None) == 0


class NoDevice(B.ContigMapper):
    """The entry points of a mapper without a device: a refusal that comes first needs none."""

    def __init__(self):
        self.contig_padding = 10 ** 9


def test_the_entry_points_refuse_a_mark_duplicates_that_is_not_a_bool():
    reads = np.full((2, 30), ord("A"), np.uint8)
    for mapper in (B.ReferenceMapper.__new__(B.ReferenceMapper), NoDevice()):
        for bad in (1, 0, "yes", None):
            for call, who in ((lambda: mapper.map_reads_sam(reads, max_distance=2, mark_duplicates=bad), "map_reads_sam"),
                              (lambda: mapper.map_reads_bam(reads, max_distance=2, sort=True, mark_duplicates=bad), "map_reads_bam"),
                              (lambda: mapper.map_pairs_sam(reads, reads, 50, 100, max_distance=2, mark_duplicates=bad), "map_pairs_sam"),
                              (lambda: mapper.map_pairs_bam(reads, reads, 50, 100, max_distance=2, compress=True, mark_duplicates=bad), "map_pairs_bam")):
                with pytest.raises(B.BgsaHipError, match=f"{who}: rc=-1: mark_duplicates .* is not a bool"):
                    call()
    assert B.check_mark_duplicates("t", True) is True and B.check_mark_duplicates("t", np.bool_(False)) is False
    assert B.DUPLICATE_FLAG == MD.DUPLICATE == 1024 and B.DUPLICATE_MIN_QUALITY == 15 and set(B.DUPLICATE_STATS) == set(MD.STATS)

"""The pileup without a GPU: the two readings of the host model tests/pileup_reference.py against each other on crafted records
rendered as SAM lines, the worked example of INTEGRATION.md §3v with its rows and its one site as literals, sites_of at its edges,
the refusals of check_pileup and of the pileup= / merge= combination, and the C entry points' refusals, which come before any HIP call."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import pileup_reference as P  # noqa: E402
import sam_reference as S  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
ACGT = np.frombuffer(b"ACGT", np.uint8)


def sam_line(rec: dict, qual, reference: bytes, name: bytes = b"q") -> bytes:
    if rec["strand"] < 0:
        return S.line(name, rec["flag"], b"*", 0, 0, "*", b"*", 0, 0, rec["read"], qual)
    return S.crafted_line(rec, name, qual, reference, b"chr", rec["flag"], rec["mapq"])


# ---- 1. the two readings agree ----------------------------------------------------------------------------------------------------------
def test_the_sam_reading_agrees_with_the_record_reading():
    rng = np.random.default_rng(46)
    ref_len = 3000
    reference = bytes(ACGT[rng.integers(4, size=ref_len)])
    shapes = ([(30, "=")], [(2, "I"), (10, "="), (3, "D"), (1, "X"), (7, "="), (4, "I"), (9, "="), (1, "I")], [(5, "I")], [(1, "X")],
              [(70, "="), (6, "D"), (70, "X")], [(3, "="), (1, "I"), (3, "="), (1, "D"), (3, "=")])
    records, quals = [], []
    for i in range(240):
        runs = shapes[i % len(shapes)]
        begin = (0, ref_len - S.consumed(runs)[0])[i % 2] if i < 12 else int(rng.integers(0, ref_len - 160))
        rec = S.craft(rng, reference, begin, runs, reverse=i % 3 == 1)
        rec.update(flag=(0, 1024, 256, 512, 2048, 1)[i % 7 % 6] | (16 if rec["strand"] == 1 else 0), mapq=int(rng.integers(0, 61)))
        if i % 11 == 0:                                       # a read byte that is no upper-case base where the script says '=' or X
            read = bytearray(rec["read"])
            read[len(read) // 2] = (ord("N"), ord("a"), ord("R"))[i % 3]
            rec["read"] = bytes(read)
            rec["forward"] = S.reverse_complement(rec["read"]) if rec["strand"] == 1 else rec["read"]
        records.append(rec)
        qual = bytes(rng.integers(33, 60, size=len(rec["read"]), dtype=np.uint8))
        quals.append(b"+" if qual == b"*" else qual)          # SAM itself cannot tell a one-base QUAL of '*' from no QUAL
    records.append(dict(read=b"ACGTACGT", strand=-1, flag=4, mapq=0, words=np.zeros(0, np.uint32), begin=-1, end=-1))
    quals.append(b"IIIIIIII")
    for with_qual in (True, False):
        given = quals if with_qual else None
        lines = [sam_line(r, given[i] if with_qual else None, reference) for i, r in enumerate(records)]
        for args in (dict(), dict(min_mapq=30), dict(min_base_quality=0), dict(min_base_quality=20, exclude_flags=0), dict(exclude_flags=0xF00)):
            counts, stats = P.pileup_of_batch(records, given, ref_len, **args)
            sam_counts, sam_stats = P.pileup_of_sam(lines, ref_len, **args)
            assert np.array_equal(counts, sam_counts) and stats == sam_stats, (with_qual, args)
            assert stats[0] + stats[1] == len(records) and stats[2] == 0 and counts[:, :5].sum() == stats[3]
            assert (stats[4] > 0) == (with_qual and args.get("min_base_quality", 13) > 0)
            assert (counts[:, 7] <= counts[:, :6].sum(axis=1)).all() and counts[:, 4].sum() > 0 and counts[:, 5].sum() > 0 < counts[:, 6].sum()
    counts, _ = P.pileup_of_batch(records, None, ref_len, exclude_flags=0)
    assert counts[0].sum() > 0 and counts[ref_len - 1].sum() > 0      # ref_begin = 0 and ref_end = ref_len are among them


# ---- 2. the worked example of INTEGRATION.md §3v ------------------------------------------------------------------------------------------
EXAMPLE_REFERENCE = b"ACGTACGTACGTACGTACGT"
# (the read as handed over, strand, ref_begin, SAM CIGAR, QUAL as handed over, flag)
EXAMPLE = [(b"GTACGTAC", 0, 2, "8=", b"IIIIIIII", 0),                     # r0
           (b"ACGTTCGT", 1, 4, "3=1X4=", b"IIIIIIII", 16),                # r1: a reverse hit, written ACGAACGT: A on the T of position 7
           (b"ACGAACAC", 0, 4, "3=1X2=2D2=", b"IIII+III", 0),             # r2: an X base at 7, a low-quality base at 8, a D run over 10 and 11
           (b"TTGTCCACG", 0, 6, "2I2=2I3=", b"IIIIIIIII", 0),             # r3: a leading I run (nowhere), an interior one behind 7
           (b"GTACGTAC", 0, 2, "8=", b"IIIIIIII", 1024),                  # r4: r0's duplicate, excluded by its flag
           (b"CGAA", 0, 5, "2=1X1=", b"IIII", 0)]                         # r5: the third A on 7
EXAMPLE_ROWS = {2: [0, 0, 1, 0, 0, 0, 0, 0], 3: [0, 0, 0, 1, 0, 0, 0, 0], 4: [3, 0, 0, 0, 0, 0, 0, 1], 5: [0, 4, 0, 0, 0, 0, 0, 1],
                6: [0, 0, 5, 0, 0, 0, 0, 1], 7: [3, 0, 0, 2, 0, 0, 1, 1], 8: [4, 0, 0, 0, 0, 0, 0, 1], 9: [0, 4, 0, 0, 0, 0, 0, 1],
                10: [0, 0, 2, 0, 0, 1, 0, 1], 11: [0, 0, 0, 1, 0, 1, 0, 1], 12: [1, 0, 0, 0, 0, 0, 0, 0], 13: [0, 1, 0, 0, 0, 0, 0, 0]}


def example_records() -> tuple:
    records = []
    for read, strand, begin, cigar, _, flag in EXAMPLE:
        runs = [(int(n), op) for n, op in S.re.findall(r"(\d+)([=XDI])", cigar)]
        records.append(dict(read=read, strand=strand, begin=begin, end=begin + S.consumed(runs)[0], flag=flag, mapq=60, runs=runs,
                            words=np.array([n << 4 | S.RUN_CODE[op] for n, op in runs], np.uint32), distance=S.consumed(runs)[2],
                            forward=S.reverse_complement(read) if strand == 1 else read))
    return records, [q for *_, q, _ in EXAMPLE]


def test_the_worked_example_of_the_integration_guide():
    records, quals = example_records()
    counts, stats = P.pileup_of_batch(records, quals, len(EXAMPLE_REFERENCE))
    want = np.zeros((20, 8), np.int32)
    for p, row in EXAMPLE_ROWS.items():
        want[p] = row
    assert np.array_equal(counts, want)
    assert stats == [5, 1, 0, 32, 1]
    lines = [sam_line(r, quals[i], EXAMPLE_REFERENCE) for i, r in enumerate(records)]
    assert lines[1].split(b"\t")[9] == b"ACGAACGT" and lines[2].split(b"\t")[5] == b"3=1X2=2D2="
    sam_counts, sam_stats = P.pileup_of_sam(lines, 20)
    assert np.array_equal(sam_counts, want) and sam_stats == stats
    codes = np.array([b"ACGT".index(c) for c in EXAMPLE_REFERENCE], np.uint8)
    sites = P.sites_of(counts, codes, min_cover=4, min_alt=3, min_percent=50)
    assert {k: v.tolist() for k, v in sites.items()} == dict(pos=[7], ref=[3], alt=[0], alt_count=[3], cover=[5], alts_mask=[1])
    with_duplicate, _ = P.pileup_of_batch(records, quals, 20, exclude_flags=0x304)      # flag 1024 honoured or not: r4 is r0 again
    assert with_duplicate[7].tolist() == [3, 0, 0, 3, 0, 0, 1, 1]
    guide = (ROOT / "INTEGRATION.md").read_text()
    assert "§3v" in guide and "stats == [5, 1, 0, 32, 1]" in guide and "pos=[7], ref=[3], alt=[0], alt_count=[3], cover=[5], alts_mask=[1]" in guide
    for p, row in EXAMPLE_ROWS.items():
        assert f"{p}: {row}" in guide, p


# ---- 3. the site test at its edges -----------------------------------------------------------------------------------------------------------
def site_edges() -> tuple:
    """(counts, reference codes, {position: what it shows}): min_cover 8, min_alt 3, min_percent 20."""
    rows = {0: ([10, 2, 0, 0, 0, 0, 0, 0], 0, "a count at min_alt - 1"),
            1: ([10, 3, 0, 0, 0, 0, 0, 0], 0, "a count at min_alt"),
            2: ([16, 0, 4, 0, 0, 0, 0, 0], 0, "100 * 4 == 20 * 20 exactly"),
            3: ([17, 0, 4, 0, 0, 0, 0, 0], 0, "one below: 400 < 420"),
            4: ([2, 5, 0, 5, 0, 0, 0, 7], 0, "a tie between C and T: the lowest column"),
            5: ([0, 9, 9, 0, 0, 0, 0, 0], 4, "a reference N"),
            6: ([6, 0, 0, 0, 0, 5, 0, 0], 0, "D as alt"),
            7: ([9, 0, 0, 0, 0, 0, 4, 0], 0, "I as alt: column 6 is no part of the cover"),
            8: ([4, 3, 0, 0, 0, 0, 0, 0], 0, "cover at min_cover - 1"),
            9: ([4, 3, 0, 0, 1, 0, 0, 0], 0, "column 4 is cover and no allele"),
            10: ([0, 0, 0, 0, 9, 0, 0, 0], 1, "only other bytes"),
            11: ([3, 0, 0, 8, 0, 0, 0, 0], 3, "the reference's own column never qualifies: A does"),
            12: ([0, 0, 0, 0, 0, 0, 0, 0], 2, "nothing")}
    counts = np.array([row for row, _, _ in rows.values()], np.int32)
    return counts, np.array([r for _, r, _ in rows.values()], np.uint8), {p: why for p, (_, _, why) in rows.items()}


def test_sites_of_at_its_edges():
    counts, codes, why = site_edges()
    got = P.sites_of(counts, codes)
    sites = {int(p): (int(r), int(a), int(n), int(c), int(m)) for p, r, a, n, c, m in
             zip(got["pos"], got["ref"], got["alt"], got["alt_count"], got["cover"], got["alts_mask"])}
    assert sites == {1: (0, 1, 3, 13, 0b10), 2: (0, 2, 4, 20, 0b100), 4: (0, 1, 5, 12, 0b1010), 6: (0, 5, 5, 11, 0b100000), 7: (0, 6, 4, 9, 0b1000000),
                     9: (0, 1, 3, 8, 0b10), 11: (3, 0, 3, 11, 0b1)}, why
    fast = P.sites_of_fast(counts, codes)
    assert all(np.array_equal(fast[k], got[k]) and fast[k].dtype == got[k].dtype for k in got)
    assert P.sites_of(counts, codes, min_cover=1, min_alt=1, min_percent=0)["pos"].tolist() == [0, 1, 2, 3, 4, 6, 7, 8, 9, 11]
    assert P.sites_of(counts, codes, min_percent=100)["pos"].tolist() == []


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------------
def test_check_pileup_refuses_what_is_out_of_range():
    assert B.check_pileup("t") == (0, 13, 0x704) == (0, 13, B.PILEUP_EXCLUDE_FLAGS) and B.check_pileup("t", 255, 93, 65535) == (255, 93, 65535)
    assert B.check_pileup("t", np.int32(7), 0, 0) == (7, 0, 0)
    for bad in (dict(min_mapq=-1), dict(min_mapq=256), dict(min_mapq=1.0), dict(min_mapq=True), dict(min_mapq=None), dict(min_base_quality=-1),
                dict(min_base_quality=94), dict(min_base_quality="13"), dict(exclude_flags=-1), dict(exclude_flags=65536), dict(exclude_flags=None)):
        name = next(iter(bad))
        with pytest.raises(B.BgsaHipError, match=f"t: rc=-1: {name} .* is not an int in 0\\.\\."):
            B.check_pileup("t", **bad)
    assert B.check_pileup_sites("t") == (8, 3, 20) and B.check_pileup_sites("t", 1, 1, 0) == (1, 1, 0) and B.check_pileup_sites("t", 9, 9, 100) == (9, 9, 100)
    for bad in (dict(min_cover=0), dict(min_cover=2 ** 31), dict(min_alt=0), dict(min_alt=1.5), dict(min_percent=-1), dict(min_percent=101),
                dict(min_percent=None)):
        with pytest.raises(B.BgsaHipError, match=f"t: rc=-1: {next(iter(bad))} .* is not an int in"):
            B.check_pileup_sites("t", **bad)
    assert B.PILEUP_STATS == P.STATS and len(B.PILEUP_COLUMNS) == P.COLUMNS == 8
    with pytest.raises(B.BgsaHipError, match="pileup: rc=-1: min_mapq 300"):      # before anything is allocated: this mapper has no device
        B.ReferenceMapper.__new__(B.ReferenceMapper).pileup(min_mapq=300)


class NoDevice(B.ContigMapper):
    """The entry points of a mapper without a device: a refusal that comes first needs none."""

    def __init__(self):
        self.contig_padding = 10 ** 9


def made(kind, **fields):
    x = kind.__new__(kind)
    for key, value in fields.items():
        setattr(x, key, value)
    return x


def test_the_entry_points_refuse_a_pileup_that_cannot_be_honoured():
    reads = np.full((2, 30), ord("A"), np.uint8)
    for mapper in (B.ReferenceMapper.__new__(B.ReferenceMapper), NoDevice()):
        other = made(B.Pileup, mapper=B.ReferenceMapper.__new__(B.ReferenceMapper))
        own = made(B.Pileup, mapper=mapper)
        marking = {ends: made(B.BamMerge, mapper=mapper, finished=False, ends=ends, mark_duplicates=True) for ends in (1, 2)}

        def calls(pileup, merge=None):
            extra = {} if merge is None else dict(merge=merge)
            out = [(lambda: mapper.map_reads_bam(reads, max_distance=2, pileup=pileup, **({} if merge is None else dict(merge=merge[1]))), "map_reads_bam"),
                   (lambda: mapper.map_pairs_bam(reads, reads, 50, 100, max_distance=2, pileup=pileup, **({} if merge is None else dict(merge=merge[2]))),
                    "map_pairs_bam")]
            if not extra:
                out += [(lambda: mapper.map_reads_sam(reads, max_distance=2, pileup=pileup), "map_reads_sam"),
                        (lambda: mapper.map_pairs_sam(reads, reads, 50, 100, max_distance=2, pileup=pileup), "map_pairs_sam")]
            return out
        for bad in (1, "pileup", {}, marking[1]):
            for call, who in calls(bad):
                with pytest.raises(B.BgsaHipError, match=f"{who}: rc=-1: pileup .* is not a Pileup"):
                    call()
        for call, who in calls(other):
            with pytest.raises(B.BgsaHipError, match=f"{who}: rc=-1: the pileup belongs to another mapper"):
                call()
        for call, who in calls(own, marking):
            with pytest.raises(B.BgsaHipError, match=f"{who}: rc=-1: pileup= beside a merge with mark_duplicates=True"):
                call()
        with pytest.raises(B.BgsaHipError, match="crafted: rc=-1: sort=True needs fmt 'bam'"):      # what sam_records refuses already comes first
            B.ReferenceMapper.sam_records(mapper, "crafted", reads, None, None, None, None, {}, None, fmt="sam", sort=True, pileup=own)
        with pytest.raises(B.BgsaHipError, match="crafted: rc=-1: merge= needs fmt 'bam'"):
            B.ReferenceMapper.sam_records(mapper, "crafted", reads, None, None, None, None, {}, None, fmt="sam", merge=marking[1], pileup=own)
        with pytest.raises(B.BgsaHipError, match="crafted: rc=-1: the pileup belongs to another mapper"):
            B.ReferenceMapper.sam_records(mapper, "crafted", reads, None, None, None, None, {}, None, fmt="bam", pileup=other)
    plain = made(B.BamMerge, mapper=None, mark_duplicates=False)
    B.check_pileup_add("t", made(B.Pileup, mapper=None), None, plain)      # a merge that does not mark duplicates is allowed


def fake_batch() -> B.SamBatch:
    """A batch of pointers that are never read and extents that pass: every call below is refused first or launches nothing."""
    return B.SamBatch(1, None, 30, 2, 1, 1, 2, 2, None, 0, 1, 1000, 1, 2, 4, *[1] * 14)


def test_the_library_exports_the_calls_and_they_refuse_bad_arguments_before_any_launch():
    L = B.lib()
    names = {"bgsa_hip_pileup_dev", "bgsa_hip_pileup_site_blocks", "bgsa_hip_pileup_sites_count_dev", "bgsa_hip_pileup_sites_emit_dev"}
    assert names <= set(B.declared_symbols()) and all(hasattr(L, name) for name in names)
    ok = dict(batch=fake_batch(), n=2, min_mapq=0, min_base_quality=13, exclude_flags=0x704, counts=1, stats=1, stream=None)

    def pileup(**over):
        return L.bgsa_hip_pileup_dev(*dict(ok, **over).values())
    for bad in (dict(batch=None), dict(counts=None), dict(stats=None), dict(n=-1), dict(min_mapq=-1), dict(min_mapq=256), dict(min_base_quality=-1),
                dict(min_base_quality=94), dict(exclude_flags=-1), dict(exclude_flags=65536)):
        assert pileup(**bad) == -1 and b"pileup_dev" in L.bgsa_hip_last_error(), bad
    unread = fake_batch()
    unread.d_flag = None
    assert pileup(batch=unread) == -1 and b"pileup_dev" in L.bgsa_hip_last_error()
    assert pileup(n=0) == 0 and pileup(n=0, min_mapq=255, min_base_quality=93, exclude_flags=65535) == 0      # nothing to do, nothing launched
    for ref_len, blocks in ((-5, 0), (0, 0), (1, 1), (255, 1), (256, 1), (257, 2), (140_000, 547), (10_000_000, 39063)):
        assert L.bgsa_hip_pileup_site_blocks(ref_len) == blocks
    ok_count = dict(counts=1, reference=1, ref_len=1000, min_cover=8, min_alt=3, min_percent=20, block_sites=1, n_blocks=4, stream=None)
    ok_emit = dict(counts=1, reference=1, ref_len=1000, min_cover=8, min_alt=3, min_percent=20, block_offsets=1, n_blocks=4, n_sites=5, pos=1, ref=1,
                   alt=1, mask=1, alt_count=1, cover=1, overflow=1, stream=None)
    shared = (dict(counts=None), dict(reference=None), dict(ref_len=0), dict(ref_len=-1), dict(min_cover=0), dict(min_alt=0), dict(min_percent=-1),
              dict(min_percent=101), dict(n_blocks=3), dict(n_blocks=5), dict(n_blocks=0))
    for bad in shared + (dict(block_sites=None),):
        assert L.bgsa_hip_pileup_sites_count_dev(*dict(ok_count, **bad).values()) == -1 and b"pileup_sites_count_dev" in L.bgsa_hip_last_error(), bad
    for bad in shared + (dict(block_offsets=None), dict(n_sites=-1), dict(pos=None), dict(ref=None), dict(alt=None), dict(mask=None),
                         dict(alt_count=None), dict(cover=None), dict(overflow=None)):
        assert L.bgsa_hip_pileup_sites_emit_dev(*dict(ok_emit, **bad).values()) == -1 and b"pileup_sites_emit_dev" in L.bgsa_hip_last_error(), bad

"""The pileup on the MI355X: the counts kernel on crafted batches row for row against tests/pileup_reference.py with sentinels
around counts and stats — every run length across the serial / whole-wave switch, both strands, with and without QUAL, every
filter at its bound, contention, malformed records of every kind —, the two site passes against sites_of on synthetic count
matrices, and the entry points with pileup= against the model's reading of the call's own SAM lines: duplicates excluded, planted
variants found, batches added up, and pileup=None byte for byte the call without the argument."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import contig_reference as C  # noqa: E402
import pileup_reference as P  # noqa: E402
import sam_reference as S  # noqa: E402
import test_bam_gpu as TB  # noqa: E402
import test_markdup_gpu as TM  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402
import test_pileup_cpu as TC  # noqa: E402
from test_bam_gpu import case, crafted, torch_gpu  # noqa: E402,F401  (fixtures)
from test_bam_index_gpu import Fenced  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 63, 64, 65, 1000)      # across the serial / whole-wave switch (kSerialBases = 4) and the wave's stride
BATCH_KEY = dict(strand="strand", ref_begin="begin", ref_end="end", read_len="read_len", read_row="read_row", n_ops="n_ops")


# ---- 1. the counts kernel on crafted batches --------------------------------------------------------------------------------------------
def run_pileup(torch, batch, min_mapq: int = 0, min_base_quality: int = 13, exclude_flags: int = P.EXCLUDE, into=None) -> tuple:
    """The kernel on a batch, counts and stats between sentinels: (counts [ref_len, 8], stats, the two Fenced to add to)."""
    counts, stats = into if into is not None else (Fenced(torch, TB.CRAFT_LEN * 8, torch.int32), Fenced(torch, 5, torch.int64))
    if into is None:
        counts.set(0)
        stats.set(0)
    B.check(B.lib().bgsa_hip_pileup_dev(batch.struct, batch.n, min_mapq, min_base_quality, exclude_flags, counts.ptr, stats.ptr, None), "pileup_dev")
    torch.cuda.synchronize()
    return counts.host().reshape(-1, 8), stats.host().tolist(), (counts, stats)


def assert_rows(got, want, what) -> None:
    if not np.array_equal(got, want):
        p = int(np.flatnonzero((got != want).any(axis=1))[0])
        raise AssertionError((what, "first differing position", p, got[p].tolist(), want[p].tolist()))


def limits_of(records, cap: int = TB.CAP) -> dict:
    return dict(ref_len=TB.CRAFT_LEN, stride=max(len(r["read"]) for r in records), n_rows=len(records), cap=cap)


def own_records(reference: bytes) -> tuple:
    """(records, quals): what crafted's records leave out — every run length of LENGTHS as '=', X, D and I runs on both strands,
    qualities on either side of the bound, every flag bit alone, MAPQ 6 and 7, seventy records on one locus."""
    rng = np.random.default_rng(460)
    records, quals = [], []

    def add(begin, runs, reverse, qual=None, flag=0, mapq=30):
        rec = S.craft(rng, reference, begin, runs, reverse=reverse)
        rec.update(name=b"p%d" % len(records), flag=flag | (16 if reverse else 0), mapq=mapq, rnext=0, pnext=0, tlen=0)
        records.append(rec)
        quals.append(bytes(rng.integers(33 + 10, 33 + 17, size=len(rec["read"]), dtype=np.uint8)) if qual is None else qual(len(rec["read"])))
    for k, n in enumerate(LENGTHS):
        for reverse in (False, True):
            add(10_000 + 4_500 * k + 17 * reverse, [(n, "="), (n, "X"), (n, "D"), (2, "="), (n, "I"), (n, "="), (n, "D"), (1, "X")], reverse)
    add(60_000, [(3, "I"), (40, "="), (2, "I")], False)                                   # I runs at both ends, and nothing else
    add(60_010, [(1, "I"), (5, "X"), (70, "I")], True)
    add(60_100, [(64, "=")], False, qual=lambda n: bytes([33 + 12, 33 + 13] * (n // 2)))      # min_base_quality - 1 and the bound, lane by lane
    add(60_100, [(64, "=")], True, qual=lambda n: bytes([33 + 13] * (n - 1) + [33 + 12]))
    add(60_200, [(3, "="), (2, "D"), (3, "=")], False, qual=lambda n: bytes([33] * n))         # every base low: the D run still counts
    for bit in range(16):
        add(61_000 + 3 * bit, [(20, "=")], bit == 4, flag=1 << bit)                          # bit 4 is the strand: it comes with a reverse record
    add(62_000, [(20, "=")], False, mapq=6)
    add(62_000, [(20, "=")], True, mapq=7)
    for k in range(70):                                                                  # contention: one locus, both strands, a D and an I among them
        add(63_000 + k % 3, [(30, "="), (1, "D"), (2, "I"), (30, "=")] if k % 7 == 0 else [(61, "=")], k % 2 == 1)
    return records, quals


@pytest.fixture(scope="module")
def crafted_pile(torch_gpu, crafted):
    reference, mapper, records = crafted
    own, own_quals = own_records(reference)
    records = [dict(r) for r in records] + own
    quals = TB.quals_of(records[: len(records) - len(own)]) + own_quals
    assert {len(r["runs"]) for r in records} >= {1, 63, 64, 65, 130} and {r["strand"] for r in records} == {-1, 0, 1}
    assert any(r["begin"] == 0 for r in records) and any(r["end"] == TB.CRAFT_LEN for r in records)
    assert any(r["strand"] >= 0 and all(op == "I" for _, op in r["runs"]) for r in records)
    return reference, mapper, records, quals


@pytest.mark.parametrize("with_qual", (False, True))
def test_the_counts_equal_the_model_row_for_row(torch_gpu, crafted_pile, with_qual):
    torch = torch_gpu
    _, mapper, records, quals = crafted_pile
    quals = quals if with_qual else None
    batch = TB.Batch(torch, mapper, records, quals)
    limits = limits_of(records)
    for args in (dict(), dict(min_mapq=7), dict(min_base_quality=0), dict(min_base_quality=14, exclude_flags=0)):
        got, stats, _ = run_pileup(torch, batch, **args)
        want, want_stats = P.pileup_of_batch(records, quals, TB.CRAFT_LEN, limits=limits, **args)
        assert_rows(got, want, (with_qual, args))
        assert stats == want_stats, (with_qual, args, stats, want_stats)
        assert stats[2] == 0 and stats[0] + stats[1] == len(records) and (stats[4] > 0) == (with_qual and args.get("min_base_quality", 13) > 0)
    assert want[:, 4].sum() > 0 and want[:, 5].sum() > 0 and want[:, 6].sum() > 0 and want[0].sum() > 0 and want[TB.CRAFT_LEN - 1].sum() > 0
    assert want[63_000: 63_064, :4].sum(axis=1).max() >= (60 if not with_qual else 20)      # the seventy on one locus


def test_every_filter_at_its_bound(torch_gpu, crafted_pile):
    torch = torch_gpu
    reference, mapper, records, quals = crafted_pile
    small = [(r, q) for r, q in zip(records, quals) if r["strand"] >= 0 and 60_000 <= r["begin"] < 63_000]
    records, quals = [r for r, _ in small], [q for _, q in small]
    batch = TB.Batch(torch, mapper, records, quals)
    limits = limits_of(records)
    assert {r["flag"] & ~16 for r in records} >= {1 << bit for bit in range(16) if bit != 4} and {6, 7} <= {r["mapq"] for r in records}
    used = {}
    for args in [dict(exclude_flags=1 << bit) for bit in range(16)] + [dict(min_mapq=6), dict(min_mapq=7), dict(min_mapq=8), dict(min_mapq=255),
                                                                       dict(min_base_quality=12), dict(min_base_quality=13), dict(min_base_quality=14),
                                                                       dict(min_base_quality=93)]:
        got, stats, _ = run_pileup(torch, batch, **dict(dict(exclude_flags=0), **args))
        want, want_stats = P.pileup_of_batch(records, quals, TB.CRAFT_LEN, limits=limits, **dict(dict(exclude_flags=0), **args))
        assert_rows(got, want, args)
        assert stats == want_stats, (args, stats, want_stats)
        used[tuple(args.items())[0]] = stats
    assert all(used[("exclude_flags", 1 << bit)][1] == (1 if bit != 4 else sum(1 for r in records if r["flag"] & 16)) for bit in range(16))
    assert used[("min_mapq", 6)][1] == 0 and used[("min_mapq", 7)][1] == 1 and used[("min_mapq", 8)][1] == 2
    assert used[("min_base_quality", 12)][4] < used[("min_base_quality", 13)][4] < used[("min_base_quality", 14)][4]      # 12 and 13 are planted
    assert used[("min_base_quality", 93)][3] == 0 and (got[:, :5] == 0).all() and got[:, 5].sum() > 0                        # only D runs and I runs are left


def test_malformed_records_touch_nothing_and_are_counted(torch_gpu, crafted_pile):
    torch = torch_gpu
    _, mapper, all_records, all_quals = crafted_pile
    mapped = [(r, q) for r, q in zip(all_records, all_quals) if r["strand"] >= 0 and len(r["runs"]) >= 2][:30]
    records, quals = [r for r, _ in mapped], [q for _, q in mapped]
    stride = max(len(r["read"]) for r in records)
    over = TM.malformed_overs(records, 1, stride)
    victims = {i for _, i in over}
    short, long_, none, wide = [i for i in range(len(records)) if i not in victims][-4:]
    over.update({("n_ops", short): len(records[short]["runs"]) - 1, ("n_ops", long_): len(records[long_]["runs"]) + 1, ("n_ops", none): 0,
                 ("n_ops", wide): TB.CAP + 1})      # runs that do not add up (a run too few, a zero word too many, none), more runs than a row holds
    assert len(over) == 13
    seen = [dict(r) for r in records]
    for (field, i), value in over.items():
        seen[i][BATCH_KEY[field]] = value
    limits = limits_of(records)
    assert sum(P.malformed(r, i, limits) for i, r in enumerate(seen)) == 13
    got, stats, _ = run_pileup(torch, TB.Batch(torch, mapper, records, quals, over=over), exclude_flags=0)
    want, want_stats = P.pileup_of_batch(seen, quals, TB.CRAFT_LEN, exclude_flags=0, limits=limits)
    assert_rows(got, want, "malformed")
    assert stats == want_stats and stats[2] == 13 and stats[0] == len(records) - 13
    clean = [r for i, r in enumerate(records) if i not in {i for _, i in over}]      # exactly the others' rows: a malformed record left counts untouched
    clean_quals = [q for i, q in enumerate(quals) if i not in {i for _, i in over}]
    assert_rows(got, P.pileup_of_batch(clean, clean_quals, TB.CRAFT_LEN, exclude_flags=0)[0], "the others alone")
    for one in over.items():                                                            # each kind alone: nothing but stats[2]
        if one == (("read_row", one[0][1]), len(records)):                              # in a batch of one row that index is another kind: beyond by more
            one = (one[0], 1)
        got, stats, _ = run_pileup(torch, TB.Batch(torch, mapper, [records[one[0][1]]], [quals[one[0][1]]], over={(one[0][0], 0): one[1]}), exclude_flags=0)
        assert not got.any() and stats == [0, 0, 1, 0, 0], one


def test_two_calls_add_up_and_the_contig_form_gives_the_same_rows(torch_gpu, crafted_pile):
    torch = torch_gpu
    _, mapper, records, quals = crafted_pile
    half = len(records) // 2
    first, second = TB.Batch(torch, mapper, records[:half], quals[:half]), TB.Batch(torch, mapper, records[half:], quals[half:])
    _, _, into = run_pileup(torch, first)
    got, stats, _ = run_pileup(torch, second, into=into)
    want, want_stats = P.pileup_of_batch(records, quals, TB.CRAFT_LEN)
    assert_rows(got, want, "two calls")
    assert stats == want_stats
    inside = [(r, q) for r, q in zip(records, quals) if r["strand"] < 0 or
              any(start <= r["begin"] and r["end"] <= start + n for _, start, n in TB.CONTIGS)]
    contig_records, contig_quals = TB.as_contig_records([r for r, _ in inside]), [q for _, q in inside]
    batch = TB.Batch(torch, mapper, contig_records, contig_quals)
    batch.struct.d_rname, batch.struct.rname_len = None, 0       # the contig form's batch: RNAME comes from the table, the pileup reads neither
    got, stats, _ = run_pileup(torch, batch)
    want, want_stats = P.pileup_of_batch(contig_records, contig_quals, TB.CRAFT_LEN)
    assert_rows(got, want, "the contig form")
    assert stats == want_stats and stats[0] > 40
    assert B.lib().bgsa_hip_pileup_dev(batch.struct, 0, 0, 13, P.EXCLUDE, into[0].ptr, into[1].ptr, None) == 0      # n == 0: nothing launched
    assert B.lib().bgsa_hip_pileup_dev(batch.struct, batch.n, 0, 94, P.EXCLUDE, into[0].ptr, into[1].ptr, None) == -1
    torch.cuda.synchronize()
    assert np.array_equal(into[0].host().reshape(-1, 8), P.pileup_of_batch(records, quals, TB.CRAFT_LEN)[0])


def test_the_driver_adds_only_after_its_last_check(torch_gpu, crafted):
    torch = torch_gpu
    reference, mapper, records = crafted
    quals = TB.quals_of(records)
    batch = TB.Batch(torch, mapper, records, quals)
    fields = {key: value for key, value in batch.dev.items() if key != "runs_row"}
    names, offsets, rows, qual_rows = (batch.keep[i].cpu().numpy() for i in (2, 3, 0, 1))
    rname = np.frombuffer(TB.RNAME, np.uint8)
    pileup = mapper.pileup()
    assert pileup.counts.shape == (TB.CRAFT_LEN, 8) and pileup.stats() == dict.fromkeys(B.PILEUP_STATS, 0)
    far = dict(fields, tlen=fields["tlen"].clone())
    far["tlen"][4] = 2 ** 33
    with pytest.raises(B.BgsaHipError, match="1 malformed records"):
        mapper.sam_records("crafted", rows, qual_rows, names, offsets, rname, far, batch.keep[5], fmt="bam", pileup=pileup)
    assert pileup.stats() == dict.fromkeys(B.PILEUP_STATS, 0) and not bool(pileup.counts.any())
    want, want_stats = P.pileup_of_batch(records, quals, TB.CRAFT_LEN)
    for k, form in enumerate((dict(fmt="sam"), dict(fmt="bam", sort=True, compress=True))):
        mapper.sam_records("crafted", rows, qual_rows, names, offsets, rname, fields, batch.keep[5], pileup=pileup, **form)
        assert np.array_equal(pileup.counts_host(), (k + 1) * want) and list(pileup.stats().values()) == [(k + 1) * x for x in want_stats]
    assert np.array_equal(pileup.depth().cpu().numpy(), 2 * want[:, :6].sum(axis=1)) and np.array_equal(pileup.counts_host(590, 610), 2 * want[590:610])
    pileup.reset()
    assert pileup.stats() == dict.fromkeys(B.PILEUP_STATS, 0) and not bool(pileup.counts.any())


# ---- 2. the site passes on synthetic count matrices ---------------------------------------------------------------------------------------
THRESHOLDS = (8, 3, 20)


def run_sites(torch, counts: np.ndarray, codes: np.ndarray, thresholds=THRESHOLDS, short: int = 0) -> tuple:
    """count -> scan -> emit on a count matrix, every output between sentinels: (the sites as sites_of returns them, the workgroups'
    counts, the overflow).  short: the outputs hold that many entries fewer than there are sites."""
    L = B.lib()
    ref_len = counts.shape[0]
    d_counts, d_codes = torch.from_numpy(np.ascontiguousarray(counts, np.int32)).cuda(), torch.from_numpy(np.ascontiguousarray(codes, np.uint8)).cuda()
    n_blocks = int(L.bgsa_hip_pileup_site_blocks(ref_len))
    block_sites = Fenced(torch, n_blocks, torch.int32)
    B.check(L.bgsa_hip_pileup_sites_count_dev(d_counts.data_ptr(), d_codes.data_ptr(), ref_len, *thresholds, block_sites.ptr, n_blocks, None),
            "pileup_sites_count_dev")
    torch.cuda.synchronize()
    per_block = block_sites.host()
    offsets = torch.from_numpy(np.concatenate(([0], np.cumsum(per_block, dtype=np.int64)[:-1]))).cuda()
    total = int(per_block.sum())
    n = total - short
    kinds = dict(pos=torch.int64, ref=torch.uint8, alt=torch.uint8, alts_mask=torch.uint8, alt_count=torch.int32, cover=torch.int32)
    outs = {key: Fenced(torch, n, kind, fill=0x5A if kind == torch.uint8 else None) for key, kind in kinds.items()}
    overflow = Fenced(torch, 1, torch.int32)
    overflow.set(0)
    B.check(L.bgsa_hip_pileup_sites_emit_dev(d_counts.data_ptr(), d_codes.data_ptr(), ref_len, *thresholds, offsets.data_ptr(), n_blocks, n,
                                             *(outs[key].ptr for key in kinds), overflow.ptr, None), "pileup_sites_emit_dev")
    torch.cuda.synchronize()
    return {key: outs[key].host() for key in kinds}, per_block, int(overflow.host()[0])


def assert_sites(got: dict, want: dict, what, upto=None) -> None:
    for key in want:
        assert np.array_equal(got[key], want[key][:upto]) and got[key].dtype == want[key].dtype, (what, key, got[key][:8], want[key][:8])


def site_matrix(rng, ref_len: int) -> tuple:
    """Random rows — most no site, about a tenth one — with a site forced at 0, 255, 256 and ref_len - 1 and the CPU test's edges laid in."""
    counts = rng.integers(0, 3, size=(ref_len, 8)).astype(np.int32)
    codes = rng.integers(0, 5, size=ref_len).astype(np.uint8)
    counts[np.arange(ref_len), codes % 4] += 9                   # the reference's own base leads
    hot = rng.random(ref_len) < 0.1
    counts[hot, rng.integers(0, 7, size=ref_len)[hot]] += rng.integers(2, 9, size=int(hot.sum())).astype(np.int32)
    edges, edge_codes, _ = TC.site_edges()
    if ref_len >= 400:
        counts[300: 300 + len(edges)], codes[300: 300 + len(edges)] = edges, edge_codes
    for p in (0, 255, 256, ref_len - 1):
        if p < ref_len:
            counts[p], codes[p] = [12, 0, 6, 0, 1, 0, 2, 5], 0
    return counts, codes


@pytest.mark.parametrize("ref_len", (1, 255, 256, 257, 140_000))
def test_the_site_passes_equal_the_model(torch_gpu, ref_len):
    rng = np.random.default_rng(ref_len)
    counts, codes = site_matrix(rng, ref_len)
    want = P.sites_of_fast(counts, codes, *THRESHOLDS)
    assert {0, min(255, ref_len - 1), ref_len - 1} <= set(want["pos"].tolist()) and (ref_len < 257 or 256 in want["pos"])
    got, per_block, overflow = run_sites(torch_gpu, counts, codes)
    assert overflow == 0
    assert per_block.tolist() == np.bincount(want["pos"] // 256, minlength=-(-ref_len // 256)).tolist()
    assert_sites(got, want, ref_len)
    if ref_len >= 400:
        assert set(range(300, 313)) & set(want["pos"].tolist()) == {301, 302, 304, 306, 307, 309, 311}      # the CPU test's edges
    for name, (some, some_codes) in dict(none=(np.zeros_like(counts), codes), every=(np.tile(np.array([9, 0, 0, 4, 0, 0, 0, 0], np.int32), (ref_len, 1)),
                                                                                   np.zeros(ref_len, np.uint8))).items():
        got, per_block, overflow = run_sites(torch_gpu, some, some_codes)
        assert overflow == 0 and got["pos"].tolist() == ([] if name == "none" else list(range(ref_len))), name
        assert name == "none" or ((got["alt"] == 3).all() and (got["alt_count"] == 4).all() and (got["cover"] == 13).all() and (got["alts_mask"] == 8).all())
    other = (1, 1, 0) if ref_len < 1000 else (12, 2, 15)       # other thresholds, the same passes
    assert_sites(run_sites(torch_gpu, counts, codes, other)[0], P.sites_of_fast(counts, codes, *other), (ref_len, other))


def test_an_output_one_too_small_counts_the_overflow_and_writes_no_further(torch_gpu):
    rng = np.random.default_rng(5)
    counts, codes = site_matrix(rng, 1000)
    want = P.sites_of(counts, codes, *THRESHOLDS)
    assert want["pos"].size > 20
    got, _, overflow = run_sites(torch_gpu, counts, codes, short=1)      # host() checks the sentinel behind the last slot
    assert overflow == 1
    assert_sites(got, want, "one short", upto=want["pos"].size - 1)
    got, _, overflow = run_sites(torch_gpu, counts, codes, short=want["pos"].size)
    assert overflow == want["pos"].size and got["pos"].size == 0


# ---- 3. the entry points --------------------------------------------------------------------------------------------------------------------
def model_of_call(sam: B.SamRecords, ref_len: int, pileup, starts=None) -> tuple:
    return P.pileup_of_sam(TM.lines_of(sam), ref_len, pileup.min_mapq, pileup.min_base_quality, pileup.exclude_flags, starts=starts)


def assert_pileup_is(pileup, want: tuple, what) -> None:
    assert_rows(pileup.counts_host(), want[0], what)
    assert list(pileup.stats().values()) == want[1] and tuple(pileup.stats()) == B.PILEUP_STATS, (what, pileup.stats(), want[1])


def test_map_reads_sam_and_bam_count_what_their_sam_lines_say(case):
    mapper = case["mapper"]
    (reads,), names, (quals,), _ = TM.copies(case, False)
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    pileup = mapper.pileup()
    sam = mapper.map_reads_sam(reads, names, quals, TB.RNAME, pileup=pileup, **args)
    want = model_of_call(sam, PM.REF_LEN, pileup)
    assert_pileup_is(pileup, want, "map_reads_sam")
    assert want[1][0] > 60 and want[1][1] >= 4 and want[1][4] > 0
    marked = mapper.map_reads_sam(reads, names, quals, TB.RNAME, mark_duplicates=True, **args)       # the same call made as SAM
    assert int((marked.flag & 1024 != 0).sum()) >= 15
    pileup.reset()
    got = mapper.map_reads_bam(reads, names, quals, TB.RNAME, sort=True, compress=True, mark_duplicates=True, pileup=pileup, **args)
    assert isinstance(got, B.SortedBamRecords) and int((got.flag & 1024 != 0).sum()) == int((marked.flag & 1024 != 0).sum())
    without = model_of_call(marked, PM.REF_LEN, pileup)
    assert_pileup_is(pileup, without, "map_reads_bam, sorted, compressed, duplicates marked")
    assert without[1][1] == want[1][1] + int((marked.flag & 1024 != 0).sum()) and without[0].sum() < want[0].sum()      # the marked duplicates are left out
    keeping = mapper.pileup(min_mapq=3, min_base_quality=20, exclude_flags=0x304)                    # other bounds; duplicates kept
    mapper.map_reads_bam(reads, names, quals, TB.RNAME, mark_duplicates=True, pileup=keeping, **args)
    assert_pileup_is(keeping, model_of_call(marked, PM.REF_LEN, keeping), "other bounds")
    bare = mapper.pileup()
    assert_pileup_is(bare, model_of_call(mapper.map_reads_sam(reads, seeded=False, pileup=bare, **args), PM.REF_LEN, bare), "no QUAL, exhaustive")
    assert bare.stats()["bases_low_quality"] == 0


def test_map_pairs_bam_counts_what_its_sam_lines_say(case):
    mapper = case["mapper"]
    (reads1, reads2), names, (quals1, quals2), _ = TM.copies(case, True)
    args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    ends = (reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME)
    pileup = mapper.pileup()
    mapper.map_pairs_bam(*ends, mark_duplicates=True, pileup=pileup, **args)
    marked = mapper.map_pairs_sam(*ends, mark_duplicates=True, **args)
    want = model_of_call(marked, PM.REF_LEN, pileup)
    assert_pileup_is(pileup, want, "map_pairs_bam")
    assert int((marked.flag & 1024 != 0).sum()) >= 20 and want[1][0] > 80 and want[0][:, 7].sum() > 0
    plain = mapper.pileup()
    assert_pileup_is(plain, model_of_call(mapper.map_pairs_sam(*ends, pileup=plain, **args), PM.REF_LEN, plain), "map_pairs_sam")
    assert plain.counts_host().sum() > want[0].sum()


def test_the_contig_form_counts_in_linear_coordinates_and_reports_local_sites(torch_gpu):
    F = C.FIXTURE
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=C.PAIRS["PADDING"])
    a, b, n = sequences[C.CHR_A], sequences[C.CHR_B], F["N"]
    planted = bytearray(b[40: 40 + n])
    planted[10] = b"CGTA"[b"ACGT".index(planted[10])]             # an SNV at chrB:50 on four reads, both strands
    reads = [b[30: 30 + n], a[30: 30 + n], bytes(planted), S.reverse_complement(bytes(planted)), bytes(planted), S.reverse_complement(bytes(planted)),
             a[50: 50 + n]]
    reads = np.array([list(x) for x in reads], dtype=np.uint8)
    pileup = mapper.pileup(min_base_quality=0)
    sam = mapper.map_reads_sam(reads, pileup=pileup, k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    starts = {name: int(start) for name, start in zip(mapper.contig_names, mapper.contig_starts)}
    assert len(set(starts.values())) >= 3 and not (sam.flag & 4).any()
    assert_pileup_is(pileup, model_of_call(sam, mapper.ref_len, pileup, starts), "contigs")
    sites = pileup.sites(min_cover=4, min_alt=3, min_percent=50)
    assert sites.contig.tolist() == [C.CHR_B] and sites.pos.tolist() == [50] and sites.alt_count.tolist() == [4] and sites.cover.tolist() == [5]
    assert sites.ref.tolist() == [b"ACGT".index(b[50])] and sites.alt.tolist() == [b"ACGT".index(planted[10])] and sites.contig.dtype == np.int32


def planted_variants() -> tuple:
    """(reference, reads, {kind: (linear position, covering reads)}): an SNV, a 2-base deletion and a 2-base insertion, each carried
    by every read over its locus, the locus at least ten bases inside every such read."""
    rng = np.random.default_rng(461)
    ref = bytearray(bytes(TB.ACGT[rng.integers(4, size=3000)]))
    ref[1497:1505], ref[1997:2003] = b"TACGTACA", b"CACTAG"      # no neighbour lets the deletion of 1500..1501 or the insertion behind 1999 slide
    reference = bytes(ref)
    snv = bytes([b"CGTA"[b"ACGT".index(reference[1000])]])
    sample = reference[:1000] + snv + reference[1001:1500] + reference[1502:2000] + b"GG" + reference[2000:]
    loci = dict(snv=1000, deletion=1500, insertion=2000)          # in the sample's coordinates: -2 behind the deletion, +2 behind the insertion
    starts = [at - back for at in (1000, 1498, 1998) for back in (30, 26, 22, 18, 14, 10)] + list(range(100, 900, 37)) + list(range(2200, 2900, 41))
    reads = [sample[s: s + 40] for s in starts]
    reads = [S.reverse_complement(r) if i % 2 else r for i, r in enumerate(reads)]
    return reference, np.array([list(r) for r in reads], dtype=np.uint8), dict(snv=(1000, 6), deletion=(1500, 6), insertion=(1999, 6)), loci


def test_planted_variants_come_back_as_sites(torch_gpu):
    reference, reads, planted, _ = planted_variants()
    mapper = B.ReferenceMapper(reference, 96, 48)
    pileup = mapper.pileup()
    sam = mapper.map_reads_sam(reads, pileup=pileup, k_best=2, max_distance=3)
    assert not (sam.flag & 4).any() and {0, 16} == set(sam.flag.tolist())
    assert_pileup_is(pileup, model_of_call(sam, 3000, pileup), "planted")
    sites = pileup.sites(min_cover=4, min_alt=3, min_percent=20)
    assert sites.contig is None and sites.pos.tolist() == [1000, 1500, 1501, 1999]
    assert sites.alt.tolist() == [b"ACGT".index(reads[0][30:31].tobytes()), 5, 5, 6] and sites.alt_count.tolist() == [6, 6, 6, 6]
    assert sites.cover.tolist() == [6, 6, 6, 6] and sites.ref.tolist() == [b"ACGT".index(reference[p]) for p in (1000, 1500, 1501, 1999)]
    assert sites.alts_mask.tolist() == [1 << a for a in sites.alt.tolist()]
    codes = mapper.d_reference.cpu().numpy()
    want = P.sites_of(pileup.counts_host(), codes, 1, 1, 0)
    got = pileup.sites(1, 1, 0)
    assert all(np.array_equal(getattr(got, key), want[key]) for key in want)
    with pytest.raises(B.BgsaHipError, match="pileup.sites: rc=-1: min_percent 101"):
        pileup.sites(min_percent=101)


def test_three_unequal_batches_add_up_to_one_call(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE, mark_duplicates=False)
    whole, parts = mapper.pileup(), mapper.pileup()
    mapper.map_reads_sam(reads, names, quals, TB.RNAME, pileup=whole, **args)
    n = reads.shape[0]
    for lo, hi in ((0, 7), (7, 7 + n // 2), (7 + n // 2, n)):
        mapper.map_reads_bam(reads[lo:hi], names[lo:hi], quals[lo:hi], TB.RNAME, pileup=parts, **args)
    assert np.array_equal(parts.counts_host(), whole.counts_host()) and parts.stats() == whole.stats() and whole.stats()["records_used"] > 60
    merged, merge = mapper.pileup(), mapper.bam_merge()          # a merge that does not mark duplicates takes a pileup beside it
    for lo, hi in ((0, 7), (7, n)):
        assert mapper.map_reads_bam(reads[lo:hi], names[lo:hi], quals[lo:hi], TB.RNAME, merge=merge, pileup=merged, k_best=2, max_distance=PM.MAX_DISTANCE) == hi - lo
    assert np.array_equal(merged.counts_host(), whole.counts_host()) and merged.stats() == whole.stats()
    with pytest.raises(B.BgsaHipError, match="pileup= beside a merge with mark_duplicates=True"):
        mapper.map_reads_bam(reads, names, quals, TB.RNAME, merge=mapper.bam_merge(mark_duplicates=True), pileup=merged, k_best=2, max_distance=PM.MAX_DISTANCE)
    with pytest.raises(B.BgsaHipError, match="the pileup belongs to another mapper"):
        B.ReferenceMapper(case["ref"], PM.W, PM.S).map_reads_sam(reads, pileup=merged, k_best=2, max_distance=PM.MAX_DISTANCE)
    assert merged.stats() == whole.stats()


def test_pileup_none_is_the_call_without_the_argument(case):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    single, pair = dict(k_best=2, max_distance=PM.MAX_DISTANCE), dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    ends = (reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME)
    calls = [lambda **kw: mapper.map_reads_sam(reads1, names, quals1, TB.RNAME, **single, **kw),
             lambda **kw: mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, block_payload=256, **single, **kw),
             lambda **kw: mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, compress=True, sort=True, mark_duplicates=True, **single, **kw),
             lambda **kw: mapper.map_pairs_sam(*ends, mark_duplicates=True, **pair, **kw),
             lambda **kw: mapper.map_pairs_bam(*ends, sort=True, **pair, **kw)]

    def flat(records):
        return [x for field in records for x in (field if isinstance(field, B.BamIndex) else (field,))]
    pileup = mapper.pileup()
    for call in calls:
        want = call()
        for got in (call(pileup=None), call(pileup=pileup)):      # text, blocks, columns and index: the same bytes, with a pileup beside them too
            assert type(got) is type(want)
            assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(flat(got), flat(want)))
    assert pileup.stats()["records_used"] > 200

"""Duplicate marking on the MI355X: the two kernels on crafted batches — single-end and paired, with and without QUAL — entry for
entry against tests/markdup_reference.py, with sentinels around every output; then the SAM / BAM entry points with
mark_duplicates=True against the model's reading of the unmarked SAM lines, sorted and compressed forms and the contig form
included; and mark_duplicates=False byte for byte the call without the argument."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bam_reference as M  # noqa: E402
import contig_reference as C  # noqa: E402
import markdup_reference as MD  # noqa: E402
import test_bam_gpu as TB  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402
from test_bam_gpu import case, crafted, torch_gpu  # noqa: E402,F401  (fixtures)
from test_bam_index_gpu import GUARD, Fenced  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 63, 64, 65, 128, 129, 1008)      # the wave's strided sum crosses its own width
BATCH_KEY = dict(strand="strand", ref_begin="begin", ref_end="end", read_len="read_len", read_row="read_row")


# ---- 1. the kernels on crafted batches ------------------------------------------------------------------------------------------------
def rec(rng, strand: int, begin: int = -1, length: int = 30, span=None, flag: int = 0) -> dict:
    """A record dict as test_bam_gpu.Batch takes it: `length` read bases on [begin, begin + span) — the runs are not read here."""
    span = length if span is None else span
    mapped = strand >= 0
    return dict(strand=strand, begin=begin if mapped else -1, end=begin + span if mapped else -1, read=bytes(TB.ACGT[rng.integers(4, size=length)]),
                name=b"q", flag=flag | (16 if strand == 1 else 0) | (0 if mapped else 4), mapq=30, rnext=0, pnext=0, tlen=0,
                words=np.array([length << 4 | 7], np.uint32), distance=0)


def single_batch(rng) -> tuple:
    """(records, quals, {name: indices}) of a single-end batch: the groups of the CPU list on reads of every length of LENGTHS."""
    records, quals, at = [], [], {}

    def plant(name, group, group_quals):
        at[name] = list(range(len(records), len(records) + len(group)))
        records.extend(group)
        quals.extend(group_quals)
    for k, n in enumerate(LENGTHS):                            # three copies: the second is the best by its LAST byte alone
        plant(f"length {n}", [rec(rng, k % 2, 1000 * k + 50, n, flag=2048 * (k % 3 == 0)) for _ in range(3)], [b"5" * n, b"5" * (n - 1) + b"I", b"5" * n])
    plant("tie", [rec(rng, 0, 20_000) for _ in range(3)], [b"5" * 30] * 3)
    plant("threshold", [rec(rng, 0, 20_100), rec(rng, 0, 20_100)], [b"/" * 30, b"!" * 29 + b"0"])               # 0 against 15
    plant("strands", [rec(rng, 0, 20_329), rec(rng, 1, 20_300)], [b"5" * 30] * 2)
    plant("reverse", [rec(rng, 1, 20_400), rec(rng, 1, 20_397, span=33), rec(rng, 1, 20_402, span=28)], [b"5" * 30, b"6" * 30, b"4" * 30])
    plant("forward", [rec(rng, 0, 20_500), rec(rng, 0, 20_500, span=33), rec(rng, 0, 20_500, 64)], [b"5" * 30, b"4" * 30, b"0" * 64])
    plant("no reference base", [rec(rng, 1, 20_600, span=0), rec(rng, 0, 20_600, span=0), rec(rng, 1, 20_600, span=0)], [b"5" * 30, b"5" * 30, b"4" * 30])
    plant("unmapped", [rec(rng, -1), rec(rng, -1)], [b"I" * 30] * 2)
    plant("alone", [rec(rng, 0, 20_700), rec(rng, 1, 20_800)], [b"5" * 30] * 2)
    plant("the reference's ends", [rec(rng, 0, 0), rec(rng, 0, 0), rec(rng, 1, TB.CRAFT_LEN - 30), rec(rng, 1, TB.CRAFT_LEN - 40, 40)],
          [b"5" * 30, b"6" * 30, b"5" * 30, b"5" * 40])
    plant("seventy", [rec(rng, 0, 30_000, flag=k % 2 * 512) for k in range(70)], [b"5" * 30] * 41 + [b"6" * 30] + [b"5" * 28 + b"6!"] * 28)
    return records, quals, at


def pair_batch(rng) -> tuple:
    """The same for a paired batch; at[name] lists PAIR indices."""
    records, quals, at = [], [], {}

    def plant(name, pairs, pair_quals):
        at[name] = list(range(len(records) // 2, len(records) // 2 + len(pairs)))
        for (one, two), (q1, q2) in zip(pairs, pair_quals):
            one["flag"], two["flag"] = one["flag"] | 65, two["flag"] | 129
            records.extend((one, two))
            quals.extend((q1, q2))

    def fr(begin, insert=300, n=30, m=30):
        return rec(rng, 0, begin, n), rec(rng, 1, begin + insert - m, m)
    for k, n in enumerate(LENGTHS):                            # end 1 of n bases, end 2 of the next length: the last byte of end 2 decides
        m = LENGTHS[(k + 1) % len(LENGTHS)]
        plant(f"length {n}", [fr(2000 * k + 50, 1100, n, m) for _ in range(3)], [(b"5" * n, b"5" * m), (b"5" * n, b"5" * (m - 1) + b"I"), (b"5" * n, b"5" * m)])
    plant("tie", [fr(20_000) for _ in range(3)], [(b"5" * 30, b"5" * 30)] * 3)
    plant("score over both ends", [fr(21_000), fr(21_000)], [(b"9" * 30, b"0" * 30), (b"5" * 30, b"6" * 30)])
    plant("threshold", [fr(21_500), fr(21_500)], [(b"/" * 30, b"/" * 30), (b"!" * 30, b"!" * 29 + b"0")])
    plant("inner end differs", [fr(22_000, 300), fr(22_000, 290)], [(b"5" * 30, b"5" * 30)] * 2)
    plant("swapped", [fr(23_000), fr(23_000)[::-1]], [(b"5" * 30, b"5" * 30), (b"4" * 30, b"4" * 30)])
    plant("fragment on a pair's end", [fr(24_000), (rec(rng, 0, 24_000), rec(rng, -1)), (rec(rng, -1), rec(rng, 1, 24_270))],
          [(b"!" * 30, b"!" * 30), (b"I" * 30, b"I" * 30), (b"I" * 30, b"I" * 30)])
    plant("fragments alone", [(rec(rng, 0, 25_000), rec(rng, -1)), (rec(rng, -1), rec(rng, 1, 25_100))], [(b"5" * 30, b"I" * 30)] * 2)
    plant("fragments together", [(rec(rng, 0, 25_500), rec(rng, -1)), (rec(rng, -1), rec(rng, 0, 25_500)), (rec(rng, 0, 25_500), rec(rng, -1))],
          [(b"5" * 30, b"I" * 30), (b"I" * 30, b"6" * 30), (b"6" * 30, b"!" * 30)])
    plant("both unmapped", [(rec(rng, -1), rec(rng, -1))], [(b"I" * 30, b"I" * 30)])
    plant("improper", [(rec(rng, 0, 26_000), rec(rng, 0, 28_000)), (rec(rng, 0, 28_000), rec(rng, 0, 26_000))], [(b"5" * 30, b"5" * 30)] * 2)
    plant("strands", [fr(29_000), (rec(rng, 1, 28_971), rec(rng, 0, 29_299))], [(b"5" * 30, b"5" * 30)] * 2)       # the 5' ends of fr, strands exchanged
    plant("seventy", [fr(40_000) for _ in range(70)], [(b"5" * 30, b"5" * 30)] * 41 + [(b"5" * 30, b"6" * 30)] + [(b"5" * 29 + b"6", b"!" * 30)] * 28)
    return records, quals, at


def malformed_overs(records, ends: int, stride: int) -> dict:
    """{(field, record): value}: one malformed record of each kind, each in a unit of its own that marking would otherwise flag or keep."""
    n = len(records)
    victims = iter([ends * u + (u % ends) for u in range(1, 1 + 3 * 9, 3)])      # copies 1 of the first length groups: far from one another
    over = {("strand", next(victims)): 2, ("strand", next(victims)): -2, ("ref_begin", next(victims)): -1}
    i = next(victims)
    over[("ref_end", i)] = records[i]["begin"] - 1
    over[("ref_end", next(victims))] = TB.CRAFT_LEN + 1
    over[("read_len", next(victims))] = -1
    over[("read_len", next(victims))] = stride + 1
    over[("read_row", next(victims))] = -1
    over[("read_row", next(victims))] = n
    assert len(over) == 9 and all(records[i]["strand"] >= 0 for _, i in over)
    return over


def seen_by_the_model(records, over) -> list:
    seen = [dict(r) for r in records]
    for (field, i), value in (over or {}).items():
        seen[i][BATCH_KEY[field]] = value
    return seen


def run_marking(torch, mapper, batch, ends: int) -> dict:
    """keys -> the mapper's stable sorts -> marks (the pair pass, then the end pass) on a batch, every output between sentinels."""
    L = B.lib()
    n, units = batch.n, batch.n // ends
    end_key, score = Fenced(torch, n, torch.int64), Fenced(torch, units, torch.int32)
    key_a, key_b = Fenced(torch, units, torch.int64), Fenced(torch, units, torch.int64)
    counts = Fenced(torch, 6, torch.int32)
    counts.set(0)
    flag = Fenced(torch, n, torch.int32)
    flag.set(batch.dev["flag"])
    B.check(L.bgsa_hip_dup_keys_dev(batch.struct, n, ends, 15, end_key.ptr, score.ptr, key_a.ptr, key_b.ptr, counts.ptr, None), "dup_keys_dev")
    torch.cuda.synchronize()
    out = dict(end_key=end_key.host().tolist(), score=score.host().tolist(), pair_key_a=key_a.host().tolist(), pair_key_b=key_b.host().tolist())
    G = slice(GUARD, GUARD + units)
    if ends == 2 and n:
        order, keys = mapper.duplicate_order(score.whole[G], key_a.whole[G], key_b.whole[G])
        B.check(L.bgsa_hip_dup_mark_dev(keys[0].data_ptr(), keys[1].data_ptr(), order.data_ptr(), n, 2, flag.ptr, counts.ptr + 12, None), "dup_mark_dev")
    if n:
        order, keys = mapper.duplicate_order(score.whole[G].repeat_interleave(ends), end_key.whole[GUARD: GUARD + n])
        B.check(L.bgsa_hip_dup_mark_dev(keys[0].data_ptr(), None, order.data_ptr(), n, 1, flag.ptr, counts.ptr + 12, None), "dup_mark_dev")
    torch.cuda.synchronize()
    out.update(flag=flag.host().tolist(), counts=counts.host().tolist())
    return out


def assert_equals_the_model(got: dict, records, quals, ends: int, stride: int, what) -> set:
    limits = dict(ref_len=TB.CRAFT_LEN, stride=stride, n_rows=len(records))
    want = MD.keys(records, ends, quals, 15, limits)
    for name in ("end_key", "score", "pair_key_a", "pair_key_b"):
        if ends == 1 and name.startswith("pair_key"):
            assert set(got[name]) <= {MD.INT64_MAX}, (what, name)
            continue
        for i, (g, w) in enumerate(zip(got[name], want[name])):
            assert g == w, (what, name, i, g, w)
        assert len(got[name]) == len(want[name]), (what, name)
    flagged, stats = MD.duplicates(records, ends, quals, 15, limits)
    assert got["flag"] == [r["flag"] | (1024 if i in flagged else 0) for i, r in enumerate(records)], what
    assert got["counts"] == [stats[k] for k in ("pair_units", "fragment_units", "records_skipped", "duplicate_pair_units",
                                                "duplicate_fragment_units", "records_flagged")], what
    return flagged


@pytest.mark.parametrize("with_qual", (False, True))
@pytest.mark.parametrize("ends", (1, 2))
def test_keys_scores_flags_and_counters_equal_the_model(torch_gpu, crafted, ends, with_qual):
    torch = torch_gpu
    _, mapper, _ = crafted
    records, quals, at = (single_batch, pair_batch)[ends - 1](np.random.default_rng(50 + ends))
    quals = quals if with_qual else None
    stride = max(LENGTHS)
    assert {len(r["read"]) for r in records} >= set(LENGTHS) and len(records) % ends == 0
    flagged = assert_equals_the_model(run_marking(torch, mapper, TB.Batch(torch, mapper, records, quals), ends), records, quals, ends, stride, (ends, with_qual))
    mark = lambda name: [tuple(i in flagged for i in range(ends * u, ends * u + ends)) for u in at[name]]      # noqa: E731
    yes, no = (True,) * ends, (False,) * ends
    better = [yes, no, yes] if with_qual else [no, yes, yes]
    assert all(mark(f"length {n}") == better for n in LENGTHS) and mark("tie") == [no, yes, yes]
    assert mark("threshold") == ([yes, no] if with_qual else [no, yes]) and mark("strands") == [no, no]
    assert sum(x == no for x in mark("seventy")) == 1 and mark("seventy")[41 if with_qual else 0] == no and len(at["seventy"]) == 70
    if ends == 1:
        assert mark("reverse") == ([yes, no, yes] if with_qual else [no, yes, yes]) and mark("forward") == ([yes, yes, no] if with_qual else [no, yes, yes])
        assert mark("no reference base") == [no, no, yes] and mark("unmapped") == [no, no] and mark("alone") == [no, no]
        assert mark("the reference's ends") == ([yes, no, yes, no] if with_qual else [no, yes, no, yes])      # 40 x 20 beats 30 x 20
    else:
        assert mark("inner end differs") == [no, no] and mark("swapped") == [no, yes] and mark("improper") == [no, yes]
        assert mark("score over both ends") == ([yes, no] if with_qual else [no, yes])
        assert mark("fragment on a pair's end") == [no, (True, False), (False, True)] and mark("fragments alone") == [no, no]
        assert mark("fragments together") == ([(True, False), no, (True, False)] if with_qual else [no, (False, True), (True, False)])
        assert mark("both unmapped") == [no]
    over = malformed_overs(records, ends, stride)
    seen = seen_by_the_model(records, over)
    got = run_marking(torch, mapper, TB.Batch(torch, mapper, records, quals, over=over), ends)
    assert_equals_the_model(got, seen, quals, ends, stride, (ends, with_qual, "malformed"))
    assert got["counts"][2] == 9
    skipped = {ends * (i // ends) + e for _, i in over for e in range(ends)}
    assert all(got["end_key"][i] == MD.INT64_MAX and got["flag"][i] == records[i]["flag"] for i in skipped)
    clean = MD.duplicates(records, ends, quals, 15)[0]
    assert {i for i in range(len(records)) if got["flag"][i] & 1024} - clean <= {i + 2 * ends for i in skipped}      # only the next copy may take its place


def test_the_smallest_batches_and_a_refused_call_writes_nothing(torch_gpu, crafted):
    torch, L = torch_gpu, B.lib()
    _, mapper, _ = crafted
    rng = np.random.default_rng(7)
    one, two = rec(rng, 0, 500), rec(rng, 0, 500)
    quals = [b"5" * 30, b"6" * 30]
    for records, ends in (([one], 1), ([one, two], 2), ([one, two], 1)):
        got = run_marking(torch, mapper, TB.Batch(torch, mapper, records, quals[: len(records)]), ends)
        assert_equals_the_model(got, records, quals[: len(records)], ends, 30, (len(records), ends))
    assert got["flag"] == [1024, 0]
    batch = TB.Batch(torch, mapper, [one, two], quals)
    outs = [Fenced(torch, 2, torch.int64), Fenced(torch, 2, torch.int32), Fenced(torch, 2, torch.int64), Fenced(torch, 2, torch.int64),
            Fenced(torch, 6, torch.int32)]
    flag = Fenced(torch, 2, torch.int32)
    order = torch.tensor([0, 1], dtype=torch.int64, device="cuda")
    same = torch.tensor([400, 400], dtype=torch.int64, device="cuda")
    ptrs = [x.ptr for x in outs]
    assert L.bgsa_hip_dup_keys_dev(batch.struct, 0, 1, 15, *ptrs, None) == 0 and L.bgsa_hip_dup_keys_dev(batch.struct, 0, 2, 15, *ptrs, None) == 0
    assert L.bgsa_hip_dup_mark_dev(same.data_ptr(), same.data_ptr(), order.data_ptr(), 0, 2, flag.ptr, outs[4].ptr, None) == 0
    for bad in (dict(n=-1), dict(ends=0), dict(ends=3), dict(n=1, ends=2), dict(min_quality=-1), dict(min_quality=94), dict(score=None)):
        args = dict(dict(batch=batch.struct, n=2, ends=1, min_quality=15, end_key=ptrs[0], score=ptrs[1], a=ptrs[2], b=ptrs[3], counts=ptrs[4], stream=None), **bad)
        assert L.bgsa_hip_dup_keys_dev(*args.values()) == -1 and b"dup_keys_dev" in L.bgsa_hip_last_error(), bad
    for bad in (dict(n=-1), dict(ends=3), dict(n=1, ends=2), dict(order=None), dict(flag=None), dict(b=None, ends=2)):
        args = dict(dict(a=same.data_ptr(), b=same.data_ptr(), order=order.data_ptr(), n=2, ends=1, flag=flag.ptr, counts=outs[4].ptr, stream=None), **bad)
        assert L.bgsa_hip_dup_mark_dev(*args.values()) == -1 and b"dup_mark_dev" in L.bgsa_hip_last_error(), bad
    torch.cuda.synchronize()
    for x in outs + [flag]:
        assert (x.host() == x.sent).all()                    # n = 0 and every refused call wrote nothing
    keys = torch.tensor([401, 401], dtype=torch.int64, device="cuda")
    flag = Fenced(torch, 2, torch.int32)
    flag.set(0)
    counts = Fenced(torch, 3, torch.int32)
    counts.set(0)
    for beyond in (2, -1, 2 ** 40):                           # a permutation entry outside the entries: skipped, nothing written
        wild = torch.tensor([0, beyond], dtype=torch.int64, device="cuda")
        B.check(L.bgsa_hip_dup_mark_dev(keys.data_ptr(), None, wild.data_ptr(), 2, 1, flag.ptr, counts.ptr, None), "dup_mark_dev")
        B.check(L.bgsa_hip_dup_mark_dev(keys.data_ptr(), keys.data_ptr(), wild.data_ptr(), 4, 2, flag.ptr, counts.ptr, None), "dup_mark_dev")
    torch.cuda.synchronize()
    assert flag.host().tolist() == [0, 0] and counts.host().tolist() == [0, 0, 0]


# ---- 2. the entry points ---------------------------------------------------------------------------------------------------------------
def lines_of(sam: B.SamRecords) -> list:
    text = sam.text.tobytes()
    return [text[sam.offsets[i]: sam.offsets[i + 1]] for i in range(sam.flag.size)]


def with_flags(lines, flagged) -> list:
    out = []
    for i, line in enumerate(lines):
        f = line.split(b"\t")
        if i in flagged:
            f[1] = str(int(f[1]) | 1024).encode()
        out.append(b"\t".join(f))
    return out


def copies(case, paired: bool) -> tuple:
    """The case's reads (or pairs) and, under new names, 21 of them again — three of them pairs whose end 2 maps nowhere —: seven with
    better QUAL, seven with worse, seven with equal."""
    picked = np.concatenate((np.arange(0, 36, 2), [84, 86, 88]))
    ends = case["reads"] if paired else case["reads"][:1]
    reads = [np.concatenate((rows, rows[picked])) for rows in ends]
    names = list(case["names"]) + [case["names"][i] + b"/copy" for i in picked]
    quals = []
    for rows, own in zip(ends, case["quals"]):
        again = [(b"~" * PM.N, b"!" * PM.N, own[i])[k % 3] for k, i in enumerate(picked)]
        quals.append(list(own) + again)
    return reads, names, quals, picked


def assert_marked_like_the_model(marked, plain, paired: bool, stats: dict, what: str) -> set:
    lines = lines_of(plain)
    flagged, want_stats = MD.duplicates_of_sam(lines, paired)
    assert lines_of(marked) == with_flags(lines, flagged), what
    assert np.array_equal(marked.flag, plain.flag | np.where(np.isin(np.arange(plain.flag.size), sorted(flagged)), 1024, 0)) and marked.flag.dtype == plain.flag.dtype
    for name in ("offsets", "pos", "mapq", "nm"):
        want = getattr(plain, name)
        if name == "offsets":                                # "77" -> "1101": two more bytes on a flagged line
            widths = np.array([len(x) for x in with_flags(lines, flagged)])
            want = np.concatenate(([0], np.cumsum(widths)))
        assert np.array_equal(getattr(marked, name), want), (what, name)
    assert stats == want_stats, what
    return flagged


def test_map_reads_with_duplicates_marked(case):
    mapper = case["mapper"]
    (reads,), names, (quals,), picked = copies(case, False)
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    plain = mapper.map_reads_sam(reads, names, quals, TB.RNAME, **args)
    mapper.last_duplicate_stats = None
    marked = mapper.map_reads_sam(reads, names, quals, TB.RNAME, mark_duplicates=True, **args)
    flagged = assert_marked_like_the_model(marked, plain, False, mapper.last_duplicate_stats, "single")
    n = case["reads"][0].shape[0]
    mapped = [(k, i) for k, i in enumerate(picked) if not plain.flag[i] & 4]
    assert len(mapped) >= 15 and len(flagged) >= len(mapped)
    gone = [(int(i) in flagged, n + k in flagged) for k, i in mapped]      # better: the original goes; worse or equal: the copy
    assert all(a != b for a, b in gone) or len({plain.pos[i] for _, i in mapped}) < len(mapped)
    assert sum(a and not b for (a, b), (k, _) in zip(gone, mapped) if k % 3 == 0) >= 4
    assert sum(b and not a for (a, b), (k, _) in zip(gone, mapped) if k % 3 != 0) >= 8
    assert not any(plain.flag[i] & 4 for i in flagged)
    bam = mapper.map_reads_bam(reads, names, quals, TB.RNAME, mark_duplicates=True, **args)
    TB.assert_decodes_to(bam, marked, [TB.RNAME], 65280, "single, stored")
    packed = mapper.map_reads_bam(reads, names, quals, TB.RNAME, compress=True, mark_duplicates=True, **args)
    assert b"".join(M.walk_blocks(packed.blocks.tobytes(), stored=False)) == b"".join(M.walk_blocks(bam.blocks.tobytes()))
    assert all(np.array_equal(a, b) for a, b in zip(packed[1:], bam[1:]))
    assert_sorted_form(mapper.map_reads_bam(reads, names, quals, TB.RNAME, sort=True, mark_duplicates=True, **args), bam,
                       mapper.map_reads_bam(reads, names, quals, TB.RNAME, sort=True, **args), "single, sorted")
    bare = mapper.map_reads_sam(reads, mark_duplicates=True, **args)          # no QUAL: every score 0, the first of a group stays
    assert_marked_like_the_model(bare, mapper.map_reads_sam(reads, **args), False, mapper.last_duplicate_stats, "single, bare")
    assert all(n + k in np.flatnonzero(bare.flag & 1024) for k, _ in mapped)


def assert_sorted_form(got, marked_unsorted, plain_sorted, what: str) -> None:
    """sort=True with marking: the marked unsorted call's records permuted by `order`; order and index those of the unmarked sorted call."""
    assert isinstance(got, B.SortedBamRecords) and np.array_equal(got.order, plain_sorted.order), what
    records = M.split_records(b"".join(M.walk_blocks(got.blocks.tobytes())))
    unsorted = M.split_records(b"".join(M.walk_blocks(marked_unsorted.blocks.tobytes())))
    assert records == [unsorted[i] for i in got.order], what
    assert np.array_equal(got.flag, marked_unsorted.flag[got.order]) and (got.flag & 1024).any(), what
    assert np.array_equal(got.offsets, plain_sorted.offsets) and np.array_equal(got.ref_id, plain_sorted.ref_id), what      # BAM's flag is two bytes either way
    for a, b in zip(got.index, plain_sorted.index):
        assert np.array_equal(a, b), what


def test_map_pairs_with_duplicates_marked(case):
    mapper = case["mapper"]
    (reads1, reads2), names, (quals1, quals2), picked = copies(case, True)
    args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    ends = (reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME)
    plain = mapper.map_pairs_sam(*ends, **args)
    marked = mapper.map_pairs_sam(*ends, mark_duplicates=True, **args)
    stats = mapper.last_duplicate_stats
    flagged = assert_marked_like_the_model(marked, plain, True, stats, "pairs")
    assert stats["pair_units"] >= 20 and stats["duplicate_pair_units"] >= 10 and stats["fragment_units"] >= 2 and stats["duplicate_fragment_units"] >= 1
    n = case["reads"][0].shape[0]
    both = [(k, i) for k, i in enumerate(picked) if not (plain.flag[2 * i] | plain.flag[2 * i + 1]) & 4]
    assert len(both) >= 10
    gone = [({2 * int(i), 2 * int(i) + 1} <= flagged, {2 * (n + k), 2 * (n + k) + 1} <= flagged) for k, i in both]
    assert sum(a and not b for (a, b), (k, _) in zip(gone, both) if k % 3 == 0) >= 3      # better: the original pair goes
    assert sum(b and not a for (a, b), (k, _) in zip(gone, both) if k % 3 != 0) >= 6      # worse or equal: the copy
    assert not any(plain.flag[i] & 4 for i in flagged)        # never an unmapped mate
    bam = mapper.map_pairs_bam(*ends, mark_duplicates=True, **args)
    TB.assert_decodes_to(bam, marked, [TB.RNAME], 65280, "pairs, stored")
    packed = mapper.map_pairs_bam(*ends, compress=True, block_payload=4096, mark_duplicates=True, **args)
    assert b"".join(M.walk_blocks(packed.blocks.tobytes(), stored=False)) == b"".join(M.walk_blocks(bam.blocks.tobytes()))
    assert_sorted_form(mapper.map_pairs_bam(*ends, sort=True, mark_duplicates=True, **args), bam, mapper.map_pairs_bam(*ends, sort=True, **args),
                       "pairs, sorted")


def test_the_contig_form_marks_by_linear_coordinates(torch_gpu):
    F, P = C.FIXTURE, C.PAIRS
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=P["PADDING"])
    a, b, n = sequences[C.CHR_A], sequences[C.CHR_B], F["N"]
    reads = [b[30: 30 + n], a[30: 30 + n], b[30: 30 + n], a[50: 50 + n], M.S.reverse_complement(b[40: 40 + n]), M.S.reverse_complement(b[40: 40 + n])]
    reads = np.array([list(x) for x in reads], dtype=np.uint8)
    quals = [b"5" * n, b"5" * n, b"6" * n, b"5" * n, b"5" * n, b"5" * n]
    args = dict(k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    plain = mapper.map_reads_sam(reads, None, quals, **args)
    marked = mapper.map_reads_sam(reads, None, quals, mark_duplicates=True, **args)
    flagged = assert_marked_like_the_model(marked, plain, False, mapper.last_duplicate_stats, "contigs")
    fields = [C.fields_of(x) for x in lines_of(plain)]
    assert [f["rname"] for f in fields] == [b"chrB", b"chrA", b"chrB", b"chrA", b"chrB", b"chrB"] and [f["pos"] for f in fields[:3]] == [31, 31, 31]
    assert flagged == {0, 5}                                  # chrB:31 twice: the better stays; chrA:31 is another key; the reverse twins tie
    order = list(F["NAMES"])
    TB.assert_decodes_to(mapper.map_reads_bam(reads, None, quals, mark_duplicates=True, **args), marked, order, 65280, "contigs, BAM")
    pairs = C.crafted_pairs(sequences)
    reads1, reads2 = (np.array([list(x[e]) for x in pairs] * 2, dtype=np.uint8) for e in (1, 2))      # every pair twice
    pair_args = dict(k_best=P["K_BEST"], max_distance=F["MAX_DISTANCE"])
    plain = mapper.map_pairs_sam(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], **pair_args)
    marked = mapper.map_pairs_sam(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], mark_duplicates=True, **pair_args)
    flagged = assert_marked_like_the_model(marked, plain, True, mapper.last_duplicate_stats, "contigs, pairs")
    assert flagged == {6, 7, 8, 9, 10}                        # the proper pair, the pair across two contigs, the mapped end of the half-mapped one
    assert mapper.last_duplicate_stats == dict(pair_units=4, fragment_units=2, duplicate_pair_units=2, duplicate_fragment_units=1, records_flagged=5,
                                               records_skipped=0)


# ---- 3. nothing moved ---------------------------------------------------------------------------------------------------------------------
def test_mark_duplicates_false_is_the_call_without_the_argument(case):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    single, pair = dict(k_best=2, max_distance=PM.MAX_DISTANCE), dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    ends = (reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME)
    calls = [lambda **kw: mapper.map_reads_sam(reads1, names, quals1, TB.RNAME, **single, **kw),
             lambda **kw: mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, block_payload=256, **single, **kw),
             lambda **kw: mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, compress=True, sort=True, **single, **kw),
             lambda **kw: mapper.map_pairs_sam(*ends, **pair, **kw),
             lambda **kw: mapper.map_pairs_bam(*ends, compress=True, **pair, **kw),
             lambda **kw: mapper.map_pairs_bam(*ends, sort=True, **pair, **kw)]
    mapper.last_duplicate_stats = "untouched"

    def flat(records):
        return [x for field in records for x in (field if isinstance(field, B.BamIndex) else (field,))]
    for call in calls:
        want, got = call(), call(mark_duplicates=False)
        assert type(got) is type(want)
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(flat(got), flat(want)))
        assert not (got.flag & 1024).any()
    assert mapper.last_duplicate_stats == "untouched"
    with pytest.raises(B.BgsaHipError, match="map_reads_bam: rc=-1: mark_duplicates 1 is not a bool"):
        mapper.map_reads_bam(reads1, names, mark_duplicates=1, **single)

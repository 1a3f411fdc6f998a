"""A reference of several contigs on the GPU: the clip kernel alone against the model on hand-written run lists, the four map_reads
entry points, map_pairs and the two SAM entry points of ContigMapper on the crafted fixture — field by field against the model
(the existing pipeline model on the padded reference, then the model's clip) and against properties that know nothing of the
model: every kept hit inside its contig, its runs consuming its interval and its read, its NM the DP minimum over the contigs —, and
the regression: one contig through ContigMapper is ReferenceMapper on that sequence."""
import re
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import contig_reference as C  # noqa: E402
import sam_reference as S  # noqa: E402

pytestmark = pytest.mark.gpu
F = C.FIXTURE
W, ST, N, MAX_DISTANCE, K_BEST = F["W"], F["S"], F["N"], F["MAX_DISTANCE"], F["K_BEST"]
NAMES = [name.decode() for name in F["NAMES"]]


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


@pytest.fixture(scope="module")
def sequences():
    return C.contigs()


@pytest.fixture(scope="module")
def crafted(sequences):
    reads = C.crafted(sequences)
    return reads, np.array([list(read) for _, _, read in reads], dtype=np.uint8)


@pytest.fixture(scope="module", params=F["PADDINGS"])
def mapped(request, torch_gpu, sequences):
    padding = request.param
    return SimpleNamespace(padding=padding, starts=C.layout(F["LENS"], W, padding)[0],
                           mapper=B.ContigMapper(NAMES, sequences, W, ST, contig_padding=None if padding == W else padding))


# ---- 1. the clip kernel alone ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k, cap", ((1, 6), (5, 6), (64, 6), (5, 4)))
def test_the_clip_kernel_equals_the_model_on_the_hand_written_lists(torch_gpu, k, cap):
    torch = torch_gpu
    lens = C.CLIP_LAYOUT["lens"]
    starts, total = C.layout(lens, C.CLIP_LAYOUT["W"])
    before = C.clip_case_lists(k, cap)
    want = C.clip_lists(starts, lens, total, **before, cap=cap)
    dev = {name: torch.from_numpy(array.copy()).cuda() for name, array in before.items()}
    n_reads = before["scores"].shape[0]
    contig = torch.full((n_reads, k), -9, dtype=torch.int32, device="cuda")
    d_starts, d_lens = torch.tensor(starts, dtype=torch.int64, device="cuda"), torch.tensor(lens, dtype=torch.int64, device="cuda")
    B.check(B.lib().bgsa_hip_contig_clip_dev(d_starts.data_ptr(), d_lens.data_ptr(), len(lens), total, n_reads, k, dev["scores"].data_ptr(),
                                             dev["strand"].data_ptr(), dev["ref_begin"].data_ptr(), dev["ref_end"].data_ptr(),
                                             dev["keep"].data_ptr(), dev["n_ops"].data_ptr(), dev["cigar"].data_ptr(), cap, contig.data_ptr(), None),
            "contig_clip_dev")
    torch.cuda.synchronize()
    got = {name: tensor.cpu().numpy() for name, tensor in dev.items()}
    for name in ("scores", "strand", "ref_begin", "ref_end", "keep", "n_ops", "cigar"):
        assert got[name].dtype == before[name].dtype and np.array_equal(got[name], want[name]), name
    assert np.array_equal(contig.cpu().numpy(), want["contig"])
    behind = np.arange(cap)[None, None, :] >= np.maximum(before["n_ops"], got["n_ops"])[:, :, None]
    assert (got["cigar"][behind] == C.SENTINEL).all()      # nothing is written behind a row's runs
    assert (got["n_ops"] > cap).any() == (cap == 4)


# ---- 2. the four map_reads entry points ---------------------------------------------------------------------------------------------
PROJECT_RUNS = re.compile(r"(\d+)([IDX=])")      # the project's letters: I consumes a reference base only, D a read base only


def assert_equal_to_the_model(got: B.ContigHits, model: dict, starts, what: str) -> None:
    want = C.local(model, starts)
    for name in C.FIELDS:
        mine = getattr(got, name)
        assert mine.shape == want[name].shape and np.array_equal(mine, want[name]), (what, name, mine.tolist(), want[name].tolist())
    assert got.cigars == want["cigars"], what


def assert_the_properties(got: B.ContigHits, reads, sequences, bound, what: str) -> None:
    for c, read in enumerate(reads):
        read = bytes(read)
        kept = np.flatnonzero(got.keep[c])
        for r in kept:
            which, begin, end = int(got.contig[c, r]), int(got.ref_begin[c, r]), int(got.ref_end[c, r])
            assert 0 <= which < len(sequences) and 0 <= begin < end <= len(sequences[which]), (what, c, r)
            runs = [(int(n), op) for n, op in PROJECT_RUNS.findall(got.cigars[c][r])]
            assert "".join(f"{n}{op}" for n, op in runs) == got.cigars[c][r]
            assert sum(n for n, op in runs if op != "D") == end - begin and sum(n for n, op in runs if op != "I") == len(read), (what, c, r)
            assert sum(n for n, op in runs if op != "=") == -int(got.scores[c, r]), (what, c, r)
        if b"N" not in read:
            best = C.contig_distance(read, sequences)
            if bound is not None and best > bound:
                assert kept.size == 0, (what, c)
            else:
                assert kept.size and -int(got.scores[c, kept[0]]) == best, (what, c, best)


def test_map_reads_and_map_reads_seeded_equal_the_model(mapped, sequences, crafted):
    _, reads = crafted
    padding = None if mapped.padding == W else mapped.padding
    for seeded in (False, True):
        what = f"padding {mapped.padding}, seeded {seeded}"
        entry = mapped.mapper.map_reads_seeded if seeded else mapped.mapper.map_reads
        got = entry(reads, K_BEST, MAX_DISTANCE)
        assert isinstance(got, B.ContigHits)
        assert_equal_to_the_model(got, C.map_reads_model(sequences, W, ST, padding, reads, K_BEST, MAX_DISTANCE, MAX_DISTANCE if seeded else None),
                                  mapped.starts, what)
        assert_the_properties(got, reads, sequences, MAX_DISTANCE, what)
        small = entry(reads, K_BEST, MAX_DISTANCE, block_rows=5)
        assert all(np.array_equal(a, b) for a, b in zip(B.reference.hit_arrays(got), B.reference.hit_arrays(small))) and got.cigars == small.cigars
        assert np.array_equal(got.contig, small.contig)
    assert mapped.mapper.contig_starts.tolist() == mapped.starts and mapped.mapper.contig_lens.tolist() == list(F["LENS"])


def test_the_ragged_entry_points_equal_the_model(mapped, sequences, crafted):
    named, _ = crafted
    reads = [read[: N - i % 5] for i, (_, _, read) in enumerate(named)]      # 20..24 bp
    assert {len(read) for read in reads} == {20, 21, 22, 23, 24}
    padding = None if mapped.padding == W else mapped.padding
    for seeded in (False, True):
        what = f"ragged, padding {mapped.padding}, seeded {seeded}"
        entry = mapped.mapper.map_reads_seeded_ragged if seeded else mapped.mapper.map_reads_ragged
        got = entry(reads, K_BEST, MAX_DISTANCE)
        assert_equal_to_the_model(got, C.map_ragged_model(sequences, W, ST, padding, reads, K_BEST, MAX_DISTANCE, seeded), mapped.starts, what)
        assert_the_properties(got, reads, sequences, MAX_DISTANCE, what)


def test_a_read_around_a_contig_is_clipped_on_both_sides(mapped, sequences):
    padding = None if mapped.padding == W else mapped.padding
    for n, want in ((24, (C.STUB, 0, 10, -14, "7D10=7D")), (30, (C.READ_LONG, 0, 24, -6, "3D24=3D"))):
        rows = np.array([list(read) for _, _, read in C.crafted_unbounded(sequences)[n]], dtype=np.uint8)
        got = mapped.mapper.map_reads(rows, K_BEST)      # max_distance=None: every selected hit is placed
        assert_equal_to_the_model(got, C.map_reads_model(sequences, W, ST, padding, rows, K_BEST, None), mapped.starts, f"{n} bp around a contig")
        assert_the_properties(got, rows, sequences, None, f"{n} bp around a contig")
        for c in range(2):
            r = int(np.flatnonzero(got.contig[c] == want[0])[0])
            assert got.keep[c, r] and (got.contig[c, r], got.ref_begin[c, r], got.ref_end[c, r], got.scores[c, r], got.cigars[c][r]) == want
            assert got.strand[c, r] == c


def test_a_clipped_script_beyond_its_row_is_reported_as_an_overflow_is(mapped, crafted):
    named, reads = crafted
    c = next(i for i, (name, strand, _) in enumerate(named) if (name, strand) == ("N tail over the end", "+"))
    one = reads[c: c + 1]      # 24= in the padded reference: one run; clipped 21=3D: two
    with pytest.raises(B.BgsaHipError, match=r"hit 0 of read 0 has 2 runs, its row holds 1 \(raise cigar_cap\)"):
        mapped.mapper.map_reads(one, K_BEST, MAX_DISTANCE, cigar_cap=1)
    with pytest.raises(B.BgsaHipError, match=r"has 2 runs, its row holds 1 \(raise cigar_cap\)"):
        mapped.mapper.map_reads_sam(one, k_best=K_BEST, max_distance=MAX_DISTANCE, seeded=False, cigar_cap=1)
    assert mapped.mapper.map_reads(one, K_BEST, MAX_DISTANCE, cigar_cap=2).cigars[0][0] == "21=3D"


# ---- 3. pairs ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def paired_case(torch_gpu, sequences):
    P = C.PAIRS
    pairs = C.crafted_pairs(sequences)
    reads1 = np.array([list(one) for _, one, _ in pairs], dtype=np.uint8)
    reads2 = np.array([list(two) for _, _, two in pairs], dtype=np.uint8)
    mapper = B.ContigMapper(NAMES, sequences, W, ST, contig_padding=P["PADDING"])
    args = dict(k_best=P["K_BEST"], max_distance=MAX_DISTANCE)
    return SimpleNamespace(mapper=mapper, reads=(reads1, reads2), args=args, starts=C.layout(F["LENS"], W, P["PADDING"])[0],
                           paired=mapper.map_pairs(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], **args))


def test_map_pairs_equals_the_model_on_the_crafted_pairs(paired_case, sequences):
    P, got = C.PAIRS, paired_case.paired
    model = C.map_pairs_model(sequences, W, ST, P["PADDING"], *paired_case.reads, P["INSERT_MIN"], P["INSERT_MAX"], P["K_BEST"], MAX_DISTANCE)
    assert_equal_to_the_model(got.end1, model["end1"], paired_case.starts, "end 1")
    assert_equal_to_the_model(got.end2, model["end2"], paired_case.starts, "end 2")
    for name in ("rescued1", "rescued2") + C.PR.OUTPUTS:
        assert np.array_equal(getattr(got, name), model[name]), (name, getattr(got, name), model[name])
    assert got.proper.tolist() == [1, 0, 0] and got.insert.tolist() == [100, 0, 0] and got.slot2[2] == -1 and (got.slot1 >= 0).all()
    chosen = paired_case.mapper.pairs_of(got)
    assert chosen[0] == (B.ContigPlacement(C.CHR_A, 0, 20, 44, 0, "24="), B.ContigPlacement(C.CHR_A, 1, 96, 120, 0, "24="), True)
    assert chosen[1] == (B.ContigPlacement(C.CHR_A, 0, 176, 200, 0, "24="), B.ContigPlacement(C.CHR_B, 1, 0, 24, 0, "24="), False)
    assert chosen[2][1] is None and chosen[2][0][:4] == (C.CHR_A, 0, 60, 84)
    for reads, end in zip(paired_case.reads, (got.end1, got.end2)):
        assert_the_properties(end, reads, sequences, MAX_DISTANCE, "an end of a pair")
    with pytest.raises(B.BgsaHipError, match="exceeds contig_padding 120"):
        paired_case.mapper.map_pairs(*paired_case.reads, P["INSERT_MIN"], P["PADDING"] + 1, **paired_case.args)


# ---- 4. SAM records ----------------------------------------------------------------------------------------------------------------------
def lines_of(records: B.SamRecords) -> list:
    text = records.text.tobytes()
    return [text[records.offsets[i]: records.offsets[i + 1]] for i in range(records.offsets.size - 1)]


def assert_records(got: B.SamRecords, want: tuple, what: str) -> list:
    lines, flag, pos, mapq, nm = want
    got_lines = lines_of(got)
    assert len(got_lines) == len(lines), what
    for i, (mine, theirs) in enumerate(zip(got_lines, lines)):
        assert mine == theirs, (what, i, mine, theirs)
    assert got.text.tobytes() == b"".join(lines)
    for name, column in (("flag", flag), ("pos", pos), ("mapq", mapq), ("nm", nm)):
        assert getattr(got, name).tolist() == column, (what, name)
    return [C.fields_of(line) for line in got_lines]


def assert_a_line_rebuilds_its_contig(f: dict, sequences) -> None:
    """RNAME names a contig, POS is local to it, and SEQ + CIGAR + MD give back exactly that contig's bases."""
    which = list(F["NAMES"]).index(f["rname"])
    spanned = S.rebuild_reference(f["seq"], f["cigar"], f["md"])
    assert 1 <= f["pos"] and f["pos"] - 1 + len(spanned) <= len(sequences[which])
    assert spanned == sequences[which][f["pos"] - 1: f["pos"] - 1 + len(spanned)]


def test_map_reads_sam_equals_the_model(mapped, sequences, crafted):
    named, reads = crafted
    names = [f"{name.replace(' ', '_')}/{strand}".encode() for name, strand, _ in named]
    quals = [bytes(np.random.default_rng(c).integers(33, 127, size=N, dtype=np.uint8)) for c in range(len(named))]
    for seeded in (True, False):
        hits = (mapped.mapper.map_reads_seeded if seeded else mapped.mapper.map_reads)(reads, K_BEST, MAX_DISTANCE)
        want = C.single_records(hits, reads, names, quals, sequences, F["NAMES"], MAX_DISTANCE if seeded else -1)
        got = mapped.mapper.map_reads_sam(reads, names, quals, k_best=K_BEST, max_distance=MAX_DISTANCE, seeded=seeded)
        mapped_lines = 0
        for f, (name, strand, read) in zip(assert_records(got, want, f"padding {mapped.padding}, seeded {seeded}"), named):
            assert (f["rnext"], f["pnext"], f["tlen"]) == (b"*", 0, 0)
            if f["flag"] & 4:
                assert (f["rname"], f["pos"], f["cigar"]) == (b"*", 0, "*") and (name == "all N" or name.endswith("by 5"))
                continue
            assert_a_line_rebuilds_its_contig(f, sequences)
            mapped_lines += 1
        assert mapped_lines == len(named) - 6
    ragged = [read[: N - i % 5] for i, (_, _, read) in enumerate(named)]
    hits = mapped.mapper.map_reads_seeded_ragged(ragged, K_BEST, MAX_DISTANCE)
    want = C.single_records(hits, ragged, None, None, sequences, F["NAMES"], MAX_DISTANCE)
    assert_records(mapped.mapper.map_reads_sam(ragged, k_best=K_BEST, max_distance=MAX_DISTANCE), want, "mixed lengths")


def test_map_pairs_sam_equals_the_model(paired_case, sequences):
    P, (reads1, reads2) = C.PAIRS, paired_case.reads
    names = [b"proper", b"across", b"half"]
    want = C.pair_records(paired_case.paired, reads1, reads2, names, None, None, sequences, F["NAMES"], paired_case.starts, (MAX_DISTANCE,) * 2)
    got = paired_case.mapper.map_pairs_sam(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], names, **paired_case.args)
    f = assert_records(got, want, "pairs")
    assert [(x["rname"], x["pos"], x["rnext"], x["pnext"], x["tlen"]) for x in f[:2]] == [(b"chrA", 21, b"=", 97, 100), (b"chrA", 97, b"=", 21, -100)]
    assert [x["flag"] for x in f[:2]] == [1 + 2 + 32 + 64, 1 + 2 + 16 + 128]
    assert [(x["rname"], x["pos"], x["rnext"], x["pnext"], x["tlen"]) for x in f[2:4]] == [(b"chrA", 177, b"chrB", 1, 0), (b"chrB", 1, b"chrA", 177, 0)]
    assert [x["flag"] for x in f[2:4]] == [1 + 32 + 64, 1 + 16 + 128]      # not proper: the contigs differ
    assert [(x["rname"], x["pos"], x["rnext"], x["pnext"], x["tlen"], x["cigar"]) for x in f[4:]] == \
        [(b"chrA", 61, b"*", 0, 0, "24="), (b"chrA", 61, b"=", 61, 0, "*")]      # the unmapped end takes its mate's contig and '='
    assert [x["flag"] for x in f[4:]] == [1 + 8 + 64, 1 + 4 + 128]
    for x in f[:5]:
        assert_a_line_rebuilds_its_contig(x, sequences)
    with pytest.raises(B.BgsaHipError, match="exceeds contig_padding 120"):
        paired_case.mapper.map_pairs_sam(reads1, reads2, P["INSERT_MIN"], P["PADDING"] + 1, names, **paired_case.args)


# ---- 5. the regression: one contig is the old path ----------------------------------------------------------------------------------
def test_one_contig_is_reference_mapper_on_that_sequence(torch_gpu, sequences, crafted):
    _, reads = crafted
    whole = sequences[C.CHR_A]
    assert len(whole) >= W
    old, new = B.ReferenceMapper(whole, W, ST), B.ContigMapper(["ref"], [whole], W, ST)
    assert new.ref_len == old.ref_len == len(whole) and new.contig_starts.tolist() == [0] and new.sam_header() == old.sam_header()
    ragged = [bytes(row[: N - i % 5]) for i, row in enumerate(reads)]
    placed = 0
    for name, args in (("map_reads", (reads, K_BEST, MAX_DISTANCE)), ("map_reads", (reads, K_BEST)), ("map_reads_seeded", (reads, K_BEST, MAX_DISTANCE)),
                       ("map_reads_ragged", (ragged, K_BEST, MAX_DISTANCE)), ("map_reads_seeded_ragged", (ragged, K_BEST, MAX_DISTANCE))):
        want, got = getattr(old, name)(*args), getattr(new, name)(*args)
        for field in B.ReferenceHits._fields:
            mine, theirs = getattr(got, field), getattr(want, field)
            assert mine == theirs if field == "cigars" else (mine.dtype == theirs.dtype and np.array_equal(mine, theirs)), (name, field)
        assert np.array_equal(got.contig, np.where(want.ref_begin >= 0, 0, -1))
        placed += int(want.keep.sum())
    assert placed > 50
    for seeded in (True, False):
        want = old.map_reads_sam(reads, k_best=K_BEST, max_distance=MAX_DISTANCE, seeded=seeded)
        got = new.map_reads_sam(reads, k_best=K_BEST, max_distance=MAX_DISTANCE, seeded=seeded)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and (got.flag != 4).sum() > 10
    pair = (np.array([list(whole[20:44]), list(whole[60:84])], np.uint8),
            np.array([list(S.reverse_complement(whole[96:120])), list(S.reverse_complement(whole[172:196]))], np.uint8))
    args = dict(k_best=1, max_distance=MAX_DISTANCE)
    wide = B.ContigMapper(["ref"], [whole], W, ST, contig_padding=120)      # room for the insert; one contig: the same reference
    want, got = old.map_pairs(*pair, 60, 120, **args), wide.map_pairs(*pair, 60, 120, **args)
    assert want.proper.tolist() == [1, 0] and all(np.array_equal(a, b) for a, b in zip(got[2:], want[2:]))
    assert all(np.array_equal(a, b) for e in (0, 1) for a, b in zip(B.reference.hit_arrays(got[e]), B.reference.hit_arrays(want[e])))
    assert got.end1.cigars == want.end1.cigars and got.end2.cigars == want.end2.cigars
    assert all(np.array_equal(a, b) for a, b in zip(wide.map_pairs_sam(*pair, 60, 120, **args), old.map_pairs_sam(*pair, 60, 120, **args)))

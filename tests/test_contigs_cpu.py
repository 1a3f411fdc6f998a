"""A reference of several contigs, without a GPU: the layout against the C call, the model's clip on hand-written run lists for
every branch of the rule, the model pipeline's NM against a plain DP per contig on the crafted reads, read_fasta, the header bytes,
ContigMapper's refusals before it touches a device, and the four new symbols: declared, exported by both flavours, prototyped,
refusing bad arguments before any HIP call."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import contig_reference as C  # noqa: E402
import sam_reference as S  # noqa: E402

EINVAL = -1
PTR = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SYMBOLS = ("bgsa_hip_contig_layout", "bgsa_hip_contig_clip_dev", "bgsa_hip_sam_measure_contigs_dev", "bgsa_hip_sam_emit_contigs_dev")
F = C.FIXTURE


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


def c_layout(L, lens, W, P):
    sizes = (ctypes.c_int64 * max(len(lens), 1))(*lens)
    starts = (ctypes.c_int64 * max(len(lens), 1))()
    total = ctypes.c_int64(-7)
    rc = L.bgsa_hip_contig_layout(ctypes.cast(sizes, ctypes.c_void_p), len(lens), W, P, ctypes.cast(starts, ctypes.c_void_p),
                                  ctypes.cast(ctypes.pointer(total), ctypes.c_void_p))
    return rc, list(starts)[: len(lens)], total.value


# ---- 1. the layout ------------------------------------------------------------------------------------------------------------------
def test_the_layout_is_the_c_calls_over_a_grid(L):
    rng = np.random.default_rng(3)
    for W in (1, 5, 48):
        for P in (W, W + 1, 3 * W + 2):
            for C_n in (1, 2, 7):
                lens = [int(x) for x in rng.integers(1, 3 * W + 2, size=C_n)]
                lens[0] = 1
                rc, starts, total = c_layout(L, lens, W, P)
                mine, whole = B.contig_layout(lens, W, P)
                assert rc == 0 and (starts, total) == C.layout(lens, W, P) == (mine.tolist(), whole)
                assert starts[0] == 0 and total == sum(lens) + P * (C_n - 1)
                assert all(b - (a + n) == P for a, n, b in zip(starts, lens, starts[1:]))
    assert B.contig_layout(F["LENS"], F["W"])[0].tolist() == [0, 78, 326, 464, 536] and B.contig_layout(F["LENS"], F["W"])[1] == 546
    assert C.padded([b"AC", b"G"], 4) == b"ACNNNNG" and C.padded([b"AC"], 4) == b"ACNN"      # padded up to the window where shorter


def test_the_layout_refusals_in_c_and_in_python(L):
    for lens, W, P, text in (([], 4, 4, "n_contigs"), ([3, 0, 2], 4, 4, "below 1"), ([3, -1], 4, 4, "below 1"), ([3, 2], 4, 3, "padding"),
                             ([3, 2], 0, 0, "window_len"), ([2 ** 62, 2 ** 62], 4, 4, "int64"), ([5, 5], 4, 2 ** 63 - 8, "int64")):
        rc, _, total = c_layout(L, lens, W, P)
        assert rc == EINVAL and total == -7 and text.encode() in L.bgsa_hip_last_error(), (lens, W, P)
        with pytest.raises(B.BgsaHipError, match="contig_layout: rc=-1"):
            B.contig_layout(lens, W, P)
    assert L.bgsa_hip_contig_layout(None, 1, 4, 4, PTR, PTR) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert B.contig_layout([3, 2], 4)[0].tolist() == [0, 7]      # padding None: the window


# ---- 2. the clip on hand-written run lists ----------------------------------------------------------------------------------------
def clip_layout():
    return C.layout(C.CLIP_LAYOUT["lens"], C.CLIP_LAYOUT["W"])


@pytest.mark.parametrize("name", sorted(C.CLIP_CASES))
def test_the_models_clip_gives_what_the_rule_says(name):
    (strand, begin, end, distance, runs), want = C.CLIP_CASES[name]
    starts, total = clip_layout()
    hit = C.clip_hit(starts, C.CLIP_LAYOUT["lens"], total, begin, end, distance, runs)
    if want is None:
        assert hit["contig"] is None
        return
    assert (hit["contig"], hit["begin"], hit["end"], hit["distance"], hit["runs"]) == want
    on_ref = sum(n for n, op in hit["runs"] if op != C.READ_ONLY)
    assert on_ref == hit["end"] - hit["begin"] and len(hit["runs"]) <= len(runs) + 2
    assert sum(n for n, op in hit["runs"] if op != C.REF_ONLY) == sum(n for n, op in runs if op != C.REF_ONLY)      # the read is whole
    s, n = starts[hit["contig"]], C.CLIP_LAYOUT["lens"][hit["contig"]]
    assert s <= hit["begin"] <= hit["end"] <= s + n and (hit["begin"] < hit["end"] or runs == hit["runs"])


def test_the_cases_cover_every_branch_of_the_rule():
    starts, total = clip_layout()
    assert (starts, total) == ([0, 28, 46], 51)
    grown = {name: len(want[4]) - len(hit[4]) for name, (hit, want) in C.CLIP_CASES.items() if want is not None}
    assert grown["the first run splits"] == 1 and grown["two more runs"] == 2 and grown["one run holds the contig"] == 2
    assert grown["reference-only columns are dropped"] == -1 and grown["a read-only run on the way"] == -2
    delta = {name: want[3] - hit[3] for name, (hit, want) in C.CLIP_CASES.items() if want is not None}
    assert delta["= on padding"] == 3 and delta["reference-only columns are dropped"] == -2 and delta["the first run splits"] == 0
    assert sum(want is None for _, want in C.CLIP_CASES.values()) == 2
    assert {hit[0] for hit, _ in C.CLIP_CASES.values()} == {0, 1}


def test_the_lists_growth_overflow_empty_result_and_keep():
    starts, total = clip_layout()
    lens, names = C.CLIP_LAYOUT["lens"], list(C.CLIP_CASES)
    before = C.clip_case_lists(5, 6)
    after = C.clip_lists(starts, lens, total, **before, cap=6)
    flat = {name: divmod(i, 5) for i, name in enumerate(names)}
    for name, at in flat.items():
        want = C.CLIP_CASES[name][1]
        if want is None:      # the empty result: unplaced, the score and the strand stay
            assert (after["ref_begin"][at], after["ref_end"][at], after["keep"][at], after["n_ops"][at], after["contig"][at]) == (-1, -1, 0, 0, -1)
            assert after["scores"][at] == before["scores"][at] and after["strand"][at] == before["strand"][at]
            assert (after["cigar"][at] == before["cigar"][at]).all()
            continue
        n = len(want[4])
        assert (after["contig"][at], after["ref_begin"][at], after["ref_end"][at], -after["scores"][at], after["n_ops"][at]) == want[:4] + (n,)
        assert after["cigar"][at][:n].tolist() == [length << 4 | op for length, op in want[4]]
        assert (after["cigar"][at][n:] == before["cigar"][at][n:]).all()          # nothing behind the runs is written
    unused = (len(before["scores"]) - 1, 4)      # behind the two hits of the last read
    assert before["ref_begin"][unused] == -1 and all((after[f][unused] == before[f][unused]).all() for f in before) and after["contig"][unused] == -1
    # the two hits that meet only before the clip: the second one is hidden before, kept after
    assert before["keep"][-1].tolist()[:2] == [1, 0] and after["keep"][-1].tolist()[:2] == [1, 1]
    assert after["ref_end"][-1, 0] == 20 and after["ref_begin"][-1, 1] == 28 and after["contig"][-1].tolist()[:2] == [0, 1]
    # a row of 4: the script of 5 runs does not fit — n_ops says so, the row is left, the interval and the score are the clipped ones
    small = C.clip_case_lists(5, 4)
    cut = C.clip_lists(starts, lens, total, **small, cap=4)
    at = flat["two more runs"]
    assert cut["n_ops"][at] == 5 and (cut["cigar"][at] == small["cigar"][at]).all() and (cut["ref_begin"][at], cut["ref_end"][at]) == (28, 38)
    at = flat["one run holds the contig"]
    assert cut["n_ops"][at] == 3 and cut["cigar"][at].tolist() == [3 << 4 | 2, 10 << 4 | 8, 3 << 4 | 2, C.SENTINEL]


# ---- 3. the crafted reads: the model pipeline against a DP that knows one contig at a time ---------------------------------------------
@pytest.fixture(scope="module")
def fixture_model():
    sequences = C.contigs()
    crafted = C.crafted(sequences)
    reads = np.array([list(read) for _, _, read in crafted], dtype=np.uint8)
    linear = C.map_reads_model(sequences, F["W"], F["S"], None, reads, F["K_BEST"], F["MAX_DISTANCE"])
    return sequences, crafted, reads, linear


def test_nm_is_the_dp_minimum_over_the_contigs_for_every_read_without_n(fixture_model):
    sequences, crafted, reads, linear = fixture_model
    checked = 0
    for c, (name, strand, read) in enumerate(crafted):
        if b"N" in read:
            continue
        kept = np.flatnonzero(linear["keep"][c])
        want = C.contig_distance(read, sequences)
        if want > F["MAX_DISTANCE"]:
            assert kept.size == 0, (name, strand)
        else:
            assert -linear["scores"][c, kept[0]] == want, (name, strand)
        checked += 1
    assert checked == len(crafted) - 4


def test_the_crafted_set_covers_what_it_names(fixture_model):
    sequences, crafted, reads, linear = fixture_model
    starts, total = C.layout(F["LENS"], F["W"])
    hits = C.local(linear, starts)
    assert B.max_stride(F["W"], F["N"], F["MAX_DISTANCE"]) == 21 >= F["S"] and total == 546
    assert F["LENS"][C.TINY] < F["W"] and F["LENS"][C.READ_LONG] == F["N"] and F["LENS"][C.STUB] < F["N"]
    first = {}
    for c, (name, strand, read) in enumerate(crafted):
        kept = np.flatnonzero(hits["keep"][c])
        first[name, strand] = None if kept.size == 0 else tuple(int(hits[f][c, kept[0]]) for f in ("contig", "strand", "ref_begin", "ref_end", "scores")) \
            + (hits["cigars"][c][kept[0]],)
    for strand, s in (("+", 0), ("-", 1)):
        assert first["interior exact", strand] == (C.CHR_A, s, 50, 74, 0, "24=")
        assert [first[f"interior {n} edit{'s' * (n > 1)}", strand][4] for n in (1, 2, 3)] == [-1, -2, -3]
        assert first["inside the contig below the window", strand][:4] == (C.TINY, s, 3, 27)
        assert first["flush at the first base", strand] == (C.CHR_A, s, 0, 24, 0, "24=")
        assert first["flush at the last base", strand] == (C.CHR_A, s, 176, 200, 0, "24=")
        assert first["the read-long contig itself", strand] == (C.READ_LONG, s, 0, 24, 0, "24=")
        for over in (1, 3):
            at_start, at_end = first[f"over the start by {over}", strand], first[f"over the end by {over}", strand]
            assert at_start[:5] == (C.CHR_B, s, 0, 24 - over, -over) and at_end[:5] == (C.CHR_B, s, 66 + over, 90, -over)
        assert first["over the start by 5", strand] is None and first["over the end by 5", strand] is None      # beyond the bound
        assert first["N tail over the end", strand] == (C.CHR_A, s, 179, 200, -3, "21=3D")      # '=' on padding: 0 before the clip
        assert first["all N", strand] is None
    # ... and the clip had work to do: in the padded reference these hits reached into the padding
    plain = C.M.map_reads_host(C.padded(sequences, F["W"]), F["W"], F["S"], reads, k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    index = {(name, strand): c for c, (name, strand, _) in enumerate(crafted)}
    c = index["N tail over the end", "+"]
    assert plain["scores"][c, 0] == 0 and plain["ref_end"][c, 0] == starts[C.CHR_A] + 203
    c = index["all N", "+"]
    assert plain["keep"][c].any() and (plain["scores"][c][plain["keep"][c] != 0] == 0).all() and not linear["keep"][c].any()
    assert (linear["ref_begin"][c] == -1).all() and (linear["contig"][c] == -1).all()
    # the reads for max_distance=None and the pairs
    around = C.crafted_unbounded(sequences)
    assert sorted(around) == [24, 30] and all(len(reads) == 2 for reads in around.values())
    for n, want in ((24, (C.STUB, 0, 10, -14, "7D10=7D")), (30, (C.READ_LONG, 0, 24, -6, "3D24=3D"))):
        rows = np.array([list(read) for _, _, read in around[n]], dtype=np.uint8)
        got = C.local(C.map_reads_model(sequences, F["W"], F["S"], None, rows, F["K_BEST"], None), starts)
        for c in range(2):
            r = int(np.flatnonzero(got["contig"][c] == want[0])[0])
            assert got["keep"][c, r] and (got["contig"][c, r], got["ref_begin"][c, r], got["ref_end"][c, r], got["scores"][c, r], got["cigars"][c][r]) == want
    pairs = C.crafted_pairs(sequences)
    assert [name for name, _, _ in pairs] == ["proper inside one contig", "mates on neighbouring contigs", "end 2 unmapped"]
    assert C.contig_distance(pairs[2][2], sequences) > F["MAX_DISTANCE"]
    far, _ = C.layout(F["LENS"], F["W"], C.PAIRS["PADDING"])
    assert far[C.CHR_B] + F["N"] - (far[C.CHR_A] + 176) > C.PAIRS["INSERT_MAX"] >= 120 - 20 >= C.PAIRS["INSERT_MIN"]
    near, _ = C.layout(F["LENS"], F["W"])
    assert C.PAIRS["INSERT_MIN"] <= near[C.CHR_B] + F["N"] - (near[C.CHR_A] + 176) <= C.PAIRS["INSERT_MAX"]     # at padding 48 it would pass


def test_the_models_sam_lines_on_the_crafted_reads(fixture_model):
    sequences, crafted, reads, linear = fixture_model
    starts, _ = C.layout(F["LENS"], F["W"])
    hits = C.local(linear, starts)
    lines, flag, pos, mapq, nm = C.single_records(hits, reads, None, None, sequences, F["NAMES"], -1)
    for c, (name, strand, read) in enumerate(crafted):
        f = C.fields_of(lines[c])
        kept = np.flatnonzero(hits["keep"][c])
        if kept.size == 0:
            assert (f["flag"], f["rname"], f["pos"], f["cigar"], f["nm"]) == (4, b"*", 0, "*", None)
            continue
        r = kept[0]
        which = int(hits["contig"][c, r])
        assert f["rname"] == F["NAMES"][which] and f["pos"] == hits["ref_begin"][c, r] + 1 and f["rnext"] == b"*" and f["tlen"] == 0
        assert S.rebuild_reference(f["seq"], f["cigar"], f["md"]) == sequences[which][f["pos"] - 1: int(hits["ref_end"][c, r])]
        assert f["nm"] == -hits["scores"][c, r] == nm[c] and flag[c] == (16 if hits["strand"][c, r] else 0)


# ---- 4. read_fasta, the header, the mapper's refusals ----------------------------------------------------------------------------------
def test_read_fasta_and_its_refusals(tmp_path):
    text = b">chr1 first\nACGT\nAC GT\n\n>chr2\nNNNN\n"
    assert B.read_fasta(text) == (["chr1", "chr2"], [b"ACGTACGT", b"NNNN"])
    (tmp_path / "ref.fa").write_bytes(text)
    assert B.read_fasta(tmp_path / "ref.fa") == B.read_fasta(str(tmp_path / "ref.fa")) == B.read_fasta(text)
    for bad, why in ((b">a\n>b\nAC\n", "record a is empty"), (b">a\nAC\n>b\n", "record b is empty"), (b">a\nAC\n>a\nGT\n", "given twice"),
                     (b"ACGT\n>a\nAC\n", "in front of the first"), (b"", "no record"), (b">\nAC\n", "no name")):
        with pytest.raises(B.BgsaHipError, match=why):
            B.read_fasta(bad)


def bare_mapper(padding: int = 48):
    mapper = object.__new__(B.ContigMapper)      # no aligner, no reference on a device: touching either raises AttributeError
    mapper.contig_names, mapper.contig_lens = list(F["NAMES"]), np.array(F["LENS"], dtype=np.int64)
    mapper.contig_padding = padding
    mapper.contig_starts, mapper.ref_len = B.contig_layout(F["LENS"], F["W"], padding)
    mapper.window_len, mapper.stride, mapper.both_strands = F["W"], F["S"], True
    mapper.n_windows = B.window_plan(mapper.ref_len, F["W"], F["S"])[0]
    mapper.n_ids, mapper.last_pair_stats, mapper.last_seed_stats = 2 * mapper.n_windows, None, None
    return mapper


def test_the_header_has_one_sq_per_contig_in_order():
    want = b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:tiny\tLN:30\n@SQ\tSN:chrA\tLN:200\n@SQ\tSN:chrB\tLN:90\n@SQ\tSN:read-long\tLN:24\n" \
           b"@SQ\tSN:stub\tLN:10\n@PG\tID:bgsa-hip\n"
    assert bare_mapper().sam_header() == want == bare_mapper(70).sam_header("ignored")


def test_the_mapper_refuses_before_it_touches_a_device():
    sequences = C.contigs()
    for over, text in ((dict(contig_padding=47), "contig_padding 47 is below window_len 48"), (dict(names=["a", "b c", "d", "e", "f"]), "name of contig 1 holds"),
                       (dict(names=["a", "b", "", "e", "f"]), "name of contig 2 is empty"), (dict(names=["a", "b", "c", "b", "f"]), "contig name b is given twice"),
                       (dict(names=["a", "b"]), "2 names for 5 sequences"), (dict(sequences=sequences[:4] + [b""]), "contig 4 is empty"),
                       (dict(sequences=sequences[:4] + [b"AC\nGT"]), "contig 4 is not the bases of one sequence")):
        args = {**dict(names=[n.decode() for n in F["NAMES"]], sequences=sequences, window_len=F["W"], stride=F["S"], device="no-such-device"), **over}
        with pytest.raises(B.BgsaHipError, match=text):
            B.ContigMapper(**args)
    mapper, reads = bare_mapper(), np.full((3, F["N"]), ord("A"), np.uint8)
    for call in (mapper.map_pairs, mapper.map_pairs_sam):
        with pytest.raises(B.BgsaHipError, match="insert_max 49 exceeds contig_padding 48"):
            call(reads, reads, 10, 49, max_distance=2)
        with pytest.raises(B.BgsaHipError, match="max_distance is required"):      # ... and then the base class's own refusals
            call(reads, reads, 10, 48)
    with pytest.raises(B.BgsaHipError, match="k_best must lie"):
        mapper.map_reads(reads, k_best=0)
    with pytest.raises(B.BgsaHipError, match="1 names for 3 reads"):
        mapper.map_reads_sam(reads, names=["a"], max_distance=2)
    assert mapper.last_pair_stats is None and mapper.last_seed_stats is None and getattr(mapper, "_nested", 0) == 0


def test_localise_and_the_placements():
    mapper = bare_mapper()
    begin = np.array([[78, 326 + 5, -1]], dtype=np.int64)
    hits = B.ReferenceHits(np.array([[0, -2, B.reference.INT32_MIN]], np.int32), np.array([[0, 1, -1]], np.int32), begin,
                           np.where(begin >= 0, begin + 24, -1), np.array([[1, 1, 0]], np.int32), [["24=", "22=2X", None]],
                           np.array([[3, 90, -1]], np.int32))
    local = mapper.localise(hits)
    assert local.contig.tolist() == [[1, 2, -1]] and local.ref_begin.tolist() == [[0, 5, -1]] and local.ref_end.tolist() == [[24, 29, -1]]
    assert B.ContigHits._fields == B.ReferenceHits._fields + ("contig",)
    assert B.ContigMapper.placements_of(local, 2) == [[B.ContigPlacement(1, 0, 0, 24, 0, "24="), B.ContigPlacement(2, 1, 5, 29, 2, "22=2X")]]


# ---- 5. the symbols and the C ABI's refusals --------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared and hasattr(flavour, name), (path.name, name)
    assert len(L.bgsa_hip_contig_layout.argtypes) == 6 and len(L.bgsa_hip_contig_clip_dev.argtypes) == 16
    assert len(L.bgsa_hip_sam_measure_contigs_dev.argtypes) == 6 and len(L.bgsa_hip_sam_emit_contigs_dev.argtypes) == 8
    assert ctypes.sizeof(B.SamContigs) == 6 * 8 and ctypes.sizeof(B.SamBatch) == 29 * 8
    for name in ("map_reads", "map_reads_seeded", "map_reads_ragged", "map_reads_seeded_ragged", "map_pairs", "map_reads_sam", "map_pairs_sam",
                 "sam_header", "pairs_of", "placements_of", "_after_place"):
        assert name in vars(B.ContigMapper) and hasattr(B.ReferenceMapper, name), name
    assert B.ReferenceMapper._after_place(None, *(None,) * 8) is None      # the base class's hook does nothing


def test_clip_call_refusals(L):
    def call(starts=PTR, lens=PTR, n_contigs=2, ref_len=100, n_reads=1, k=3, lists=(PTR,) * 7, cap=8, contig=PTR):
        return L.bgsa_hip_contig_clip_dev(starts, lens, n_contigs, ref_len, n_reads, k, *lists[:6], lists[6], cap, contig, None)
    assert call(starts=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error() and call(lens=None) == EINVAL and call(contig=None) == EINVAL
    for i in range(7):
        lists = [PTR] * 7
        lists[i] = None
        assert call(lists=tuple(lists)) == EINVAL, i
    for k in (0, -1, 65):
        assert call(k=k) == EINVAL and b"1..64" in L.bgsa_hip_last_error()
    assert call(n_contigs=0) == EINVAL and call(n_contigs=2 ** 31) == EINVAL and call(ref_len=0) == EINVAL and call(cap=0) == EINVAL
    assert call(n_reads=-1) == EINVAL and b"n_reads" in L.bgsa_hip_last_error()
    assert call(n_reads=0) == 0 and call(n_reads=0, k=64) == 0       # nothing to do: nothing is launched


def good_batch(**over):
    fields = {name: (PTR if kind is ctypes.c_void_p else 8) for name, kind in B.SamBatch._fields_}
    fields.update(over)
    return B.SamBatch(**fields)


def good_table(**over):
    fields = {name: (PTR if kind is ctypes.c_void_p else 8) for name, kind in B.SamContigs._fields_}
    fields.update(over)
    return B.SamContigs(**fields)


def test_contig_record_call_refusals(L):
    def measure(batch, table, n=1, lengths=PTR, malformed=PTR):
        return L.bgsa_hip_sam_measure_contigs_dev(batch, table, n, lengths, malformed, None)

    def emit(batch, table, n=1, offsets=PTR, text=PTR, text_bytes=100, malformed=PTR):
        return L.bgsa_hip_sam_emit_contigs_dev(batch, table, n, offsets, text, text_bytes, malformed, None)
    assert measure(None, good_table()) == EINVAL and emit(None, good_table()) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    assert measure(good_batch(), None) == EINVAL and emit(good_batch(), None) == EINVAL and b"contig table is NULL" in L.bgsa_hip_last_error()
    for name, kind in B.SamBatch._fields_:
        bad = good_batch(**{name: None if kind is ctypes.c_void_p else 0})
        if name in ("d_quals", "d_rname", "rname_len"):        # optional; RNAME comes from the table
            assert measure(bad, good_table(), n=0) == 0 and emit(bad, good_table(), n=0) == 0, name
        else:
            assert measure(bad, good_table()) == EINVAL and emit(bad, good_table()) == EINVAL, name
    for name, kind in B.SamContigs._fields_:
        bad = good_table(**{name: None if kind is ctypes.c_void_p else 0})
        assert measure(good_batch(), bad) == EINVAL and emit(good_batch(), bad) == EINVAL, name
    assert measure(good_batch(), good_table(n_contigs=2 ** 31)) == EINVAL and b"n_contigs" in L.bgsa_hip_last_error()
    assert measure(good_batch(), good_table(), lengths=None) == EINVAL and measure(good_batch(), good_table(), malformed=None) == EINVAL
    assert emit(good_batch(), good_table(), offsets=None) == EINVAL and emit(good_batch(), good_table(), text=None) == EINVAL
    assert emit(good_batch(), good_table(), text_bytes=-1) == EINVAL and measure(good_batch(), good_table(), n=-1) == EINVAL
    assert measure(good_batch(), good_table(), n=0) == 0 and emit(good_batch(), good_table(), n=0, text_bytes=0) == 0
    one = good_batch(d_rname=None)      # the one-sequence calls still want their name
    assert L.bgsa_hip_sam_measure_dev(one, 1, PTR, PTR, None) == EINVAL and L.bgsa_hip_sam_emit_dev(one, 1, PTR, PTR, 100, PTR, None) == EINVAL

"""SAM records, without a GPU: the host model checks itself (SEQ + CIGAR + MD rebuild the reference on a crafted set), the MAPQ
table, the TLEN sign, every refusal of check_sam_call, the header bytes, the SAM entry points refusing before they touch a device,
and the three new symbols: declared, exported by both flavours, prototyped, refusing bad arguments before any HIP call."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import sam_reference as S  # noqa: E402

EINVAL = -1
PTR = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SYMBOLS = ("bgsa_hip_sam_mapq_dev", "bgsa_hip_sam_measure_dev", "bgsa_hip_sam_emit_dev")

#                      0         1         2         3         4         5
#                      012345678901234567890123456789012345678901234567890123456789
REFERENCE = b"ACGTTGCAAGCTNACGGATCCATGACTTGACCAGTNNTACGATCGGATTACAGCTAGCTAAGG"
CRAFTED = {      # name -> (begin, SAM runs, the MD the definitions give)
    "exact": (0, [(20, "=")], "20"),
    "substitution": (2, [(5, "="), (1, "X"), (6, "=")], "5A6"),
    "adjacent substitutions": (2, [(5, "="), (2, "X"), (5, "=")], "5A0A5"),
    "deletion then mismatch": (14, [(4, "="), (2, "D"), (1, "X"), (5, "=")], "4^TC0C5"),
    "insertion between two deletions": (20, [(3, "="), (2, "D"), (3, "I"), (2, "D"), (4, "=")], "3^GA0^CT4"),
    "leading and trailing insertion": (30, [(2, "I"), (9, "="), (3, "I")], "9"),
    "insertion inside a match": (40, [(4, "="), (2, "I"), (5, "="), (1, "X"), (3, "=")], "9A3"),
    "N over N": (8, [(10, "=")], "10"),
    "mismatch first and last": (45, [(1, "X"), (6, "="), (1, "X")], "0G6G0"),
    "deletion at the end of the reference": (52, [(6, "="), (3, "D"), (2, "=")], None),
}


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- 1. the model checks itself -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CRAFTED))
@pytest.mark.parametrize("reverse", (False, True))
def test_seq_cigar_and_md_rebuild_the_reference(name, reverse):
    begin, runs, md = CRAFTED[name]
    rec = S.craft(np.random.default_rng(5), REFERENCE, begin, runs, reverse)
    text = S.crafted_line(rec, b"q", None, REFERENCE, b"ref", 16 if reverse else 0, 60)
    fields = text[:-1].split(b"\t")
    assert len(fields) == 13 and text.endswith(b"\n") and fields[0] == b"q" and fields[2] == b"ref" and fields[10] == b"*"
    pos, cigar, seq = int(fields[3]), fields[5].decode(), fields[9]
    assert fields[11].startswith(b"NM:i:") and fields[12].startswith(b"MD:Z:")
    nm, got_md = int(fields[11][5:]), fields[12][5:].decode()
    on_ref, on_read, edits = S.consumed(rec["runs"])
    assert pos == begin + 1 and len(seq) == on_read and rec["end"] - rec["begin"] == on_ref
    assert S.rebuild_reference(seq, cigar, got_md) == REFERENCE[pos - 1: pos - 1 + on_ref]
    assert nm == edits == sum(int(n) for n, op in re.findall(r"(\d+)([XID])", cigar))
    assert re.fullmatch(r"[0-9]+(([ACGTN]|\^[ACGTN]+)[0-9]+)*", got_md)
    assert md is None or got_md == md
    assert seq == rec["forward"] and (S.reverse_complement(rec["read"]) == seq if reverse else rec["read"] == seq)


def test_the_crafted_set_covers_what_it_names():
    assert REFERENCE[12] == ord("N") and S.craft(np.random.default_rng(5), REFERENCE, 8, [(10, "=")])["read"][4] == ord("N")
    assert CRAFTED["deletion at the end of the reference"][0] + 11 == len(REFERENCE)
    assert S.reverse_complement(b"ACGTNacgt") == b"NNNNNACGT"
    assert S.sam_runs("3=2I1X4D") == [(3, "="), (2, "D"), (1, "X"), (4, "I")]      # the window is the query: I and D trade places


# ---- 2. MAPQ ------------------------------------------------------------------------------------------------------------------------
def one_list(distances, keep=None):
    return -np.array(distances, np.int32), np.ones(len(distances), np.int32) if keep is None else np.array(keep, np.int32)


@pytest.mark.parametrize("n1, want", ((2, 3), (3, 2), (4, 1), (9, 1), (10, 0), (40, 0)))
def test_mapq_of_a_repeated_best_distance(n1, want):
    scores, keep = one_list([1] * n1 + [5])
    assert S.list_fields(scores, keep, 3) == (0, want, n1, 5) and B.list_mapq(1, n1, 5, 3) == want


@pytest.mark.parametrize("gap", range(8))
def test_mapq_of_a_unique_best_distance_follows_the_gap(gap):
    want = min(60, 10 * gap)
    assert S.list_fields(*one_list([2, 2 + gap] if gap else [2]), 1)[1] == want            # gap 0: only bound + 1 - d1 = 0 gives it
    assert B.list_mapq(2, 1, 2 + gap if gap else None, 1) == want
    assert S.list_fields(*one_list([3]), 2 + gap)[:2] == (0, want) and B.list_mapq(3, 1, -1, 2 + gap) == want     # from the bound alone


def test_mapq_without_a_bound_and_at_the_bound():
    assert S.list_fields(*one_list([4]), -1) == (0, 60, 1, -1) and B.list_mapq(4, 1, None, -1) == 60       # bound -1: gap 6
    assert S.list_fields(*one_list([4]), 4) == (0, 10, 1, -1) and B.list_mapq(4, 1, None, 4) == 10         # bound = d1: gap 1
    assert S.list_fields(*one_list([0, 1]), 4)[1] == 10                                                     # d2 goes before the bound
    assert S.list_fields(*one_list([7, 0, 3], keep=[0, 1, 1]), 5) == (1, 30, 1, 3)                          # the first KEPT slot
    assert S.list_fields(*one_list([1, 2], keep=[0, 0]), 5) == (-1, 0, 0, -1)                               # unmapped
    assert S.pair_fields(1, 1, 3, -1, 7, 8) == (60, 60) and S.pair_fields(1, 1, 3, 5, 7, 8) == (20, 20)
    assert S.pair_fields(1, 3, 3, 5, 7, 8) == (2, 2) and S.pair_fields(0, 0, 3, -1, 7, 8) == (7, 8)


def test_tlen_sign_and_the_tie_on_equal_begins():
    assert S.tlen_fields(100, 132, 200, 232) == (132, -132)
    assert S.tlen_fields(200, 232, 100, 132) == (-132, 132)
    assert S.tlen_fields(100, 132, 100, 140) == (40, -40)          # equal begins: end 1 positive
    assert S.tlen_fields(100, 180, 120, 150) == (80, -80)          # the rightmost END, whichever end has it


# ---- 3. check_sam_call ------------------------------------------------------------------------------------------------------------
def test_every_refusal_of_check_sam_call_has_its_text():
    lens = [4, 4, 3]
    good = dict(who="map_reads_sam", lens=lens, names=["a", "b", "c"], quals=[b"IIII", b"!~!~", b"III"], reference_name="chr1")
    rname, flat, offsets, rows = B.check_sam_call(**good)
    assert rname.tobytes() == b"chr1" and flat.tobytes() == b"abc" and offsets.tolist() == [0, 1, 2, 3] and rows.shape == (3, 4)
    for over, text in ((dict(reference_name=""), "reference_name is empty"), (dict(reference_name="chr 1"), "reference_name holds a tab, a space"),
                       (dict(reference_name=b"chr\t1"), "reference_name holds"), (dict(names=["a", "b"]), "2 names for 3 reads"),
                       (dict(names=["a", "", "c"]), "name of read 1 is empty"), (dict(names=[b"a", b"b", b"c d"]), "name of read 2 holds a tab, a space"),
                       (dict(names=["a\tb", "b", "c"]), "name of read 0 holds"), (dict(names=["a", "b\nc", "c"]), "name of read 1 holds"),
                       (dict(quals=[b"IIII", b"IIII"]), "2 QUAL strings for 3 reads"),
                       (dict(quals=[b"IIII", b"III", b"III"]), "QUAL of read 1 has 3 bytes, the read 4"),
                       (dict(quals=[b"IIII", b"IIII", b"I I"]), "QUAL of read 2 holds a byte outside"),
                       (dict(quals=np.full((3, 5), 73, np.uint8)), "QUAL of read 0 has 5 bytes, the read 4")):
        with pytest.raises(B.BgsaHipError, match=text):
            B.check_sam_call(**{**good, **over})
    _, flat, offsets, rows = B.check_sam_call("map_reads_sam", [5] * 12, None, None, "ref")
    assert flat.tobytes() == b"r0r1r2r3r4r5r6r7r8r9r10r11" and offsets[-3:].tolist() == [20, 23, 26] and rows is None


def bare_mapper():
    mapper = object.__new__(B.ReferenceMapper)      # no aligner, no reference on a device: touching either raises AttributeError
    mapper.ref_len, mapper.window_len, mapper.stride, mapper.both_strands = 3000, 96, 48, True
    mapper.n_windows = B.window_plan(3000, 96, 48)[0]
    mapper.n_ids, mapper.last_pair_stats, mapper.last_seed_stats = 2 * mapper.n_windows, None, None
    return mapper


def test_the_sam_entry_points_refuse_before_they_touch_a_device():
    mapper, reads = bare_mapper(), np.full((4, 32), ord("A"), np.uint8)
    for over, text in ((dict(names=["a"]), "1 names for 4 reads"), (dict(reference_name="a b"), "reference_name holds"),
                       (dict(quals=[b"II"] * 4), "QUAL of read 0 has 2 bytes"), (dict(max_distance=None), "max_distance is required"),
                       (dict(k_best=0), "k_best must lie"), (dict(reads=[b"ACGT", b""]), "empty"), (dict(cigar_cap=0), "cigar_cap")):
        with pytest.raises(B.BgsaHipError, match=text):
            mapper.map_reads_sam(**{**dict(reads=reads, max_distance=2), **over})
    for over, text in ((dict(names=["a", "b", "c", "d e"]), "name of read 3 holds"), (dict(quals1=reads + 1), "quals1 and quals2 come together"),
                       (dict(quals1=reads - 40, quals2=reads), "QUAL of read 0 holds a byte outside"), (dict(insert_min=0), "insert_min"),
                       (dict(rescue_distance=1), "below max_distance")):
        with pytest.raises(B.BgsaHipError, match=text):
            mapper.map_pairs_sam(**{**dict(reads1=reads, reads2=reads, insert_min=60, insert_max=200, max_distance=2), **over})
    assert mapper.last_pair_stats is None and mapper.last_seed_stats is None


def test_the_header_bytes(tmp_path):
    mapper = bare_mapper()
    assert mapper.sam_header() == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:ref\tLN:3000\n@PG\tID:bgsa-hip\n"
    assert mapper.sam_header("chr7") == b"@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chr7\tLN:3000\n@PG\tID:bgsa-hip\n"
    with pytest.raises(B.BgsaHipError, match="reference_name"):
        mapper.sam_header("chr 7")
    records = B.SamRecords(np.frombuffer(b"a\t4\n", np.uint8), np.array([0, 4]), *(np.zeros(1, np.int32),) * 4)
    B.write_sam(tmp_path / "out.sam", mapper.sam_header(), records)
    assert (tmp_path / "out.sam").read_bytes() == mapper.sam_header() + b"a\t4\n"


# ---- 4. the symbols and the C ABI's refusals ------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared and hasattr(flavour, name), (path.name, name)
    assert len(L.bgsa_hip_sam_mapq_dev.argtypes) == 10 and len(L.bgsa_hip_sam_measure_dev.argtypes) == 5
    assert len(L.bgsa_hip_sam_emit_dev.argtypes) == 7 and ctypes.sizeof(B.SamBatch) == 29 * 8
    assert B.SamRecords._fields == ("text", "offsets", "flag", "pos", "mapq", "nm")
    for name in ("map_reads_sam", "map_pairs_sam", "sam_header"):
        assert hasattr(B.ReferenceMapper, name)


def test_mapq_call_refusals(L):
    def call(scores=PTR, keep=PTR, ns=1, k=3, bound=2, outs=(PTR,) * 4):
        return L.bgsa_hip_sam_mapq_dev(scores, keep, ns, k, bound, *outs, None)
    assert call(scores=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error() and call(keep=None) == EINVAL
    for i in range(4):
        outs = [PTR] * 4
        outs[i] = None
        assert call(outs=tuple(outs)) == EINVAL
    for k in (0, -1, 65):
        assert call(k=k) == EINVAL and b"1..64" in L.bgsa_hip_last_error()
    assert call(bound=-2) == EINVAL and call(ns=-1) == EINVAL
    assert call(ns=0) == 0 and call(ns=0, k=64, bound=-1) == 0       # nothing to do: nothing is launched


def good_batch(**over):
    fields = {name: (PTR if kind is ctypes.c_void_p else 8) for name, kind in B.SamBatch._fields_}
    fields.update(over)
    return B.SamBatch(**fields)


def test_record_call_refusals(L):
    def measure(batch, n=1, lengths=PTR, malformed=PTR):
        return L.bgsa_hip_sam_measure_dev(batch, n, lengths, malformed, None)

    def emit(batch, n=1, offsets=PTR, text=PTR, text_bytes=100, malformed=PTR):
        return L.bgsa_hip_sam_emit_dev(batch, n, offsets, text, text_bytes, malformed, None)
    assert measure(None) == EINVAL and emit(None) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
    for name, kind in B.SamBatch._fields_:
        bad = good_batch(**{name: None if kind is ctypes.c_void_p else 0})
        if name == "d_quals":        # optional
            assert measure(bad, n=0) == 0 and emit(bad, n=0) == 0
        else:
            assert measure(bad) == EINVAL and emit(bad) == EINVAL, name
    assert measure(good_batch(read_stride=2 ** 31)) == EINVAL
    assert measure(good_batch(), lengths=None) == EINVAL and measure(good_batch(), malformed=None) == EINVAL
    assert emit(good_batch(), offsets=None) == EINVAL and emit(good_batch(), text=None) == EINVAL and emit(good_batch(), malformed=None) == EINVAL
    assert emit(good_batch(), text_bytes=-1) == EINVAL and measure(good_batch(), n=-1) == EINVAL and emit(good_batch(), n=-1) == EINVAL
    assert measure(good_batch(), n=0) == 0 and emit(good_batch(), n=0, text_bytes=0) == 0      # nothing to do: nothing is launched

"""The merge of many calls' BAM records without a GPU: the model (tests/bam_merge_reference.py) on a hand-made case and on the worked
example of INTEGRATION.md §3u, byte for byte; gather's window rule at every cut of one record; the host refusals of
check_bam_merge, of a call with merge= and of bgsa_hip_bam_gather_dev, each before any launch; the declarations."""
import re
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bam_merge_reference as G  # noqa: E402
import bam_reference as M  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
REF_NAMES, REF_LENS = [b"chrT"], [1000]


def record(name: bytes, pos: int, flag: int, seq: bytes = b"AC", mapq: int = 30) -> bytes:
    """A BAM record without QUAL and tags: mapped at `pos` with one '=' run over its bases, or (flag & 4) without coordinates."""
    mapped = not flag & 4
    cigar = struct.pack("<I", len(seq) << 4 | 7) if mapped else b""
    ref_id, pos = (0, pos) if mapped else (-1, -1)
    body = struct.pack("<iiBBHHHIiii", ref_id, pos, len(name) + 1, mapq if mapped else 0, M.reg2bin(pos, pos + len(seq)) if mapped else 4680,
                       len(cigar) // 4, flag, len(seq), -1, -1, 0)
    body += name + b"\x00" + cigar + M.pack_seq(seq) + b"\xff" * len(seq)
    return struct.pack("<i", len(body)) + body


def worked_example() -> list:
    """§3u's: two batches of two records; `c` repeats `b` in a LATER batch, `d` has no coordinates."""
    return [[record(b"a", 300, 0), record(b"b", 100, 0)], [record(b"c", 100, 0), record(b"d", 0, 4)]]


# ---- 1. the model -----------------------------------------------------------------------------------------------------------------------
def test_the_worked_example_of_the_integration_guide_byte_for_byte():
    batches = worked_example()
    P, segment_blocks = 32, 2
    got = G.merged(batches, P, None, REF_LENS, REF_NAMES, mark_duplicates=True)
    assert [len(x) for batch in batches for x in batch] == [45, 45, 45, 41]
    assert got["order"] == [1, 2, 0, 3]                       # b, c (a tie: input order), a, then the record without coordinates
    assert got["offsets"] == [0, 45, 90, 135, 176]
    assert got["flag"] == [0, 0x400, 0, 4] and got["ref_id"] == [0, 0, 0, -1]
    assert got["stats"] == dict(pair_units=0, fragment_units=3, duplicate_pair_units=0, duplicate_fragment_units=1, records_flagged=1,
                                records_skipped=0)
    source = batches[1][0]
    assert got["records"][1] == source[:18] + b"\x00\x04" + source[20:] and source[18:20] == b"\x00\x00"
    assert [got["records"][i] for i in (0, 2, 3)] == [batches[0][1], batches[0][0], batches[1][1]]      # the others byte for byte
    span = P * segment_blocks                                 # 64: c's byte 18 is the last of segment 0, its byte 19 the first of segment 1
    assert got["offsets"][1] + 18 == span - 1
    payload = b"".join(got["records"])
    src = b"".join(x for batch in batches for x in batch)
    flags = [0, 0, 0x400, 4]                                  # in INPUT order
    pieces = []
    for lo in range(0, len(payload), span):
        hi = min(lo + span, len(payload))
        written, bad = G.gather(src, [0, 45, 90, 135, 176], got["order"], got["offsets"], 0, 4, lo, hi, flags)
        assert bad == 0 and sorted(written) == list(range(lo, hi))
        pieces.append(bytes(written[p] for p in range(lo, hi)))
    assert b"".join(pieces) == payload and len(pieces) == 3
    assert pieces[0][-1] == 0x00 and pieces[1][0] == 0x04
    chunks = got["index"]["chunks"]                           # b, c and a share bin 4681: one chunk from offset 0 to a's end
    assert chunks == [(0, 4681, 0, (135 // P * (P + 31)) << 16 | 135 % P)] and got["index"]["n_intv"] == [1]
    text = (ROOT / "INTEGRATION.md").read_text()
    section = text[text.index("## 3u."):]
    for what in (source.hex(), got["records"][1].hex(), "order = [1, 2, 0, 3]", "dst_offsets = [0, 45, 90, 135, 176]", "flag = [0, 0, 1024, 4]"):
        assert what in section, what


def test_the_model_on_a_hand_made_case():
    """Pairs in two batches: the second batch repeats the first one's pair; both of its records get bit 1024, nothing else moves."""
    def pair(name, pos1, pos2):
        one = bytearray(record(name, pos1, 1 + 2 + 32 + 64))
        two = bytearray(record(name, pos2, 1 + 2 + 16 + 128))
        for rec, mate in ((one, pos2), (two, pos1)):
            struct.pack_into("<ii", rec, 24, 0, mate)             # next_refID, next_pos
        return [bytes(one), bytes(two)]
    batches = [pair(b"p0", 200, 260) + pair(b"p1", 50, 90), pair(b"p2", 200, 260)]
    plain = G.merged(batches, 61, None, REF_LENS, REF_NAMES, paired=True)
    got = G.merged(batches, 61, None, REF_LENS, REF_NAMES, mark_duplicates=True, paired=True)
    assert plain["order"] == got["order"] == [2, 3, 0, 4, 1, 5] and plain["offsets"] == got["offsets"]
    assert plain["stats"] is None and plain["flag"] == [G.flag_of(batches[i // 4][i % 4]) for i in got["order"]]
    assert [g ^ p for g, p in zip(got["flag"], plain["flag"])] == [0, 0, 0, 1024, 0, 1024]
    assert got["stats"]["pair_units"] == 3 and got["stats"]["duplicate_pair_units"] == 1 and got["stats"]["records_flagged"] == 2
    assert got["index"] == plain["index"]                     # the index does not read bit 1024
    starts = [0, 40, 95, 130, 170, 200, 260]                  # made-up deflated blocks: the offsets move, the records do not
    packed = G.merged(batches, 61, starts, REF_LENS, REF_NAMES, mark_duplicates=True, paired=True)
    assert packed["records"] == got["records"] and packed["index"]["voff_beg"][1] == starts[got["offsets"][1] // 61] << 16 | got["offsets"][1] % 61


# ---- 2. gather's window rule -------------------------------------------------------------------------------------------------------------
def test_every_cut_through_one_record():
    rec = bytes(range(100, 140))                              # 40 bytes, every one different
    front, back = bytes(27), bytes(25)
    src, src_offsets = front + rec + back, [0, 27, 67, 92]
    order, dst_offsets = [2, 1, 0], [0, 25, 65, 92]           # the record moves from 27 to 25
    flag = [0, 0xBEEF, 0]
    want = bytearray(back + rec + front)
    want[25 + 18: 25 + 20] = b"\xef\xbe"
    for cut in range(25, 66):                                 # every cut position, between bytes 18 and 19 included
        low, bad_low = G.gather(src, src_offsets, order, dst_offsets, 0, 3, 0, cut, flag)
        high, bad_high = G.gather(src, src_offsets, order, dst_offsets, 0, 3, cut, 92, flag)
        assert bad_low == bad_high == 0
        assert sorted(low) == list(range(cut)) and sorted(high) == list(range(cut, 92))       # no byte twice, none missing
        assert bytes({**low, **high}[p] for p in range(92)) == bytes(want), cut
    low, _ = G.gather(src, src_offsets, order, dst_offsets, 0, 3, 0, 25 + 19, flag)
    assert low[25 + 18] == 0xef and 25 + 19 not in low
    only, _ = G.gather(src, src_offsets, order, dst_offsets, 1, 1, 0, 92, None)                # one record, the source's own flag bytes
    assert bytes(only[p] for p in sorted(only)) == rec and sorted(only) == list(range(25, 65))
    assert G.gather(src, src_offsets, order, dst_offsets, 0, 0, 0, 92, flag) == ({}, 0)
    assert G.gather(src, src_offsets, order, dst_offsets, 0, 3, 29, 29, flag) == ({}, 0)


def test_the_model_refuses_per_record():
    src, src_offsets = bytes(100), [0, 30, 60, 90]
    good = dict(order=[0, 1, 2], dst_offsets=[0, 30, 60, 90])
    assert G.gather(src, src_offsets, good["order"], good["dst_offsets"], 0, 3, 0, 90, [0] * 3)[1] == 0
    for what, order, s_off, d_off in (("order = n_src", [0, 3, 2], src_offsets, good["dst_offsets"]),
                                      ("order < 0", [0, -1, 2], src_offsets, good["dst_offsets"]),
                                      ("the lengths differ", good["order"], src_offsets, [0, 30, 61, 91]),
                                      ("the source leaves src", good["order"], [0, 30, 101, 131], [0, 30, 101, 131]),
                                      ("a source pair that is not monotone", good["order"], [0, 30, 20, 50], good["dst_offsets"]),
                                      ("a destination pair that is not monotone", good["order"], src_offsets, [0, 30, 20, 50]),
                                      ("a negative offset", [1, 0, 2], [-30, 0, 30, 60], good["dst_offsets"])):
        written, bad = G.gather(src, s_off, order, d_off, 0, 2, 0, 200, None)      # output records 0 and 1: record 1 is the bad one
        assert bad == 1 and sorted(written) == list(range(30)), what
    short = G.gather(bytes(60), [0, 19, 39, 59], [0, 1, 2], [0, 19, 39, 59], 0, 3, 0, 59, [0] * 3)
    assert short[1] == 1 and sorted(short[0]) == list(range(19, 59))                           # length 19 with a flag: refused, not a byte
    assert G.gather(bytes(60), [0, 19, 39, 59], [0, 1, 2], [0, 19, 39, 59], 0, 3, 0, 59, None)[1] == 0


# ---- 3. the host refusals ----------------------------------------------------------------------------------------------------------------
class Mapper:
    """What a BamMerge asks of its mapper before the first batch."""

    def __init__(self, ref_lens=(1000,)):
        self.ref_lens = ref_lens

    def index_ref_lens(self):
        return np.asarray(self.ref_lens, dtype=np.int64)


def test_check_bam_merge_refuses_before_anything_is_allocated():
    B.check_bam_merge("bam_merge")
    B.check_bam_merge("bam_merge", 1, True, True, 1, 0, [2 ** 29])
    B.check_bam_merge("bam_merge", np.int64(61), np.bool_(False), False, np.int32(3), np.int64(10))
    for kwargs, message in ((dict(compress=1), "bam_merge: rc=-1: compress 1 is not a bool"),
                            (dict(mark_duplicates="yes"), "bam_merge: rc=-1: mark_duplicates 'yes' is not a bool"),
                            (dict(block_payload=0), "bam_merge: rc=-1: block_payload 0 outside 1..65280"),
                            (dict(block_payload=65281), "bam_merge: rc=-1: block_payload 65281 outside 1..65280"),
                            (dict(block_payload=True), "bam_merge: rc=-1: block_payload True outside 1..65280"),
                            (dict(block_payload=61.0), "bam_merge: rc=-1: block_payload 61.0 outside 1..65280"),
                            (dict(segment_blocks=0), "bam_merge: rc=-1: segment_blocks 0 is not an int >= 1"),
                            (dict(segment_blocks=2.0), "bam_merge: rc=-1: segment_blocks 2.0 is not an int >= 1"),
                            (dict(segment_blocks=True), "bam_merge: rc=-1: segment_blocks True is not an int >= 1"),
                            (dict(reserve_bytes=-1), "bam_merge: rc=-1: reserve_bytes -1 is neither None nor an int >= 0"),
                            (dict(reserve_bytes=1.5), "bam_merge: rc=-1: reserve_bytes 1.5 is neither None nor an int >= 0"),
                            (dict(ref_lens=[5, 2 ** 29 + 1]), "bam_merge: rc=-1: reference 1 has 536870913 bases, a BAI index reaches 2^29")):
        with pytest.raises(B.BgsaHipError, match=re.escape(message)):
            B.check_bam_merge("bam_merge", **kwargs)
    with pytest.raises(B.BgsaHipError, match="reference 0 has 536870913 bases"):
        B.BamMerge(Mapper([2 ** 29 + 1]))
    merge = B.BamMerge(Mapper(), 61, True, True, 3, 100)
    assert (merge.block_payload, merge.compress, merge.mark_duplicates, merge.segment_blocks, merge.reserve_bytes) == (61, True, True, 3, 100)
    assert (merge.n, merge.payload_bytes, merge.ends, merge.finished, merge.payload) == (0, 0, None, False, None)      # nothing allocated


def test_a_call_with_a_merge_refuses_before_any_launch():
    mapper = Mapper()
    merge = B.BamMerge(mapper)
    B.check_bam_merge_add("map_reads_bam", merge, mapper, 1)
    B.check_bam_merge_add("map_pairs_bam", merge, mapper, 2)      # a merge without a batch takes either kind
    for kwargs, message in ((dict(sort=True), "map_reads_bam: rc=-1: sort beside merge=: they belong to the merge"),
                            (dict(compress=True), "map_reads_bam: rc=-1: compress beside merge="),
                            (dict(block_payload=61), "map_reads_bam: rc=-1: block_payload beside merge="),
                            (dict(mark_duplicates=True), "map_reads_bam: rc=-1: mark_duplicates beside merge="),
                            (dict(sort=True, block_payload=61), "map_reads_bam: rc=-1: sort, block_payload beside merge=")):
        with pytest.raises(B.BgsaHipError, match=re.escape(message)):
            B.check_bam_merge_add("map_reads_bam", merge, mapper, 1, **kwargs)
    with pytest.raises(B.BgsaHipError, match="map_reads_bam: rc=-1: merge 'm' is not a BamMerge"):
        B.check_bam_merge_add("map_reads_bam", "m", mapper, 1)
    with pytest.raises(B.BgsaHipError, match="map_pairs_bam: rc=-1: the merge belongs to another mapper"):
        B.check_bam_merge_add("map_pairs_bam", merge, Mapper(), 2)
    merge.ends = 1
    B.check_bam_merge_add("map_reads_bam", merge, mapper, 1)
    with pytest.raises(B.BgsaHipError, match="map_pairs_bam: rc=-1: a paired batch into a merge of single-end ones"):
        B.check_bam_merge_add("map_pairs_bam", merge, mapper, 2)
    merge.ends = 2
    with pytest.raises(B.BgsaHipError, match="map_reads_bam: rc=-1: a single-end batch into a merge of paired ones"):
        B.check_bam_merge_add("map_reads_bam", merge, mapper, 1)
    merge.finished = True
    with pytest.raises(B.BgsaHipError, match="map_pairs_bam: rc=-1: the merge is finished"):
        B.check_bam_merge_add("map_pairs_bam", merge, mapper, 2)
    with pytest.raises(B.BgsaHipError, match=re.escape("bam_merge.write: rc=-1: the header's @HD line does not say SO:coordinate")):
        B.BamMerge(mapper).write("never-opened.bam", M.encode_header(b"@HD\tVN:1.6\tSO:unsorted\n", [(b"chrT", 1000)]))
    assert not Path("never-opened.bam").exists()


def test_the_gather_call_refuses_bad_arguments_before_any_launch():
    L = B.lib()
    names = ("src", "src_bytes", "src_offsets", "n_src", "order", "dst_offsets", "n", "first", "count", "lo", "hi", "flag", "out", "refused", "stream")
    ok = [1, 100, 1, 4, 1, 1, 4, 0, 4, 0, 100, None, 1, 1, None]      # pointers that are never read: every call below is refused first

    def gather(**over):
        return L.bgsa_hip_bam_gather_dev(*[over.get(name, value) for name, value in zip(names, ok)])
    for bad in (dict(src=None), dict(src_offsets=None), dict(order=None), dict(dst_offsets=None), dict(out=None), dict(refused=None),
                dict(src_bytes=-1), dict(n_src=-1), dict(n=-1), dict(first=-1), dict(count=-1), dict(first=1), dict(count=5), dict(first=5, count=0),
                dict(first=2 ** 62, count=2 ** 62), dict(lo=10, hi=9), dict(lo=0, hi=-1)):
        assert gather(**bad) == -1 and b"bam_gather_dev" in L.bgsa_hip_last_error(), bad
    assert gather(count=0) == 0 and gather(first=4, count=0) == 0      # nothing to do, nothing launched
    assert gather(lo=7, hi=7) == 0 and gather(lo=7, hi=7, flag=1) == 0      # an empty window


# ---- 4. the declarations -----------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_listed_and_built():
    header = (ROOT / "include" / "bgsa_hip.h").read_text()
    assert "BAM records: merge" in header and re.search(r"\nint bgsa_hip_bam_gather_dev\(const uint8_t \*d_src, int64_t src_bytes,", header)
    assert '("bgsa_hip_bam_gather_dev", [' in (ROOT / "bgsa_amd" / "__init__.py").read_text()
    assert "bam_merge.hip" in re.search(r"^SRCS\s*:=(.*)$", (ROOT / "bgsa_amd" / "csrc" / "Makefile").read_text(), re.M).group(1).split()
    call = B.lib().bgsa_hip_bam_gather_dev
    assert len(call.argtypes) == 15 and call.restype is not None
    for name in ("BamMerge", "check_bam_merge", "check_bam_merge_add"):
        assert hasattr(B, name), name

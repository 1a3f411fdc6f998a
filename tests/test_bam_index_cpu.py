"""Coordinate order and the BAI index without a GPU: the host model tests/bai_reference.py against brute force — its region
queries find exactly the records that overlap —, bgsa_amd.bai_bytes against the model byte for byte, the worked example of
INTEGRATION.md §3s, the refusals of sort, sort_order and write_bam(index=True), and the host-only window table of the library."""
import struct
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bai_reference as R  # noqa: E402
import bam_reference as M  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
REF_LENS = (70_000_000, 40_000, 100)
BOUNDARIES = (2 ** 14, 2 ** 17, 2 ** 20, 2 ** 23, 2 ** 26)
PAYLOADS = (61, 256, 65280)


def synthetic(seed: int = 29, n: int = 2000) -> dict:
    """About n records on three references, sorted by the model's key (stable): positions planted on both sides of every level's
    boundary, lengths 1..40,000, unmapped ends beside a mate, records without coordinates, fake record byte lengths >= 8."""
    rng = np.random.default_rng(seed)
    rows = []
    for boundary in BOUNDARIES:
        for pos, length in ((boundary - 1, 1), (boundary, 1), (boundary - 1, 2), (boundary - 40, 40), (boundary - 40, 41), (boundary - 7, 40_000),
                            (boundary + 5, 3), (boundary - 16_384, 16_384), (boundary - 16_385, 16_386)):
            rows.append((0, max(pos, 0), pos + length, int(rng.integers(2)) * 16))
    for _ in range(n - len(rows) - 260):
        ref = int(rng.choice(3, p=(0.6, 0.3, 0.1)))
        length = int(rng.choice((1, 2, 35, 150, 1000, 40_000))) if rng.random() < 0.5 else int(rng.integers(1, 40_001))
        length = min(length, REF_LENS[ref])
        pos = int(rng.integers(0, REF_LENS[ref] - length + 1))
        if ref == 0 and rng.random() < 0.5:                 # most of them close together: chunks of more than one record
            pos = int(rng.integers(0, 200_000 - length)) if length < 200_000 else pos
        rows.append((ref, pos, pos + length, int(rng.integers(2)) * 16))
    for _ in range(200):                                    # unmapped ends that borrow a place
        ref = int(rng.integers(3))
        pos = int(rng.integers(0, REF_LENS[ref]))
        rows.append((ref, pos, pos + 1, 4 + 64))
    rows += [(-1, -1, 0, 4)] * 60
    rows = [rows[i] for i in rng.permutation(len(rows))]
    rows.sort(key=lambda x: R.sort_key(x[0], x[1], x[3]))   # stable
    ref_id, pos, end, flag = (np.array(x) for x in zip(*rows))
    bins = np.array([4680 if p < 0 else M.reg2bin(int(p), int(e)) for p, e in zip(pos, end)])
    lengths = rng.integers(8, 300, size=len(rows))
    lengths[:: 97] = 8
    return dict(ref_id=ref_id, pos=pos, end=end, bin=bins, flag=flag, offsets=np.concatenate(([0], np.cumsum(lengths))).astype(np.int64))


def fake_payload(offsets) -> bytes:
    """Records of the given byte lengths: block_size, the record's index, filler."""
    out = []
    for i in range(len(offsets) - 1):
        size = int(offsets[i + 1] - offsets[i])
        out.append(struct.pack("<ii", size - 4, i) + bytes([i % 251]) * (size - 8))
    return b"".join(out)


def deflated(payload: bytes, P: int) -> tuple:
    """(BGZF blocks with zlib's deflate, their n_blocks + 1 byte offsets)."""
    out, offsets = [], [0]
    for at in range(0, len(payload), P):
        piece = payload[at: at + P]
        packer = zlib.compressobj(6, zlib.DEFLATED, -15)
        body = packer.compress(piece) + packer.flush()
        out.append(bytes.fromhex("1f8b08040000000000ff0600") + b"BC\x02\x00" + struct.pack("<H", len(body) + 25) + body +
                   struct.pack("<II", zlib.crc32(piece), len(piece)))
        offsets.append(offsets[-1] + len(out[-1]))
    return b"".join(out), offsets


def regions() -> list:
    out = [(0, 0, REF_LENS[0]), (1, 0, REF_LENS[1]), (2, 0, REF_LENS[2]), (2, 99, 100), (1, 39_999, 40_000),
           (0, 69_000_000, 69_000_001), (0, 30_000_000, 30_000_500),       # stretches that may well be empty
           (0, REF_LENS[0] - 1, REF_LENS[0]), (1, 32_768, 40_000), (0, 100_000, 180_000)]
    for boundary in BOUNDARIES:
        out += [(0, boundary - 1, boundary), (0, boundary, boundary + 1), (0, boundary - 1, boundary + 1)]
    return out


@pytest.fixture(scope="module")
def records():
    return synthetic()


@pytest.mark.parametrize("P", PAYLOADS)
@pytest.mark.parametrize("deflate", (False, True))
def test_region_queries_return_exactly_the_records_that_overlap(records, P, deflate):
    s = records
    payload = fake_payload(s["offsets"])
    blocks, block_offsets = deflated(payload, P) if deflate else (M.frame(payload, P), None)
    header = b"not a BAM header, only bytes in front of the blocks" * 3
    base = len(B.bgzf_blocks(header))
    file_bytes = B.bgzf_blocks(header) + blocks + B.BGZF_EOF
    index = R.build_index(s["ref_id"], s["pos"], s["end"], s["bin"], s["offsets"], P, block_offsets, REF_LENS)
    parsed = R.parse_bai(R.bai_bytes(index, s["flag"], s["ref_id"], base))
    placed = int((s["ref_id"] >= 0).sum())
    everything = [pair for one in parsed["refs"] for pairs in one["bins"].values() for pair in pairs]
    reached = sorted(struct.unpack_from("<i", x, 4)[0] for x in R.fetch(file_bytes, sorted(everything)))
    assert reached == list(range(placed))                   # every placed record lies in exactly one chunk
    assert parsed["n_no_coor"] == len(s["ref_id"]) - placed == 60
    found_some = 0
    for ref, beg, end in regions():
        got = R.fetch(file_bytes, R.query(parsed, ref, beg, end))
        ids = [struct.unpack_from("<i", x, 4)[0] for x in got]
        assert len(set(ids)) == len(ids), (ref, beg, end)
        want = R.overlaps(s["ref_id"], s["pos"], s["end"], ref, beg, end)
        hit = [i for i in ids if s["ref_id"][i] == ref and s["pos"][i] < end and s["end"][i] > beg]
        assert sorted(hit) == want, (P, ref, beg, end)
        found_some += bool(want)
    assert found_some >= 20
    beyond = R.query(parsed, 1, 39_000, 40_000)             # a region in the last window, and one past every window of a short reference
    assert isinstance(beyond, list) and R.query(parsed, 2, 16_384, 16_500) == []
    for c, one in enumerate(parsed["refs"]):
        mine = s["ref_id"] == c
        assert one["meta"][1] == (int((mine & (s["flag"] & 4 == 0)).sum()), int((mine & (s["flag"] & 4 != 0)).sum()))
        assert one["meta"][0] == (min(index["voff_beg"][i] for i in np.flatnonzero(mine)) + (base << 16),
                                  max(index["voff_end"][i] for i in np.flatnonzero(mine)) + (base << 16))
        assert len(one["linear"]) == max(int(e - 1) >> 14 for e in s["end"][mine]) + 1
        assert all(a <= b for a, b in zip(one["linear"], one["linear"][1:]))


def as_bam_index(index: dict) -> B.BamIndex:
    chunks = index["chunks"]
    return B.BamIndex(np.array(index["ref_lens"], np.int64), np.array([x[0] for x in chunks], np.int32), np.array([x[1] for x in chunks], np.int32),
                      np.array([x[2] for x in chunks], np.int64), np.array([x[3] for x in chunks], np.int64), np.array(index["window_base"], np.int64),
                      np.array(index["linear"], np.int64), np.array(index["n_intv"], np.int64))


@pytest.mark.parametrize("P", PAYLOADS)
def test_bai_bytes_equal_the_model_and_parse_back(records, P):
    s = records
    index = R.build_index(s["ref_id"], s["pos"], s["end"], s["bin"], s["offsets"], P, None, REF_LENS)
    plain = B.bai_bytes(as_bam_index(index), s["flag"], s["ref_id"], 0)
    assert plain == R.bai_bytes(index, s["flag"], s["ref_id"], 0)
    base = 1234
    moved = B.bai_bytes(as_bam_index(index), s["flag"], s["ref_id"], base)
    assert moved == R.bai_bytes(index, s["flag"], s["ref_id"], base) and len(moved) == len(plain)
    a, b = R.parse_bai(plain), R.parse_bai(moved)
    shift = base << 16
    for one, other in zip(a["refs"], b["refs"]):
        assert list(one["bins"]) == list(other["bins"]) == sorted(one["bins"])
        for k in one["bins"]:
            assert [(lo + shift, hi + shift) for lo, hi in one["bins"][k]] == other["bins"][k]
        assert [v + shift for v in one["linear"]] == other["linear"]
        assert other["meta"] == ((one["meta"][0][0] + shift, one["meta"][0][1] + shift), one["meta"][1])
    assert a["n_no_coor"] == b["n_no_coor"] == 60
    chunks = [(c, k, lo, hi) for c, one in enumerate(a["refs"]) for k, pairs in one["bins"].items() for lo, hi in pairs]
    assert chunks == index["chunks"]                        # the round trip loses nothing
    assert R.bai_bytes(R.build_index([], [], [], [], [0], P, None, REF_LENS), [], [], 7) == \
        b"BAI\x01" + struct.pack("<i", 3) + struct.pack("<ii", 0, 0) * 3 + struct.pack("<Q", 0)
    empty = as_bam_index(R.build_index([], [], [], [], [0], P, None, REF_LENS))
    assert B.bai_bytes(empty, np.zeros(0, np.int32), np.zeros(0, np.int32), 7) == R.bai_bytes(R.build_index([], [], [], [], [0], P, None, REF_LENS), [], [], 7)


# the worked example of INTEGRATION.md §3s: one reference of 40,000 bp, three records of 100, 100 and 60 bytes in input order
EXAMPLE_BAI = ("4241490101000000030000004912000001000000000000000000000064000000000000004a120000010000006400000000000000c8000000000000004a92"
               "0000020000000000000000000000c8000000000000000200000000000000000000000000000002000000000000000000000064000000000000000100"
               "000000000000")


def test_the_worked_example_of_the_integration_guide():
    recs = [dict(strand=0, begin=20_000, end=20_100, flag=0, rnext=0, pnext=0), dict(strand=1, begin=100, end=200, flag=16, rnext=0, pnext=0),
            dict(strand=-1, begin=-1, end=-1, flag=4, rnext=0, pnext=0)]
    coords = [R.coordinates(r, 40_000) for r in recs]
    assert [c[0] for c in coords] == [40_002, 203, 0x7fffffff << 32]
    assert coords == [(40_002, 0, 20_000, 20_100, 4682), (203, 0, 100, 200, 4681), (0x7fffffff << 32, -1, -1, 0, 4680)]
    order = sorted(range(3), key=lambda i: coords[i][0])
    assert order == [1, 0, 2]
    lengths = [100, 100, 60]
    offsets = np.concatenate(([0], np.cumsum([lengths[i] for i in order])))
    _, ref_id, pos, end, bins = zip(*(coords[i] for i in order))
    index = R.build_index(ref_id, pos, end, bins, offsets, 65280, None, [40_000])
    assert index["chunks"] == [(0, 4681, 0, 100), (0, 4682, 100, 200)] and index["linear"][:2] == [0, 100] and index["n_intv"] == [2]
    flag = [recs[i]["flag"] for i in order]
    data = R.bai_bytes(index, flag, ref_id, 0)
    assert data.hex() == EXAMPLE_BAI and len(data) == 128
    assert B.bai_bytes(as_bam_index(index), np.array(flag), np.array(ref_id), 0) == data
    guide = (ROOT / "INTEGRATION.md").read_text()
    assert "§3s" in guide and EXAMPLE_BAI in guide.replace("\n", "").replace("#", "").replace(" ", "")


class FakeMapper(B.ContigMapper):
    """A ContigMapper's header methods without a device: only the names and the lengths."""

    def __init__(self, names, lens):
        self.contig_names, self.contig_lens = [n.encode() for n in names], np.array(lens, np.int64)


def test_refusals_of_sort_sort_order_and_an_indexed_file(tmp_path):
    good = dict(who="t", lens=np.array([30, 30]), names=None, quals=None, reference_name="ref")
    assert len(B.check_bam_call(**good, sort=True, ref_lens=[2 ** 29, 5])) == 4 and len(B.check_bam_call(**good, sort=False, ref_lens=[2 ** 29 + 1])) == 4
    for bad in (1, 0, "yes", None):
        with pytest.raises(B.BgsaHipError, match="sort .* is not a bool"):
            B.check_bam_call(**good, sort=bad)
    with pytest.raises(B.BgsaHipError, match="reference 1 has 536870913 bases"):
        B.check_bam_call(**good, sort=True, ref_lens=[7, 2 ** 29 + 1])
    mapper = FakeMapper(["a", "b"], [50, 60])
    assert mapper.sam_header() == mapper.sam_header(sort_order="unsorted") and b"SO:unsorted" in mapper.sam_header()
    assert mapper.sam_header(sort_order="coordinate") == mapper.sam_header().replace(b"SO:unsorted", b"SO:coordinate")
    assert M.decode_header(mapper.bam_header(sort_order="coordinate"))[0] == mapper.sam_header(sort_order="coordinate")
    for bad in ("queryname", "", None, b"coordinate", "Coordinate"):
        for call in (mapper.sam_header, mapper.bam_header, lambda sort_order: B.ReferenceMapper.sam_header(mapper, "r", sort_order)):
            with pytest.raises(B.BgsaHipError, match="neither 'unsorted' nor 'coordinate'"):
                call(sort_order=bad)
    s = synthetic(n=400)
    index = as_bam_index(R.build_index(s["ref_id"], s["pos"], s["end"], s["bin"], s["offsets"], 256, None, REF_LENS))
    blocks = np.frombuffer(M.frame(fake_payload(s["offsets"]), 256), np.uint8)
    columns = (s["flag"].astype(np.int32), s["pos"].astype(np.int64) + 1, np.zeros(len(s["flag"]), np.int32), np.zeros(len(s["flag"]), np.int32))
    plain = B.BamRecords(blocks, s["offsets"], *columns)
    sorted_records = B.SortedBamRecords(blocks, s["offsets"], *columns, s["ref_id"].astype(np.int32), np.arange(len(s["flag"])), index)
    sorted_header, unsorted_header = mapper.bam_header(sort_order="coordinate"), mapper.bam_header()
    for records, header in ((plain, sorted_header), ([sorted_records], sorted_header), ((sorted_records, sorted_records), sorted_header),
                            (sorted_records, unsorted_header)):
        with pytest.raises(B.BgsaHipError, match="ONE SortedBamRecords|SO:coordinate"):
            B.write_bam(tmp_path / "no.bam", header, records, index=True)
        assert not (tmp_path / "no.bam").exists() and not (tmp_path / "no.bam.bai").exists()
    B.write_bam(tmp_path / "yes.bam", sorted_header, sorted_records, index=True)
    base = len(B.bgzf_blocks(sorted_header))
    assert (tmp_path / "yes.bam.bai").read_bytes() == B.bai_bytes(index, s["flag"], s["ref_id"], base)
    assert (tmp_path / "yes.bam").read_bytes() == B.bgzf_blocks(sorted_header) + blocks.tobytes() + B.BGZF_EOF
    B.write_bam(tmp_path / "plain.bam", unsorted_header, (plain, sorted_records))        # without an index a sorted batch is a batch
    assert not (tmp_path / "plain.bam.bai").exists()


def test_the_window_table_of_the_library():
    L = B.lib()
    lens = np.array(REF_LENS + (16_384, 16_385, 1, 2 ** 29), np.int64)
    base = np.full(lens.size + 2, -7, np.int64)
    total = L.bgsa_hip_bam_index_windows(lens.ctypes.data, lens.size, base.ctypes.data)
    assert base[: lens.size + 1].tolist() == R.windows(lens) and total == base[lens.size] and base[-1] == -7
    assert R.windows(lens)[-1] == 4273 + 3 + 1 + 1 + 2 + 1 + 32_768
    for bad in (0, -1, 2 ** 29 + 1):
        assert L.bgsa_hip_bam_index_windows(np.array([5, bad], np.int64).ctypes.data, 2, base.ctypes.data) == -1
    assert L.bgsa_hip_bam_index_windows(None, 1, base.ctypes.data) == -1 and L.bgsa_hip_bam_index_windows(lens.ctypes.data, -1, base.ctypes.data) == -1
    assert L.bgsa_hip_bam_index_windows(lens.ctypes.data, 0, base.ctypes.data) == 0 and base[0] == 0


def test_the_index_calls_refuse_bad_arguments_before_any_launch():
    L = B.lib()
    ok = [1] * 4 + [1, 1, 10, 256, None, 1, 1, 1] + [1] * 5 + [None]      # pointers that are never read: every call below is refused first

    def marks(**over):
        names = ("ref_id", "pos", "end", "bin", "n", "offsets", "payload_bytes", "P", "block_offsets", "n_blocks", "window_base", "n_refs",
                 "voff_beg", "voff_end", "chunk_start", "linear", "refused", "stream")
        return L.bgsa_hip_bam_index_marks_dev(*[over.get(name, value) for name, value in zip(names, ok)])
    for bad in (dict(ref_id=None), dict(offsets=None), dict(window_base=None), dict(linear=None), dict(refused=None), dict(n=-1), dict(P=0),
                dict(P=65281), dict(payload_bytes=-1), dict(n_blocks=-1), dict(n_refs=-1)):
        assert marks(**bad) == -1 and b"bam_index_marks_dev" in L.bgsa_hip_last_error(), bad
    assert marks(n=0) == 0                                  # nothing to do, nothing launched
    assert L.bgsa_hip_bam_index_chunks_dev(*[1] * 6, -1, 0, *[1] * 5, None) == -1 and L.bgsa_hip_bam_index_chunks_dev(*[1] * 6, 1, -1, *[1] * 5, None) == -1
    assert L.bgsa_hip_bam_index_chunks_dev(*[1] * 5, None, 1, 0, *[1] * 5, None) == -1 and L.bgsa_hip_bam_index_chunks_dev(*[1] * 6, 0, 0, *[1] * 5, None) == 0
    assert L.bgsa_hip_bam_coordinates_dev(None, 1, *[1] * 6, None) == -1

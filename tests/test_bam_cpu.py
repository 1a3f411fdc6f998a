"""BAM records and BGZF framing, without a GPU: the host model checks itself (encoder -> decoder, reg2bin against the definition, the
sliced CRC against zlib), bgzf_blocks against gzip and the block walker, the six new symbols — declared, exported by both
flavours, prototyped, refusing bad arguments before any HIP call —, and check_bam_call, bam_header and write_bam."""
import ctypes
import gzip
import struct
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import bgsa_amd as B  # noqa: E402
import bam_reference as M  # noqa: E402
import sam_reference as S  # noqa: E402
import test_sam_cpu as SC  # noqa: E402

EINVAL = -1
PTR = 0x10000   # a non-null "device pointer": every call below must return before it is looked at
SYMBOLS = ("bgsa_hip_bam_measure_dev", "bgsa_hip_bam_emit_dev", "bgsa_hip_bam_measure_contigs_dev", "bgsa_hip_bam_emit_contigs_dev",
           "bgsa_hip_bgzf_framed_bytes", "bgsa_hip_bgzf_frame_dev")
PAYLOADS = (1, 61, 256, 65280)


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- 1. the model checks itself -------------------------------------------------------------------------------------------------
def crafted(name: str, reverse: bool, **over) -> dict:
    begin, runs, _ = SC.CRAFTED[name]
    rec = S.craft(np.random.default_rng(5), SC.REFERENCE, begin, runs, reverse)
    rec.update(dict(name=b"q" + name.encode().replace(b" ", b"_"), flag=16 if reverse else 0, mapq=37, rnext=0, pnext=0, tlen=0), **over)
    return rec


@pytest.mark.parametrize("name", sorted(SC.CRAFTED))
@pytest.mark.parametrize("reverse", (False, True))
@pytest.mark.parametrize("with_qual", (False, True))
def test_encoder_and_decoder_round_trip_to_the_sam_line(name, reverse, with_qual):
    rec = crafted(name, reverse, rnext=1, pnext=41, tlen=-77)
    qual = bytes(33 + (7 * j) % 94 for j in range(len(rec["read"]))) if with_qual else None
    record = M.encode(rec, qual, SC.REFERENCE)
    assert M.split_records(record + record) == [record, record]
    got = M.decode(record, [b"ref"])
    assert got["line"] == S.crafted_line(rec, rec["name"], qual, SC.REFERENCE, b"ref", rec["flag"], 37, 1, 41, -77)
    assert got["ref_id"] == 0 and got["next_ref_id"] == 0 and got["pos"] == rec["begin"] and got["nm"] == rec["distance"]
    assert got["bin"] == M.reg2bin(rec["begin"], max(rec["end"], rec["begin"] + 1))
    assert [w & 15 for w in got["cigar"]] == [M.BAM_OP[op] for _, op in rec["runs"]]


def test_unmapped_records_and_the_sequence_alphabet():
    letters = b"ACGTNacgtnRYKMSWBDHV=xz."
    rec = dict(read=letters, strand=-1, name=b"u", flag=4, mapq=9, rnext=0, pnext=0, tlen=0, runs=[], begin=-1, end=-1, distance=0)
    got = M.decode(M.encode(rec, None, SC.REFERENCE), [b"ref"])
    assert got["seq"] == b"ACGTNACGTNRYKMSWBDHV=NNN" and (got["ref_id"], got["pos"], got["bin"], got["mapq"]) == (-1, -1, 4680, 0)
    assert got["line"] == S.line(b"u", 4, b"*", 0, 0, "*", b"*", 0, 0, got["seq"], None)
    beside = dict(rec, flag=69, rnext=1, pnext=778)        # beside a mapped mate: its refID and pos
    got = M.decode(M.encode(beside, b"I" * len(letters), SC.REFERENCE), [b"ref"])
    assert (got["ref_id"], got["pos"], got["next_ref_id"], got["next_pos"], got["bin"]) == (0, 777, 0, 777, M.reg2bin(777, 778))
    assert got["line"].split(b"\t")[1:9] == [b"69", b"ref", b"778", b"0", b"*", b"=", b"778", b"0"]
    assert M.pack_seq(b"ACG") == bytes([0x12, 0x40])
    other = M.decode(M.encode(dict(beside, strand=0, begin=205, end=229, runs=[(24, "=")], flag=65), None, b"A" * 300, ref_id=2, start=200,
                              mate=(0, 0)), [b"one", b"two", b"three"])
    assert (other["ref_id"], other["pos"], other["next_ref_id"]) == (2, 5, 0) and other["line"].split(b"\t")[6] == b"one"


def test_reg2bin_is_the_smallest_bin_that_contains_the_interval():
    rng = np.random.default_rng(14)
    assert M.reg2bin(-1, 0) == 4680 == M.smallest_bin(-1, 0)
    cases = [(0, 1), (0, 2 ** 29), (2 ** 29 - 1, 2 ** 29), (2 ** 14 - 1, 2 ** 14), (2 ** 14 - 1, 2 ** 14 + 1), (2 ** 14, 2 ** 14 + 1)]
    for edge in (2 ** 14, 2 ** 17, 2 ** 20, 2 ** 23, 2 ** 26):
        for k in (1, 3, 5):
            cases += [(k * edge - int(a), k * edge + int(b)) for a, b in rng.integers(1, 300, size=(8, 2))]      # straddles the edge
            cases += [(k * edge - int(a), k * edge) for a in rng.integers(1, 300, size=4)] + [(k * edge, k * edge + int(a)) for a in rng.integers(1, 300, size=4)]
    begs = rng.integers(0, 2 ** 29 - 1, size=400)
    cases += [(int(b), int(min(2 ** 29, b + n))) for b, n in zip(begs, rng.integers(1, 10 ** rng.integers(1, 8, size=400)))]
    levels = set()
    for beg, end in cases:
        got = M.reg2bin(beg, end)
        assert got == M.smallest_bin(beg, end), (beg, end)
        levels.add(sum(got >= first for first in (1, 9, 73, 585, 4681)))
    assert levels == set(range(6))


@pytest.mark.parametrize("lanes", (64, 256))
def test_the_sliced_crc_equals_zlib(lanes):
    rng = np.random.default_rng(lanes)
    data = rng.integers(0, 256, size=1020 * 64 + 1, dtype=np.uint8).tobytes()
    for n in list(range(301)) + [65279, 65280, 1020 * 64 - 1, 1020 * 64 + 1]:
        assert M.sliced_crc(data[:n], lanes) == zlib.crc32(data[:n]), n
    assert M.sliced_crc(b"\x00" * 700, lanes) == zlib.crc32(b"\x00" * 700)        # slices whose raw state is 0
    assert M.gf_mul(0x80000000, 0x12345678) == 0x12345678 and M.x_pow_bytes(0) == 0x80000000 and M.x_pow_bytes(1) == 0x00800000


# ---- 2. the host framing ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PAYLOADS)
def test_bgzf_blocks_inflate_and_pass_the_walker(P):
    rng = np.random.default_rng(P)
    for n in (0, 1, P - 1, P, P + 1, 2 * P + 17):
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        blocks = B.bgzf_blocks(data, P)
        assert blocks == M.frame(data, P) and len(blocks) == n + 31 * -(-n // P)
        assert gzip.decompress(blocks + B.BGZF_EOF) == data
        pieces = M.walk_blocks(blocks + B.BGZF_EOF)
        assert b"".join(pieces) == data and pieces[-1] == b"" and [len(x) for x in pieces[:-1]] == [P] * (n // P) + [n % P] * (n % P > 0)
    assert B.BGZF_EOF == M.BGZF_EOF and len(B.BGZF_EOF) == 28 and M.walk_blocks(B.BGZF_EOF) == [b""]
    with pytest.raises(AssertionError):
        M.walk_blocks(blocks[:40] + bytes([blocks[40] ^ 1]) + blocks[41:])       # the walker sees a damaged byte
    for bad in (0, 65281, -1):
        with pytest.raises(B.BgsaHipError, match="block_payload"):
            B.bgzf_blocks(b"abc", bad)


# ---- 3. the symbols and the C ABI's refusals ------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped(L):
    declared = B.declared_symbols()
    for path in (B.LIB_PATH, B.LIB_AB_PATH):
        flavour = ctypes.CDLL(str(path))
        for name in SYMBOLS:
            assert name in declared and hasattr(flavour, name), (path.name, name)
    assert [len(getattr(L, name).argtypes) for name in SYMBOLS] == [5, 7, 6, 8, 2, 6]
    assert L.bgsa_hip_bgzf_framed_bytes.restype is ctypes.c_int64
    assert B.BamRecords._fields == ("blocks", "offsets", "flag", "pos", "mapq", "nm")
    for name in ("map_reads_bam", "map_pairs_bam", "bam_header"):
        assert hasattr(B.ReferenceMapper, name) and name in vars(B.ContigMapper)


def test_framed_bytes_is_the_formula(L):
    f = L.bgsa_hip_bgzf_framed_bytes
    for P in PAYLOADS + (65279,):
        for n in (0, 1, P - 1, P, P + 1, 2 * P + 17, 10 ** 9 + 7):
            assert f(n, P) == n + 31 * -(-n // P), (n, P)
    assert f(0, 65280) == 0 and f(36_700_000, 65280) == 36_700_000 + 31 * 563
    assert f(-1, 256) == -1 and f(5, 0) == -1 and f(5, -3) == -1 and f(5, 65281) == -1 and f(5, 65505) == -1 and f(2 ** 62, 1) == -1


def test_frame_call_refusals(L):
    def frame(payload=PTR, n=100, P=64, out=PTR, out_bytes=None):
        return L.bgsa_hip_bgzf_frame_dev(payload, n, P, out, n + 31 * -(-n // max(P, 1)) if out_bytes is None else out_bytes, None)
    assert frame(payload=None) == EINVAL and b"NULL" in L.bgsa_hip_last_error() and frame(out=None) == EINVAL
    for P in (0, -1, 65281, 65505):
        assert frame(P=P, out_bytes=200) == EINVAL and b"1..65280" in L.bgsa_hip_last_error()
    assert frame(n=-1, out_bytes=0) == EINVAL
    for wrong in (99, 100, 161, 163, 0):
        assert frame(out_bytes=wrong) == EINVAL and b"framed_bytes" in L.bgsa_hip_last_error()
    assert frame(n=0) == 0 and frame(n=0, P=65280, out_bytes=0) == 0       # nothing to do: nothing is launched
    assert frame(n=0, out_bytes=31) == EINVAL


def test_record_call_refusals(L):
    table = B.SamContigs(PTR, PTR, 8, PTR, PTR, 3)

    def passes(contigs):
        extra = (table,) if contigs else ()
        measure = L.bgsa_hip_bam_measure_contigs_dev if contigs else L.bgsa_hip_bam_measure_dev
        emit = L.bgsa_hip_bam_emit_contigs_dev if contigs else L.bgsa_hip_bam_emit_dev
        return (lambda batch, n=1, lengths=PTR, malformed=PTR: measure(batch, *extra, n, lengths, malformed, None),
                lambda batch, n=1, offsets=PTR, payload=PTR, payload_bytes=100, malformed=PTR: emit(batch, *extra, n, offsets, payload, payload_bytes,
                                                                                                  malformed, None))
    for contigs in (False, True):
        measure, emit = passes(contigs)
        assert measure(None) == EINVAL and emit(None) == EINVAL and b"NULL" in L.bgsa_hip_last_error()
        for name, kind in B.SamBatch._fields_:
            bad = SC.good_batch(**{name: None if kind is ctypes.c_void_p else 0})
            if name == "d_quals" or (contigs and name in ("d_rname", "rname_len")):        # optional / not read by the contig form
                assert measure(bad, n=0) == 0 and emit(bad, n=0) == 0
            else:
                assert measure(bad) == EINVAL and emit(bad) == EINVAL, name
        good = SC.good_batch()
        assert measure(good, lengths=None) == EINVAL and measure(good, malformed=None) == EINVAL
        assert emit(good, offsets=None) == EINVAL and emit(good, payload=None) == EINVAL and emit(good, malformed=None) == EINVAL
        assert emit(good, payload_bytes=-1) == EINVAL and measure(good, n=-1) == EINVAL and emit(good, n=-1) == EINVAL
        assert measure(good, n=0) == 0 and emit(good, n=0, payload_bytes=0) == 0      # nothing to do: nothing is launched
    assert L.bgsa_hip_bam_measure_contigs_dev(SC.good_batch(), None, 1, PTR, PTR, None) == EINVAL
    assert L.bgsa_hip_bam_emit_contigs_dev(SC.good_batch(), B.SamContigs(PTR, PTR, 8, PTR, PTR, 0), 1, PTR, PTR, 10, PTR, None) == EINVAL


# ---- 4. check_bam_call, bam_header, write_bam --------------------------------------------------------------------------------------------
def test_check_bam_call_adds_its_refusals_to_check_sam_calls():
    good = dict(who="map_reads_bam", lens=[4, 4], names=["a", "b" * 254], quals=[b"IIII", b"!~!~"], reference_name="chr1")
    got, want = B.check_bam_call(**good), B.check_sam_call(**good)
    assert all(np.array_equal(x, y) for x, y in zip(got, want)) and len(got) == 4
    assert all(np.array_equal(x, y) for x, y in zip(B.check_bam_call(**good, block_payload=1), want))
    for over, text in ((dict(names=["a", "b" * 255]), "name of read 1 has 255 bytes, a BAM record holds 254"), (dict(names=["a"]), "1 names for 2 reads"),
                       (dict(reference_name="chr 1"), "reference_name holds"), (dict(quals=[b"III", b"IIII"]), "QUAL of read 0 has 3 bytes"),
                       (dict(block_payload=0), "block_payload 0 outside 1..65280"), (dict(block_payload=65281), "block_payload 65281 outside"),
                       (dict(block_payload=256.0), "block_payload"), (dict(block_payload=None), "block_payload"), (dict(block_payload=True), "block_payload")):
        with pytest.raises(B.BgsaHipError, match=text):
            B.check_bam_call(**{**good, **over})


def test_the_bam_entry_points_refuse_before_they_touch_a_device():
    mapper, reads = SC.bare_mapper(), np.full((4, 32), ord("A"), np.uint8)
    for over, text in ((dict(names=["n" * 255] * 4), "holds 254 at the most"), (dict(block_payload=0), "block_payload"), (dict(block_payload=65281), "block_payload"),
                       (dict(names=["a"]), "1 names for 4 reads"), (dict(max_distance=None), "max_distance is required"), (dict(cigar_cap=0), "cigar_cap")):
        with pytest.raises(B.BgsaHipError, match=text):
            mapper.map_reads_bam(**{**dict(reads=reads, max_distance=2), **over})
    for over, text in ((dict(names=["a", "b", "c", "d" * 300]), "name of read 3 has 300 bytes"), (dict(block_payload=-5), "block_payload"),
                       (dict(quals1=reads + 1), "quals1 and quals2 come together"), (dict(insert_min=0), "insert_min")):
        with pytest.raises(B.BgsaHipError, match=text):
            mapper.map_pairs_bam(**{**dict(reads1=reads, reads2=reads, insert_min=60, insert_max=200, max_distance=2), **over})
    assert mapper.last_pair_stats is None and mapper.last_seed_stats is None


def bare_contig_mapper(names, lens):
    mapper = object.__new__(B.ContigMapper)
    mapper.contig_names, mapper.contig_lens = [n.encode() for n in names], np.array(lens, dtype=np.int64)
    return mapper


def test_bam_headers_decode_to_what_went_in():
    one = SC.bare_mapper()
    text, references, used = M.decode_header(one.bam_header("chr7"))
    assert text == one.sam_header("chr7") and references == [(b"chr7", 3000)] and used == len(one.bam_header("chr7"))
    assert one.bam_header() == M.encode_header(one.sam_header(), [(b"ref", 3000)])
    with pytest.raises(B.BgsaHipError, match="reference_name"):
        one.bam_header("chr 7")
    one.ref_len = 2 ** 31
    with pytest.raises(B.BgsaHipError, match="2\\^31 - 1 at the most"):
        one.bam_header()
    three = bare_contig_mapper(["chrA", "b", "scaffold_17"], [5000, 31, 2 ** 31 - 1])
    text, references, used = M.decode_header(three.bam_header())
    assert text == three.sam_header() and references == [(b"chrA", 5000), (b"b", 31), (b"scaffold_17", 2 ** 31 - 1)]
    assert used == len(three.bam_header()) and text.count(b"@SQ") == 3
    with pytest.raises(B.BgsaHipError, match="b has 2147483648 bases"):
        bare_contig_mapper(["a", "b"], [5, 2 ** 31]).bam_header()


def test_write_bam_of_two_hand_made_batches_decodes_whole(tmp_path):
    mapper = SC.bare_mapper()
    recs = [crafted(name, i % 2 == 1) for i, name in enumerate(sorted(SC.CRAFTED))]
    recs.append(dict(read=b"ACGTN", strand=-1, name=b"u", flag=4, mapq=0, rnext=0, pnext=0, tlen=0, runs=[], begin=-1, end=-1, distance=0))
    encoded = [M.encode(r, None, SC.REFERENCE) for r in recs]
    batches = []
    for part, P in ((encoded[:4], 61), (encoded[4:], 65280)):      # a record straddles blocks in the first batch
        offsets = np.concatenate(([0], np.cumsum([len(x) for x in part]))).astype(np.int64)
        blocks = np.frombuffer(B.bgzf_blocks(b"".join(part), P), np.uint8)
        batches.append(B.BamRecords(blocks, offsets, *(np.zeros(len(part), np.int32),) * 4))
    header = mapper.bam_header("chrT")
    B.write_bam(tmp_path / "two.bam", header, batches)
    data = (tmp_path / "two.bam").read_bytes()
    assert data.endswith(B.BGZF_EOF) and b"".join(M.walk_blocks(data)) == gzip.decompress(data)
    whole = gzip.decompress(data)
    text, references, used = M.decode_header(whole)
    assert text == mapper.sam_header("chrT") and references == [(b"chrT", 3000)] and whole[:used] == header
    records = M.split_records(whole[used:])
    assert records == encoded
    lines = [M.decode(x, [b"chrT"])["line"] for x in records]
    assert lines[:-1] == [S.crafted_line(r, r["name"], None, SC.REFERENCE, b"chrT", r["flag"], 37) for r in recs[:-1]]
    B.write_bam(tmp_path / "one.bam", header, batches[1])      # one BamRecords, not a sequence
    assert M.split_records(gzip.decompress((tmp_path / "one.bam").read_bytes())[used:]) == encoded[4:]
    B.write_bam(tmp_path / "none.bam", header, [])
    assert gzip.decompress((tmp_path / "none.bam").read_bytes()) == header

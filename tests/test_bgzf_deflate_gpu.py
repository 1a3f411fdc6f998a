"""The BGZF deflate stage on the MI355X: deflate, scan and pack on the device at odd byte addresses between sentinels, byte for byte
against the host model of tests/deflate_reference.py and inflated by zlib; pack's refusals; map_reads_bam / map_pairs_bam with
compress=True decoded back to the text the SAM entry points write; a file of a compressed and a stored batch; compress=False
unmoved."""
import gzip
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bam_reference as M  # noqa: E402
import contig_reference as C  # noqa: E402
import deflate_reference as D  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = 0xA5           # what a byte holds where nobody may write
RNAME = b"chrT"
LEAD, TAIL = 17, 64   # sentinel bytes in front of and behind every buffer; LEAD is odd: the bytes start at an odd address


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


def fenced(torch, n: int):
    """A buffer of n bytes at an odd address between sentinels: (the whole tensor, the address of its n bytes)."""
    buffer = torch.full((LEAD + n + TAIL,), SENT, dtype=torch.uint8, device="cuda")
    assert (buffer.data_ptr() + LEAD) % 2 == 1
    return buffer, buffer.data_ptr() + LEAD


def unfenced(buffer, n: int) -> np.ndarray:
    host = buffer.cpu().numpy()
    assert (host[:LEAD] == SENT).all() and (host[LEAD + n:] == SENT).all(), "a byte outside the buffer was written"
    return host[LEAD: LEAD + n]


# ---- 1. deflate, scan, pack ---------------------------------------------------------------------------------------------------------------
def deflate_on_device(torch, data: bytes, P: int) -> tuple:
    """(the packed blocks, the block lengths, the slots as the deflate call left them)."""
    L = B.lib()
    n_blocks = -(-len(data) // P)
    source, at = fenced(torch, len(data))
    source[LEAD: LEAD + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    slots, slots_at = fenced(torch, n_blocks * (P + 31))
    lengths = torch.full((n_blocks + 1,), -7, dtype=torch.int64, device="cuda")
    room = int(L.bgsa_hip_bgzf_deflate_workspace_bytes(len(data), P))
    assert room >= 0
    workspace = torch.zeros(room // 4 + 1, dtype=torch.int32, device="cuda")
    B.check(L.bgsa_hip_bgzf_deflate_dev(at, len(data), P, slots_at, n_blocks * (P + 31), lengths.data_ptr(), workspace.data_ptr(), room, None),
            "bgzf_deflate_dev")
    offsets = torch.zeros(n_blocks + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(lengths[:n_blocks], 0)
    out_bytes = int(offsets[-1].item())
    out, out_at = fenced(torch, out_bytes)
    refused = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.check(L.bgsa_hip_bgzf_pack_dev(slots_at, P, n_blocks, offsets.data_ptr(), out_at, out_bytes, refused.data_ptr(), None), "bgzf_pack_dev")
    torch.cuda.synchronize()
    assert int(refused.item()) == 0 and int(lengths[n_blocks].item()) == -7
    assert unfenced(source, len(data)).tobytes() == data
    return unfenced(out, out_bytes).tobytes(), lengths[:n_blocks].cpu().numpy(), unfenced(slots, n_blocks * (P + 31))


@pytest.mark.parametrize("name", sorted(D.payloads()))
def test_device_blocks_equal_the_model_and_inflate(torch_gpu, name):
    data = D.payloads()[name]
    for P in D.BLOCK_PAYLOADS:
        want = D.modelled(name, P)
        got, lengths, slots = deflate_on_device(torch_gpu, data, P)
        assert lengths.tolist() == [len(b) for b in want], (name, P)
        assert got == b"".join(want), (name, P)
        assert b"".join(M.walk_blocks(got, stored=False)) == data and gzip.decompress(got + B.BGZF_EOF) == data
        slots = slots.reshape(len(want), P + 31)
        for b in (0, len(want) // 2, len(want) - 1):          # block b complete at slot b, the rest of the slot untouched
            assert slots[b, : len(want[b])].tobytes() == want[b] and (slots[b, len(want[b]):] == SENT).all(), (name, P, b)
        used = np.arange(P + 31)[None, :] < lengths[:, None]
        assert (slots[~used] == SENT).all(), (name, P)


def test_an_empty_payload_gives_no_block(torch_gpu):
    got, lengths, _ = deflate_on_device(torch_gpu, b"", 256)
    assert got == b"" and lengths.size == 0


def test_pack_refuses_and_counts_what_it_cannot_place(torch_gpu):
    torch, L = torch_gpu, B.lib()
    P, n_blocks = 256, 4
    slots = torch.arange(n_blocks * (P + 31), dtype=torch.int32, device="cuda").to(torch.uint8)
    host = slots.cpu().numpy().reshape(n_blocks, P + 31)
    good = [0, 100, 100 + 287, 100 + 287 + 50, 100 + 287 + 50 + 30]

    def pack(offsets, out_bytes):
        out, at = fenced(torch, good[-1])
        refused = torch.zeros(1, dtype=torch.int32, device="cuda")
        d_offsets = torch.tensor(offsets, dtype=torch.int64, device="cuda")
        B.check(L.bgsa_hip_bgzf_pack_dev(slots.data_ptr(), P, n_blocks, d_offsets.data_ptr(), at, out_bytes, refused.data_ptr(), None), "pack")
        torch.cuda.synchronize()
        return unfenced(out, good[-1]), int(refused.item())

    def expected(offsets, placed):
        want = np.full(good[-1], SENT, np.uint8)
        for b in placed:
            want[offsets[b]: offsets[b + 1]] = host[b, : offsets[b + 1] - offsets[b]]
        return want
    out, refused = pack(good, good[-1])
    assert refused == 0 and np.array_equal(out, expected(good, range(4)))
    backwards = [0, 100, 90, 437, 467]                          # block 1 runs backwards; block 2 is then 347 long: more than its slot
    out, refused = pack(backwards, good[-1])
    assert refused == 2 and np.array_equal(out, expected(backwards, (0, 3)))
    oversized = [0, 100, 100 + 288, 438, 467]                   # 288 bytes: one more than a slot holds
    out, refused = pack(oversized, good[-1])
    assert refused == 1 and np.array_equal(out, expected(oversized, (0, 2, 3)))
    out, refused = pack(good, good[-1] - 1)                     # the last block would leave out_bytes
    assert refused == 1 and np.array_equal(out, expected(good, (0, 1, 2)))
    out, refused = pack([-5, 100, 387, 437, 467], good[-1])     # a negative offset
    assert refused == 1 and np.array_equal(out, expected(good, (1, 2, 3)))


# ---- 2. the entry points ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(torch_gpu):
    ref, reads1, reads2, kinds, _ = PM.make_case()
    rng = np.random.default_rng(7)
    extra = ACGT[rng.integers(4, size=(2, 4, PM.N))]      # four pairs of unrelated ends: both ends unmapped
    reads1, reads2 = np.concatenate((reads1, extra[0])), np.concatenate((reads2, extra[1]))
    names = [f"pair{c}/{kind}".encode() for c, kind in enumerate(list(kinds) + ["nowhere"] * 4)]
    quals = [bytes(rng.integers(33, 127, size=PM.N, dtype=np.uint8)) for _ in range(2 * len(names))]
    return dict(ref=ref, reads=(reads1, reads2), names=names, quals=(quals[::2], quals[1::2]), mapper=B.ReferenceMapper(ref, PM.W, PM.S))


def splits_a_block_size(offsets, P: int) -> bool:
    """Whether some record's 4-byte block_size field lies in two blocks of P payload bytes."""
    return bool((offsets[:-1] % P > P - 4).any())


def block_list(blocks: bytes) -> list:
    out, at = [], 0
    while at < len(blocks):
        size = int.from_bytes(blocks[at + 16: at + 18], "little") + 1
        out.append(blocks[at: at + size])
        at += size
    return out


def assert_compressed_form_of(got: B.BamRecords, stored: B.BamRecords, sam: B.SamRecords, ref_names, P: int, what: str) -> list:
    """The compressed call's blocks are the model's blocks of the stored call's payload, inflate to it, decode to the SAM text; the
    other fields are the stored call's."""
    payload = b"".join(M.walk_blocks(stored.blocks.tobytes()))
    blocks = got.blocks.tobytes()
    assert b"".join(M.walk_blocks(blocks, stored=False)) == payload and gzip.decompress(blocks + B.BGZF_EOF) == payload, what
    assert blocks == b"".join(D.deflate_blocks(payload, P)), what
    assert len(blocks) <= len(stored.blocks), what
    for name in ("offsets", "flag", "pos", "mapq", "nm"):
        assert np.array_equal(getattr(got, name), getattr(stored, name)) and getattr(got, name).dtype == getattr(stored, name).dtype, (what, name)
    text = sam.text.tobytes()
    decoded = [M.decode(x, ref_names) for x in M.split_records(payload)]
    assert b"".join(d["line"] for d in decoded) == text and len(decoded) == sam.flag.size, what
    return block_list(blocks)


def test_map_reads_bam_compressed_decodes_to_map_reads_sam(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    sam = mapper.map_reads_sam(reads, names, quals, RNAME, **args)
    stored = mapper.map_reads_bam(reads, names, quals, RNAME, **args)
    whole = mapper.map_reads_bam(reads, names, quals, RNAME, compress=True, **args)
    blocks = assert_compressed_form_of(whole, stored, sam, [RNAME], 65280, "single, the default block")
    assert any(D.is_dynamic(b) for b in blocks) and len(whole.blocks) < len(stored.blocks)
    small = next(P for P in (256, 61) if splits_a_block_size(stored.offsets, P))
    cut = mapper.map_reads_bam(reads, names, quals, RNAME, block_payload=small, compress=True, **args)
    assert_compressed_form_of(cut, mapper.map_reads_bam(reads, names, quals, RNAME, block_payload=small, **args), sam, [RNAME], small,
                              f"single, blocks of {small}")
    bare = mapper.map_reads_bam(reads, compress=True, **args)                        # default names, no QUAL: long runs of 0xff
    blocks = assert_compressed_form_of(bare, mapper.map_reads_bam(reads, **args), mapper.map_reads_sam(reads, **args), [b"ref"], 65280,
                                       "single, bare")
    assert all(D.is_dynamic(b) for b in blocks)
    with pytest.raises(B.BgsaHipError, match="compress"):
        mapper.map_reads_bam(reads, names, quals, RNAME, compress=1, **args)


def test_map_pairs_bam_compressed_decodes_to_map_pairs_sam(case):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    ends = (reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, RNAME)
    sam = mapper.map_pairs_sam(*ends, **args)
    stored = mapper.map_pairs_bam(*ends, **args)
    whole = mapper.map_pairs_bam(*ends, compress=True, **args)
    blocks = assert_compressed_form_of(whole, stored, sam, [RNAME], 65280, "pairs, the default block")
    assert any(D.is_dynamic(b) for b in blocks) and len(whole.blocks) < len(stored.blocks)
    small = next(P for P in (256, 61) if splits_a_block_size(stored.offsets, P))
    cut = mapper.map_pairs_bam(*ends, block_payload=small, compress=True, **args)
    assert_compressed_form_of(cut, mapper.map_pairs_bam(*ends, block_payload=small, **args), sam, [RNAME], small, f"pairs, blocks of {small}")
    mid = mapper.map_pairs_bam(*ends, block_payload=4096, compress=True, **args)     # several blocks, each with its own codes
    blocks = assert_compressed_form_of(mid, mapper.map_pairs_bam(*ends, block_payload=4096, **args), sam, [RNAME], 4096, "pairs, blocks of 4,096")
    assert len(blocks) >= 2 and any(D.is_dynamic(b) for b in blocks)


def test_the_contig_form_compresses_too(torch_gpu):
    F = C.FIXTURE
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=C.PAIRS["PADDING"])
    order = list(F["NAMES"])
    reads = np.array([list(read) for _, _, read in C.crafted(sequences)], dtype=np.uint8)
    args = dict(k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    sam = mapper.map_reads_sam(reads, **args)
    got = mapper.map_reads_bam(reads, compress=True, **args)
    blocks = assert_compressed_form_of(got, mapper.map_reads_bam(reads, **args), sam, order, 65280, "contigs, single")
    assert any(D.is_dynamic(b) for b in blocks) and len(got.blocks) < len(mapper.map_reads_bam(reads, **args).blocks)


# ---- 3. a file, and nothing moved -------------------------------------------------------------------------------------------------------------
def test_write_bam_takes_a_compressed_and_a_stored_batch(case, tmp_path):
    mapper, (reads1, reads2), names = case["mapper"], case["reads"], case["names"]
    one = mapper.map_reads_bam(reads1, names, None, RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, compress=True)
    two = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, None, None, RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                               rescue_distance=PM.RESCUE_DISTANCE, block_payload=256)
    assert any(D.is_dynamic(b) for b in block_list(one.blocks.tobytes()))
    B.write_bam(tmp_path / "out.bam", mapper.bam_header(RNAME), (one, two))
    data = (tmp_path / "out.bam").read_bytes()
    assert data[-28:] == B.BGZF_EOF
    whole = gzip.decompress(data)
    assert whole == b"".join(M.walk_blocks(data, stored=False)) and whole[:4] == b"BAM\x01"
    text, references, used = M.decode_header(whole)
    assert text == mapper.sam_header(RNAME) and references == [(RNAME, PM.REF_LEN)]
    records = M.split_records(whole[used:])
    assert len(records) == reads1.shape[0] * 3
    sam = mapper.map_reads_sam(reads1, names, None, RNAME, k_best=2, max_distance=PM.MAX_DISTANCE).text.tobytes() + \
        mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, None, None, RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                             rescue_distance=PM.RESCUE_DISTANCE).text.tobytes()
    assert b"".join(M.decode(x, [RNAME])["line"] for x in records) == sam


def test_a_compressed_call_leaves_the_stored_call_as_it_was(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    before = mapper.map_reads_bam(reads, names, quals, RNAME, compress=False, **args)
    mapper.map_reads_bam(reads, names, quals, RNAME, compress=True, **args)
    after = mapper.map_reads_bam(reads, names, quals, RNAME, **args)
    assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(before, after))
    assert before.blocks.tobytes() == M.frame(b"".join(M.walk_blocks(before.blocks.tobytes())), 65280)

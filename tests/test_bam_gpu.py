"""BAM records on the MI355X: the BGZF framing kernel alone on random bytes, the two record kernels on crafted records (no mapping
involved) byte for byte against tests/bam_reference.py — one sequence and three contigs —, map_reads_bam / map_pairs_bam decoded
back to the text map_reads_sam / map_pairs_sam write for the same call, a file of two batches, and the SAM entry points unmoved."""
import gzip
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bam_reference as M  # noqa: E402
import contig_reference as C  # noqa: E402
import sam_reference as S  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = 0xA5           # what a byte holds where nobody may write
RNAME = b"chrT"
LEAD, TAIL = 17, 64   # sentinel bytes in front of and behind every output; LEAD is odd: the output starts at an odd address


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


def unfenced(buffer, n: int) -> bytes:
    host = buffer.cpu().numpy()
    assert (host[:LEAD] == SENT).all() and (host[LEAD + n:] == SENT).all(), "a byte outside the output was written"
    return host[LEAD: LEAD + n].tobytes()


# ---- 1. framing alone ---------------------------------------------------------------------------------------------------------------------
def frame_on_device(torch, data: bytes, P: int) -> bytes:
    L = B.lib()
    framed = int(L.bgsa_hip_bgzf_framed_bytes(len(data), P))
    assert framed == len(data) + 31 * -(-len(data) // P)
    source, at = fenced(torch, len(data))      # the payload at an odd address too
    source[LEAD: LEAD + len(data)] = torch.from_numpy(np.frombuffer(data, np.uint8).copy()).cuda()
    out, out_at = fenced(torch, framed)
    B.check(L.bgsa_hip_bgzf_frame_dev(at, len(data), P, out_at, framed, None), "bgzf_frame_dev")
    torch.cuda.synchronize()
    return unfenced(out, framed)


@pytest.mark.parametrize("P", (1, 61, 256, 65280))
def test_framed_blocks_equal_the_model_and_inflate(torch_gpu, P):
    rng = np.random.default_rng(P)
    lengths = (65279, 65280, 65281, 130577) if P == 65280 else (0, 1, P - 1, P, P + 1, 2 * P + 17, 1000)
    for n in lengths:
        data = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        got = frame_on_device(torch_gpu, data, P)
        assert got == M.frame(data, P), (P, n)
        assert gzip.decompress(got + B.BGZF_EOF) == data and b"".join(M.walk_blocks(got)) == data
    zeros = frame_on_device(torch_gpu, b"\x00" * (2 * P + 3), P)        # slices whose own CRC state is 0
    assert zeros == M.frame(b"\x00" * (2 * P + 3), P)


def test_a_wrong_out_bytes_is_refused_and_nothing_is_written(torch_gpu):
    torch, L = torch_gpu, B.lib()
    data = torch.arange(1000, dtype=torch.int32, device="cuda").to(torch.uint8)
    framed = int(L.bgsa_hip_bgzf_framed_bytes(1000, 256))
    for wrong in (framed - 1, framed + 1, 1000, 0):
        out, at = fenced(torch, framed)
        assert L.bgsa_hip_bgzf_frame_dev(data.data_ptr(), 1000, 256, at, wrong, None) == -1 and b"framed_bytes" in L.bgsa_hip_last_error()
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == SENT).all()
    out, at = fenced(torch, framed)
    assert L.bgsa_hip_bgzf_frame_dev(data.data_ptr(), 1000, 65281, at, framed, None) == -1
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENT).all()


# ---- 2. the record kernels on crafted records ----------------------------------------------------------------------------------------
CRAFT_LEN, CAP = 140_000, 130
CONTIGS = ((b"cA", 0, 18_000), (b"cB", 20_000, 70_000), (b"cC", 95_000, 45_000))      # name, linear start, length: three, padding between


def mixed_runs(n_runs: int) -> list:
    """n_runs SAM runs, no two neighbours alike, every op among them, I at both ends from 4 runs on."""
    cycle = [(3, "="), (1, "X"), (2, "="), (1, "D"), (4, "="), (2, "I"), (1, "="), (2, "X"), (2, "D"), (3, "I")]
    if n_runs == 1:
        return [(32, "=")]
    runs = [cycle[i % len(cycle)] for i in range(n_runs)]
    if n_runs >= 4:
        runs[0], runs[-1] = (2, "I"), (1, "I")
        if runs[1][1] == "I" or runs[-2][1] == "I":
            runs[1], runs[-2] = (2, "="), (2, "=")
    return runs


def x_bases(runs) -> list:
    """The indices, in the forward read, of the bases of its X runs."""
    out, at = [], 0
    for n, op in runs:
        if op == "X":
            out += range(at, at + n)
        if op in "=XI":
            at += n
    return out


@pytest.fixture(scope="module")
def crafted(torch_gpu):
    """(reference, mapper, the well-formed records with their per-record fields); every mapped record lies inside one of CONTIGS."""
    rng = np.random.default_rng(140)
    ref = ACGT[rng.integers(4, size=CRAFT_LEN)].copy()
    ref[[0, 7, 600, 601, 2 ** 14, CRAFT_LEN - 1]] = ord("N")
    reference = ref.tobytes()
    mapper = B.ReferenceMapper(ref, 96, 48)
    scripts = [(100 + 300 * i, mixed_runs(n)) for i, n in enumerate((1, 63, 64, 65, 130))]
    scripts += [(2000, [(1, "=")]), (2100, [(2, "=")]), (2200, [(33, "=")]), (2300, [(30, "="), (1, "X"), (3, "=")]),      # 1, 2, 33, 34 bp
                (3000, [(1000, "="), (1, "X"), (7, "=")]), (5000, [(5, "I")]),                                                 # 1,008 bp; no reference base
                (0, [(6, "="), (2, "X"), (20, "=")]), (0, [(1, "X"), (30, "=")]),                                              # ref_begin = 0
                (CRAFT_LEN - 40, [(10, "="), (3, "D"), (27, "=")]), (CRAFT_LEN - 5, [(4, "="), (1, "X")]),                     # ref_end = ref_len
                (2 ** 14 - 10, [(12, "="), (1, "X"), (17, "=")]), (2 ** 14 - 1, [(1, "=")]), (2 ** 14, [(1, "X")]),            # across and at 2^14
                (2 ** 17 - 20, [(15, "="), (4, "D"), (3, "I"), (30, "=")]), (2 ** 17 - 33, [(33, "=")]),                       # across and up to 2^17
                (590, [(8, "="), (1, "D"), (2, "X"), (1, "D"), (10, "=")]), (40_000, [(9, "="), (6, "X"), (2, "I"), (9, "=")])]
    records = []
    for i, (begin, runs) in enumerate(scripts):
        rec = S.craft(rng, reference, begin, runs, reverse=i % 2 == 1)
        rec.update(name=(b"q", b"n" * 254, b"read/%05d" % i)[i % 3], flag=(0, 16, 99, 147, 2048 + 16, 65535)[i % 6], mapq=(0, 7, 60, 255)[i % 4],
                   rnext=i % 2, pnext=(0, 9, 1234567, 2 ** 31)[i % 4], tlen=(0, -1, 310, -99999, 2 ** 31 - 1, -2 ** 31)[i % 6])
        records.append(rec)
    for rec, letters in ((records[-1], b"RyKmsn"), (records[-2], b"a")):      # IUPAC, lower case and N where the script says X: forward and reverse
        at = x_bases(rec["runs"])[: len(letters)]
        read = bytearray(rec["read"])
        for j, letter in zip(at, letters):
            read[len(read) - 1 - j if rec["strand"] == 1 else j] = letter
        rec["read"] = bytes(read)
    assert records[-1]["strand"] == 1 and records[-2]["strand"] == 0 and b"R" in records[-1]["read"] and b"a" in records[-2]["read"]
    assert {len(r["read"]) for r in records} >= {1, 2, 33, 34, 1008} and {len(r["runs"]) for r in records} >= {1, 63, 64, 65, 130}
    assert {len(r["name"]) for r in records} == {1, 254, 10}
    for i, (mapped_mate, name) in enumerate(((0, b"u"), (1, b"unmapped-with-a-mapped-mate"))):
        records.append(dict(read=(b"ACGTNacgtnRYKMSWBDHV=x.", bytes(ACGT[rng.integers(4, size=34)]))[i], strand=-1, name=name,
                            flag=(4, 69 + 8 * (1 - mapped_mate))[i], mapq=13, rnext=mapped_mate, pnext=777 * mapped_mate, tlen=0,
                            words=np.zeros(0, np.uint32), begin=-1, end=-1, distance=0, runs=[]))
    return reference, mapper, records


def quals_of(records, seed: int = 3) -> list:
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(33, 127, size=len(r["read"]), dtype=np.uint8)) for r in records]


def contig_of(linear: int) -> tuple:
    """(index, start) of the contig of CONTIGS that holds the linear position."""
    index = max(i for i, (_, start, _) in enumerate(CONTIGS) if start <= linear)
    assert linear < CONTIGS[index][1] + CONTIGS[index][2]
    return index, CONTIGS[index][1]


def as_contig_records(records) -> list:
    """The crafted records for the contig form: pnext linear and on a contig wherever rnext is 1, the mates of some on another contig."""
    out = []
    for i, r in enumerate(records):
        out.append(dict(r, pnext=(25_000, 96_000, 5, 17_999 + 1)[i % 4] if r["rnext"] else 0, tlen=(0, -1, 310)[i % 3]))
    return out


def expected(records, quals, reference, contigs: bool) -> list:
    out = []
    for i, r in enumerate(records):
        own = contig_of(r["begin"]) if contigs and r["strand"] >= 0 else (0, 0)
        mate = contig_of(r["pnext"] - 1) if contigs and r["rnext"] else None
        out.append(M.encode(r, None if quals is None else quals[i], reference, ref_id=own[0], start=own[1], mate=mate))
    return out


class Batch:
    """The device side of a list of record dicts: every array of bgsa_hip_sam_batch_t, the struct, and the contig table.  over:
    {(field, record): value} written into the per-record arrays before they go up."""

    def __init__(self, torch, mapper, records, quals, cap=CAP, over=None):
        n = len(records)
        stride = max(len(r["read"]) for r in records)
        rows = np.full((n, stride), ord("N"), np.uint8)
        qual_rows = np.full((n, stride), ord("!"), np.uint8)
        runs = np.zeros((n, cap), np.uint32)
        for i, r in enumerate(records):
            rows[i, : len(r["read"])] = np.frombuffer(r["read"], np.uint8)
            if quals is not None:
                qual_rows[i, : len(r["read"])] = np.frombuffer(quals[i], np.uint8)
            runs[i, : min(len(r["words"]), cap)] = r["words"][:cap]
        names = np.frombuffer(b"".join(r["name"] for r in records), np.uint8)
        offsets = np.concatenate(([0], np.cumsum([len(r["name"]) for r in records]))).astype(np.int64)
        host = dict(read_row=np.arange(n, dtype=np.int64), name_of=np.arange(n, dtype=np.int64), runs_row=np.arange(n, dtype=np.int64),
                    read_len=np.array([len(r["read"]) for r in records], np.int32), strand=np.array([r["strand"] for r in records], np.int32),
                    ref_begin=np.array([r["begin"] for r in records], np.int64), ref_end=np.array([r["end"] for r in records], np.int64),
                    distance=np.array([r["distance"] for r in records], np.int32), n_ops=np.array([len(r["words"]) for r in records], np.int32),
                    flag=np.array([r["flag"] for r in records], np.int32), mapq=np.array([r["mapq"] for r in records], np.int32),
                    rnext=np.array([r["rnext"] for r in records], np.int32), pnext=np.array([r["pnext"] for r in records], np.int64),
                    tlen=np.array([r["tlen"] for r in records], np.int64))
        for (key, i), value in (over or {}).items():
            host[key][i] = value
        up = lambda x: torch.from_numpy(np.array(x)).cuda()      # noqa: E731
        self.n = n
        d = self.dev = {key: up(value) for key, value in host.items()}
        self.keep = [up(rows), up(qual_rows) if quals is not None else None, up(names), up(offsets), up(np.frombuffer(RNAME, np.uint8)),
                     up(runs.view(np.int32))]
        self.struct = B.SamBatch(self.keep[0].data_ptr(), None if quals is None else self.keep[1].data_ptr(), stride, n, self.keep[2].data_ptr(),
                                 self.keep[3].data_ptr(), n, names.size, self.keep[4].data_ptr(), len(RNAME), mapper.d_reference.data_ptr(),
                                 mapper.ref_len, self.keep[5].data_ptr(), n, cap, d["read_row"].data_ptr(), d["name_of"].data_ptr(),
                                 d["runs_row"].data_ptr(), d["read_len"].data_ptr(), d["strand"].data_ptr(), d["ref_begin"].data_ptr(),
                                 d["ref_end"].data_ptr(), d["distance"].data_ptr(), d["n_ops"].data_ptr(), d["flag"].data_ptr(),
                                 d["mapq"].data_ptr(), d["rnext"].data_ptr(), d["pnext"].data_ptr(), d["tlen"].data_ptr())
        table_names = b"".join(name for name, _, _ in CONTIGS)
        self.table_keep = [up(np.frombuffer(table_names, np.uint8)), up(np.concatenate(([0], np.cumsum([len(name) for name, _, _ in CONTIGS]))).astype(np.int64)),
                           up(np.array([start for _, start, _ in CONTIGS], np.int64)), up(np.array([n for _, _, n in CONTIGS], np.int64))]
        self.table = B.SamContigs(self.table_keep[0].data_ptr(), self.table_keep[1].data_ptr(), len(table_names), self.table_keep[2].data_ptr(),
                                  self.table_keep[3].data_ptr(), len(CONTIGS))


def run_passes(torch, batch: Batch, contigs: bool = False, shift=None):
    """measure -> scan -> emit with the payload at an odd byte address between sentinels: (lengths, offsets, the payload, both
    counters).  shift: (k, by) moves offsets[k] before the emit pass."""
    L = B.lib()
    extra = (batch.table,) if contigs else ()
    measure = L.bgsa_hip_bam_measure_contigs_dev if contigs else L.bgsa_hip_bam_measure_dev
    emit = L.bgsa_hip_bam_emit_contigs_dev if contigs else L.bgsa_hip_bam_emit_dev
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    lengths = torch.full((batch.n + 3,), -7, dtype=torch.int64, device="cuda")
    B.check(measure(batch.struct, *extra, batch.n, lengths.data_ptr(), counters.data_ptr(), None), "bam_measure_dev")
    torch.cuda.synchronize()
    assert lengths[batch.n:].tolist() == [-7] * 3
    offsets = torch.zeros(batch.n + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(lengths[: batch.n], 0)
    total = int(offsets[-1].item())
    if shift is not None:
        offsets[shift[0]] += shift[1]
    buffer, at = fenced(torch, total)
    B.check(emit(batch.struct, *extra, batch.n, offsets.data_ptr(), at, total, counters[1:].data_ptr(), None), "bam_emit_dev")
    torch.cuda.synchronize()
    return lengths[: batch.n].cpu().numpy(), offsets.cpu().numpy(), unfenced(buffer, total), counters.cpu().numpy().tolist()


@pytest.mark.parametrize("contigs", (False, True))
@pytest.mark.parametrize("with_qual", (False, True))
def test_crafted_records_equal_the_model_byte_for_byte(torch_gpu, crafted, with_qual, contigs):
    reference, mapper, records = crafted
    if contigs:
        records = as_contig_records(records)
        mates = {(contig_of(r["begin"])[0], contig_of(r["pnext"] - 1)[0]) for r in records if r["strand"] >= 0 and r["rnext"]}
        assert any(a != b for a, b in mates) and any(a == b for a, b in mates) and {contig_of(r["begin"])[0] for r in records if r["strand"] >= 0} == {0, 1, 2}
    quals = quals_of(records) if with_qual else None
    want = expected(records, quals, reference, contigs)
    lengths, offsets, payload, counters = run_passes(torch_gpu, Batch(torch_gpu, mapper, records, quals), contigs)
    assert counters == [0, 0]
    assert lengths.tolist() == [len(x) for x in want]
    for i, record in enumerate(want):
        got = payload[offsets[i]: offsets[i + 1]]
        assert got == record, (i, records[i]["runs"][:6], got[:120].hex(), record[:120].hex())
    assert M.split_records(payload) == want
    names = [name for name, _, _ in CONTIGS] if contigs else [RNAME]
    decoded = [M.decode(x, names) for x in want]
    assert {r["strand"] for r in records} == {-1, 0, 1}
    assert {d["bin"] for d in decoded} >= ({4680, 4681, 4682, 585} if contigs else {4680, 4681, 4682, 585, 73})      # 73: across 2^17, linear only
    assert any(r["begin"] == 0 for r in records) and any(r["end"] == CRAFT_LEN for r in records) and any(r["begin"] == r["end"] >= 0 for r in records)


def malformed_batch(torch, mapper, records):
    """Five victims, one per rule, among the well-formed records: ({why: index}, the batch)."""
    mapped = [i for i, r in enumerate(records) if r["strand"] >= 0 and len(r["name"]) < 200]
    victims = dict(zip(("a 255-byte name", "pnext = 2^31 + 1", "tlen = 2^33", "n_ops > cigar_cap", "an interval outside the reference"), mapped[2:12:2]))
    changed = [dict(r) for r in records]
    changed[victims["a 255-byte name"]]["name"] = b"N" * 255
    over = {("pnext", victims["pnext = 2^31 + 1"]): 2 ** 31 + 1, ("tlen", victims["tlen = 2^33"]): 2 ** 33,
            ("n_ops", victims["n_ops > cigar_cap"]): CAP + 1, ("ref_end", victims["an interval outside the reference"]): CRAFT_LEN + 1}
    return victims, Batch(torch, mapper, changed, None, over=over)


def test_malformed_records_get_length_zero_are_counted_and_write_nothing(torch_gpu, crafted):
    reference, mapper, records = crafted
    victims, batch = malformed_batch(torch_gpu, mapper, records)
    bad = set(victims.values())
    assert len(bad) == 5 and all(i + 1 not in bad for i in bad)
    want = expected(records, None, reference, False)
    lengths, offsets, payload, counters = run_passes(torch_gpu, batch)
    assert counters == [5, 5]
    assert [i for i in range(len(records)) if lengths[i] == 0] == sorted(bad)
    assert payload == b"".join(x for i, x in enumerate(want) if i not in bad)        # the neighbours' bytes, and nothing else
    for i in sorted(bad):
        assert payload[offsets[i - 1]: offsets[i]] == want[i - 1] and payload[offsets[i + 1]: offsets[i + 2]] == want[i + 1]


def test_the_emit_pass_refuses_a_record_whose_room_is_not_its_length(torch_gpu, crafted):
    reference, mapper, records = crafted
    want = expected(records, None, reference, False)
    k = 6                                                 # offsets[k] moves: record k - 1 gets a byte too many, record k one too few
    lengths, offsets, payload, counters = run_passes(torch_gpu, Batch(torch_gpu, mapper, records, None), shift=(k, 1))
    assert counters == [0, 2]
    good = np.concatenate(([0], np.cumsum(lengths)))
    for i, record in enumerate(want):
        got = payload[good[i]: good[i + 1]]
        assert got == (bytes([SENT]) * len(record) if i in (k - 1, k) else record), i
    _, _, payload, counters = run_passes(torch_gpu, Batch(torch_gpu, mapper, records, None), shift=(len(records), 1))      # beyond the buffer
    assert counters == [0, 1] and payload == b"".join(want[:-1]) + bytes([SENT]) * len(want[-1])


def test_the_driver_frames_crafted_records_and_names_a_malformed_read(torch_gpu, crafted):
    reference, mapper, records = crafted
    batch = Batch(torch_gpu, mapper, records, None)
    fields = {key: value for key, value in batch.dev.items() if key != "runs_row"}
    names, offsets, rows = batch.keep[2].cpu().numpy(), batch.keep[3].cpu().numpy(), batch.keep[0].cpu().numpy()
    want = expected(records, None, reference, False)
    for P in (61, 65280):
        got = mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), fields, batch.keep[5], fmt="bam", block_payload=P)
        assert isinstance(got, B.BamRecords) and got.blocks.tobytes() == M.frame(b"".join(want), P)
        assert got.offsets.tolist() == np.concatenate(([0], np.cumsum([len(x) for x in want]))).tolist()
        assert got.nm.tolist() == [r["distance"] if r["strand"] >= 0 else -1 for r in records]
    far = dict(fields, tlen=fields["tlen"].clone())
    far["tlen"][4] = 2 ** 33
    with pytest.raises(B.BgsaHipError, match="1 malformed records, the first the one of read 4"):
        mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), far, batch.keep[5], fmt="bam")
    sam = mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), far, batch.keep[5])      # SAM prints that TLEN
    assert isinstance(sam, B.SamRecords) and b"\t8589934592\t" in sam.text.tobytes()


# ---- 3. the entry points: every record decoded back to the line the SAM entry point writes ------------------------------------------------
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


def small_payload(offsets) -> int:
    return next(P for P in (256, 61) if splits_a_block_size(offsets, P))


def assert_decodes_to(got: B.BamRecords, sam: B.SamRecords, ref_names, P: int, what: str) -> list:
    """The blocks walked, inflated and split; the records agree with the offsets and decode to the SAM text; the columns agree."""
    blocks = got.blocks.tobytes()
    pieces = M.walk_blocks(blocks)
    payload = b"".join(pieces)
    assert gzip.decompress(blocks + B.BGZF_EOF) == payload, what
    assert all(len(x) == P for x in pieces[:-1]) and 1 <= len(pieces[-1]) <= P, what
    records = M.split_records(payload)
    assert got.offsets.tolist() == np.concatenate(([0], np.cumsum([len(x) for x in records]))).tolist(), what
    decoded = [M.decode(x, ref_names) for x in records]
    text = sam.text.tobytes()
    for i, d in enumerate(decoded):
        assert d["line"] == text[sam.offsets[i]: sam.offsets[i + 1]], (what, i, d["line"], text[sam.offsets[i]: sam.offsets[i + 1]])
    assert b"".join(d["line"] for d in decoded) == text, what
    for name in ("flag", "pos", "mapq", "nm"):
        assert np.array_equal(getattr(got, name), getattr(sam, name)) and getattr(got, name).dtype == getattr(sam, name).dtype, (what, name)
    assert [d["flag"] for d in decoded] == got.flag.tolist() and [d["nm"] for d in decoded] == got.nm.tolist()
    return decoded


def test_map_reads_bam_decodes_to_map_reads_sam(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    sam = mapper.map_reads_sam(reads, names, quals, RNAME, **args)
    whole = mapper.map_reads_bam(reads, names, quals, RNAME, **args)
    assert_decodes_to(whole, sam, [RNAME], 65280, "single, the default block")
    small = small_payload(whole.offsets)
    cut = mapper.map_reads_bam(reads, names, quals, RNAME, block_payload=small, **args)
    assert splits_a_block_size(cut.offsets, small) and np.array_equal(cut.offsets, whole.offsets)
    decoded = assert_decodes_to(cut, sam, [RNAME], small, f"single, blocks of {small}")
    assert {d["flag"] for d in decoded} >= {0, 4, 16} and (sam.flag != 4).sum() > 60
    bare_sam = mapper.map_reads_sam(reads, seeded=False, **args)                     # default names, no QUAL, exhaustive
    assert_decodes_to(mapper.map_reads_bam(reads, seeded=False, **args), bare_sam, [b"ref"], 65280, "single, bare")
    ragged = [bytes(row[: 24 + i % 9]) for i, row in enumerate(reads)]               # mixed lengths: odd and even l_seq
    assert_decodes_to(mapper.map_reads_bam(ragged, names, block_payload=61, **args), mapper.map_reads_sam(ragged, names, **args), [b"ref"], 61,
                      "single, mixed lengths")


def test_map_pairs_bam_decodes_to_map_pairs_sam(case):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    sam = mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, RNAME, **args)
    whole = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, RNAME, **args)
    assert_decodes_to(whole, sam, [RNAME], 65280, "pairs, the default block")
    small = small_payload(whole.offsets)
    cut = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, RNAME, block_payload=small, **args)
    assert splits_a_block_size(cut.offsets, small)
    decoded = assert_decodes_to(cut, sam, [RNAME], small, f"pairs, blocks of {small}")
    flags = cut.flag.reshape(-1, 2)
    assert ((flags & 2) == 2).any() and ((flags & 4) == 4).any() and ((flags[:, 0] & 8) != (flags[:, 1] & 8)).any()
    assert any(d["tlen"] < 0 for d in decoded) and any(d["ref_id"] == 0 and d["flag"] & 4 for d in decoded)      # an unmapped end beside its mate


def test_the_contig_form_writes_ref_ids_in_the_headers_order(torch_gpu):
    F, P = C.FIXTURE, C.PAIRS
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=P["PADDING"])
    text, references, _ = M.decode_header(mapper.bam_header())
    assert text == mapper.sam_header() and references == list(zip(F["NAMES"], F["LENS"])) and len(references) >= 3
    order = [name for name, _ in references]
    named = C.crafted(sequences)
    reads = np.array([list(read) for _, _, read in named], dtype=np.uint8)
    args = dict(k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    sam = mapper.map_reads_sam(reads, **args)
    decoded = assert_decodes_to(mapper.map_reads_bam(reads, block_payload=61, **args), sam, order, 61, "contigs, single")
    assert len({d["ref_id"] for d in decoded} - {-1}) >= 3
    pairs = C.crafted_pairs(sequences)
    reads1, reads2 = (np.array([list(x[e]) for x in pairs], dtype=np.uint8) for e in (1, 2))
    pair_args = dict(k_best=P["K_BEST"], max_distance=F["MAX_DISTANCE"])
    sam = mapper.map_pairs_sam(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], [b"proper", b"across", b"half"], **pair_args)
    got = mapper.map_pairs_bam(reads1, reads2, P["INSERT_MIN"], P["INSERT_MAX"], [b"proper", b"across", b"half"], **pair_args)
    decoded += assert_decodes_to(got, sam, order, 65280, "contigs, pairs")
    across = decoded[-4:-2]                               # the pair whose ends lie on chrA and chrB
    assert [(d["ref_id"], d["next_ref_id"], d["tlen"]) for d in across] == [(C.CHR_A, C.CHR_B, 0), (C.CHR_B, C.CHR_A, 0)]
    assert [(d["ref_id"], d["next_ref_id"]) for d in decoded[-2:]] == [(C.CHR_A, -1), (C.CHR_A, C.CHR_A)]      # the unmapped end takes its mate's
    for d in decoded:                                     # refID is the index of the name the SAM line prints
        rname = d["line"].split(b"\t")[2]
        assert d["ref_id"] == (-1 if rname == b"*" else order.index(rname))
    with pytest.raises(B.BgsaHipError, match="exceeds contig_padding 120"):
        mapper.map_pairs_bam(reads1, reads2, P["INSERT_MIN"], P["PADDING"] + 1, **pair_args)


# ---- 4. a file ------------------------------------------------------------------------------------------------------------------------------
def test_write_bam_streams_two_calls_into_one_file(case, tmp_path):
    mapper, (reads1, reads2), names = case["mapper"], case["reads"], case["names"]
    one = mapper.map_reads_bam(reads1, names, None, RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, block_payload=256)
    two = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, None, None, RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                               rescue_distance=PM.RESCUE_DISTANCE)
    B.write_bam(tmp_path / "out.bam", mapper.bam_header(RNAME), (one, two))
    data = (tmp_path / "out.bam").read_bytes()
    assert data[-28:] == B.BGZF_EOF
    whole = gzip.decompress(data)
    assert whole == b"".join(M.walk_blocks(data)) and whole[:4] == b"BAM\x01"
    text, references, used = M.decode_header(whole)
    assert text == mapper.sam_header(RNAME) and references == [(RNAME, PM.REF_LEN)]
    records = M.split_records(whole[used:])              # exactly the records, and nothing after them
    want = M.split_records(b"".join(M.walk_blocks(one.blocks.tobytes()))) + M.split_records(b"".join(M.walk_blocks(two.blocks.tobytes())))
    assert records == want and len(records) == reads1.shape[0] * 3
    sam = mapper.map_reads_sam(reads1, names, None, RNAME, k_best=2, max_distance=PM.MAX_DISTANCE).text.tobytes() + \
        mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, None, None, RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                             rescue_distance=PM.RESCUE_DISTANCE).text.tobytes()
    assert b"".join(M.decode(x, [RNAME])["line"] for x in records) == sam


# ---- 5. nothing moved --------------------------------------------------------------------------------------------------------------------------
def test_bam_calls_leave_the_sam_entry_points_as_they_were(case):
    mapper, (reads1, reads2), names = case["mapper"], case["reads"], case["names"]
    pair_args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)

    def sam():
        return (mapper.map_reads_sam(reads1, names, k_best=2, max_distance=PM.MAX_DISTANCE),
                mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, **pair_args), mapper.last_seed_stats, mapper.last_pair_stats)

    def same(a, b):
        return type(a) is type(b) is B.SamRecords and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))
    before = sam()
    mapper.map_reads_bam(reads1, names, k_best=2, max_distance=PM.MAX_DISTANCE, block_payload=61)
    mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, **pair_args)
    middle = sam()
    for call in (lambda: mapper.map_reads_bam(reads1, [b"n" * 255] * reads1.shape[0], k_best=2, max_distance=PM.MAX_DISTANCE),
                 lambda: mapper.map_reads_bam(reads1, names, k_best=2, max_distance=PM.MAX_DISTANCE, block_payload=0),
                 lambda: mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, block_payload=65281, **pair_args)):
        with pytest.raises(B.BgsaHipError, match="254 at the most|block_payload"):
            call()
    after = sam()
    for other in (middle, after):
        assert same(before[0], other[0]) and same(before[1], other[1]) and before[2:] == other[2:]

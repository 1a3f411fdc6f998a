"""SAM records on the MI355X: the two record kernels on crafted records (no mapping involved) byte for byte against
tests/sam_reference.py, the MAPQ kernel on random lists, and ReferenceMapper.map_reads_sam / map_pairs_sam against the model fed
with the existing entry points' results on the case of test_pair_map_gpu.py."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import sam_reference as S  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
SENT = 0xA5           # what a byte holds where nobody may write
RNAME = b"chrT"


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


# ---- 1. the record kernels on crafted records ----------------------------------------------------------------------------------------
CRAFT_LEN, CAP = 1200, 130


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


@pytest.fixture(scope="module")
def crafted(torch_gpu):
    """The crafted records: (reference, mapper, the well-formed records with their per-record fields)."""
    rng = np.random.default_rng(1200)
    ref = ACGT[rng.integers(4, size=CRAFT_LEN)].copy()
    ref[[0, 7, 600, 601, CRAFT_LEN - 1]] = ord("N")
    reference = ref.tobytes()
    mapper = B.ReferenceMapper(ref, 96, 48)
    scripts = [(100, mixed_runs(n)) for n in (1, 63, 64, 65, 130)]
    for n in (9, 10, 99, 100, 999, 1000):
        scripts += [(50, [(n, "="), (1, "X"), (5, "=")]), (60, [(5, "="), (n, "D"), (5, "=")]), (70, [(4, "="), (n, "X"), (4, "=")]),
                    (80, [(3, "="), (n, "I"), (3, "=")])]
    scripts += [(0, [(6, "="), (2, "X"), (20, "=")]), (0, [(1, "X"), (30, "=")]),                 # ref_begin = 0, an N under the first base
                (CRAFT_LEN - 40, [(10, "="), (3, "D"), (27, "=")]), (CRAFT_LEN - 5, [(4, "="), (1, "X")]),      # ref_end = ref_len
                (590, [(8, "="), (1, "D"), (2, "X"), (1, "D"), (10, "=")]), (595, [(5, "="), (5, "D"), (3, "I"), (2, "D"), (6, "=")])]
    records = []
    for i, (begin, runs) in enumerate(scripts):
        rec = S.craft(rng, reference, begin, runs, reverse=i % 2 == 1)
        rec.update(name=(b"q" if i % 3 == 0 else b"read/" + b"x" * 30 + b"%05d" % i), flag=(0, 16, 99, 147, 2048 + 16, 65535)[i % 6],
                   mapq=(0, 7, 60, 255)[i % 4], rnext=i % 2, pnext=(0, 9, 1234567, 2 ** 40 + 5)[i % 4],
                   tlen=(0, -1, 310, -99999, 2 ** 33)[i % 5])
        records.append(rec)
    assert {len(r["name"]) for r in records} == {1, 40} and max(len(r["read"]) for r in records) == 1008
    assert {len(r["runs"]) for r in records} >= {1, 63, 64, 65, 130}
    for i, (mapped_mate, name) in enumerate(((0, b"u"), (1, b"unmapped-with-a-mapped-mate"))):
        records.append(dict(read=bytes(ACGT[rng.integers(4, size=33 + i)]), strand=-1, name=name, flag=(4, 69 + 8 * (1 - mapped_mate))[i],
                            mapq=13, rnext=mapped_mate, pnext=777 * mapped_mate, tlen=0, words=np.zeros(0, np.uint32), begin=-1, end=-1, distance=0,
                            runs=[]))
    return reference, mapper, records


def expected_line(rec: dict, qual, reference: bytes) -> bytes:
    if rec["strand"] < 0:
        named = rec["rnext"] == 1
        return S.line(rec["name"], rec["flag"], RNAME if named else b"*", rec["pnext"] if named else 0, 0, "*", b"=" if named else b"*",
                      rec["pnext"], rec["tlen"], rec["read"], qual)
    return S.crafted_line(rec, rec["name"], qual, reference, RNAME, rec["flag"], rec["mapq"], rec["rnext"], rec["pnext"], rec["tlen"])


def quals_of(records, seed: int = 3) -> list:
    rng = np.random.default_rng(seed)
    return [bytes(rng.integers(33, 127, size=len(r["read"]), dtype=np.uint8)) for r in records]


class Batch:
    """The device side of a list of record dicts: every array of bgsa_hip_sam_batch_t, and the struct."""

    def __init__(self, torch, mapper, records, quals, cap=CAP):
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
        up = lambda x: torch.from_numpy(np.array(x)).cuda()      # noqa: E731
        self.n, self.host = n, host
        self.dev = {key: up(value) for key, value in host.items()}
        self.keep = [up(rows), up(qual_rows) if quals is not None else None, up(names), up(offsets), up(np.frombuffer(RNAME, np.uint8)),
                     up(runs.view(np.int32))]
        d = self.dev
        self.struct = B.SamBatch(self.keep[0].data_ptr(), None if quals is None else self.keep[1].data_ptr(), stride, n, self.keep[2].data_ptr(),
                                 self.keep[3].data_ptr(), n, names.size, self.keep[4].data_ptr(), len(RNAME), mapper.d_reference.data_ptr(),
                                 mapper.ref_len, self.keep[5].data_ptr(), n, cap, d["read_row"].data_ptr(), d["name_of"].data_ptr(),
                                 d["runs_row"].data_ptr(), d["read_len"].data_ptr(), d["strand"].data_ptr(), d["ref_begin"].data_ptr(),
                                 d["ref_end"].data_ptr(), d["distance"].data_ptr(), d["n_ops"].data_ptr(), d["flag"].data_ptr(),
                                 d["mapq"].data_ptr(), d["rnext"].data_ptr(), d["pnext"].data_ptr(), d["tlen"].data_ptr())


def run_passes(torch, batch: Batch, lead: int = 17, tail: int = 64):
    """measure -> scan -> emit with the text at an odd byte address between sentinels: (lengths, the text, both counters)."""
    L = B.lib()
    counters = torch.zeros(2, dtype=torch.int32, device="cuda")
    lengths = torch.full((batch.n + 3,), -7, dtype=torch.int64, device="cuda")
    B.check(L.bgsa_hip_sam_measure_dev(batch.struct, batch.n, lengths.data_ptr(), counters.data_ptr(), None), "sam_measure_dev")
    torch.cuda.synchronize()
    assert lengths[batch.n:].tolist() == [-7] * 3
    offsets = torch.zeros(batch.n + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(lengths[: batch.n], 0)
    total = int(offsets[-1].item())
    buffer = torch.full((lead + total + tail,), SENT, dtype=torch.uint8, device="cuda")
    assert (buffer.data_ptr() + lead) % 2 == 1
    B.check(L.bgsa_hip_sam_emit_dev(batch.struct, batch.n, offsets.data_ptr(), buffer.data_ptr() + lead, total, counters[1:].data_ptr(), None),
            "sam_emit_dev")
    torch.cuda.synchronize()
    host = buffer.cpu().numpy()
    assert (host[:lead] == SENT).all() and (host[lead + total:] == SENT).all(), "a byte outside the text was written"
    return lengths[: batch.n].cpu().numpy(), host[lead: lead + total].tobytes(), counters.cpu().numpy().tolist()


@pytest.mark.parametrize("with_qual", (False, True))
def test_crafted_records_equal_the_model_byte_for_byte(torch_gpu, crafted, with_qual):
    reference, mapper, records = crafted
    quals = quals_of(records) if with_qual else None
    want = [expected_line(r, None if quals is None else quals[i], reference) for i, r in enumerate(records)]
    lengths, text, counters = run_passes(torch_gpu, Batch(torch_gpu, mapper, records, quals))
    assert counters == [0, 0]
    assert lengths.tolist() == [len(x) for x in want]
    at = 0
    for i, line in enumerate(want):
        got = text[at: at + len(line)]
        assert got == line, (i, records[i]["runs"][:6], got[:200], line[:200])
        at += len(line)
    assert {r["strand"] for r in records} == {-1, 0, 1}
    assert any(r["begin"] == 0 for r in records) and any(r["end"] == CRAFT_LEN for r in records)


MALFORMED = {      # one per guard: the field of the record that is changed, and to what
    "n_ops > cigar_cap": ("n_ops", CAP + 1),
    "ref_begin < 0": ("ref_begin", -1),
    "ref_end > ref_len": ("ref_end", CRAFT_LEN + 1),
    "reference runs do not add up": ("ref_end", None),       # the record's own ref_end + 1
    "read runs do not add up": ("read_len", None),           # the record's own length - 1
}


def test_malformed_records_get_length_zero_are_counted_and_write_nothing(torch_gpu, crafted):
    reference, mapper, records = crafted
    mapped = [i for i, r in enumerate(records) if r["strand"] >= 0 and r["end"] < CRAFT_LEN - 2]
    victims = dict(zip(MALFORMED, mapped[3:8]))
    batch = Batch(torch_gpu, mapper, records, None)
    for why, (key, value) in MALFORMED.items():
        i = victims[why]
        if value is None:
            value = records[i]["end"] + 1 if key == "ref_end" else len(records[i]["read"]) - 1
        batch.host[key][i] = value
        batch.dev[key][i] = value
    lengths, text, counters = run_passes(torch_gpu, batch)
    assert counters == [5, 5]
    bad = set(victims.values())
    want = b"".join(expected_line(r, None, reference) for i, r in enumerate(records) if i not in bad)
    assert [i for i in range(len(records)) if lengths[i] == 0] == sorted(bad) and text == want


def test_the_driver_raises_and_names_the_read(torch_gpu, crafted):
    reference, mapper, records = crafted
    torch = torch_gpu
    batch = Batch(torch, mapper, records, None)
    fields = {key: value for key, value in batch.dev.items() if key != "runs_row"}
    names, offsets = batch.keep[2].cpu().numpy(), batch.keep[3].cpu().numpy()
    rows = batch.keep[0].cpu().numpy()
    got = mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), fields, batch.keep[5])
    want = [expected_line(r, None, reference) for r in records]
    assert got.text.tobytes() == b"".join(want) and got.offsets.tolist() == np.concatenate(([0], np.cumsum([len(x) for x in want]))).tolist()
    assert got.nm.tolist() == [r["distance"] if r["strand"] >= 0 else -1 for r in records]
    over = dict(fields, n_ops=fields["n_ops"].clone())
    over["n_ops"][5] = CAP + 3
    with pytest.raises(B.BgsaHipError, match=rf"hit of read 5 has {CAP + 3} runs, its row holds {CAP} \(raise cigar_cap\)"):
        mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), over, batch.keep[5])
    off = dict(fields, ref_end=fields["ref_end"].clone())
    off["ref_end"][6] += 1
    with pytest.raises(B.BgsaHipError, match="1 malformed records, the first the one of read 6"):
        mapper.sam_records("crafted", rows, None, names, offsets, np.frombuffer(RNAME, np.uint8), off, batch.keep[5])


# ---- 2. the MAPQ kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 3, 64))
@pytest.mark.parametrize("bound", (-1, 3))
def test_list_mapq_equals_the_model(torch_gpu, k, bound):
    torch = torch_gpu
    rng = np.random.default_rng(64 * k + bound)
    ns, rows = 130, 134                 # 130 reads: 33 workgroups, the last one half empty; four rows behind them
    distances = np.sort(rng.integers(0, 5 if k > 3 else 9, size=(rows, k)), axis=1)
    distances[:20] = distances[:20, :1] + (np.arange(k) >= rng.integers(1, k + 1, size=(20, 1)))       # n1 from 1 up to k
    keep = (rng.random((rows, k)) < 0.7).astype(np.int32)
    keep[20:24], keep[24:28] = 0, 1
    scores = (-distances).astype(np.int32)
    outs = [torch.full((rows,), -77, dtype=torch.int32, device="cuda") for _ in range(4)]
    d_scores, d_keep = torch.from_numpy(scores).cuda(), torch.from_numpy(keep).cuda()
    B.check(B.lib().bgsa_hip_sam_mapq_dev(d_scores.data_ptr(), d_keep.data_ptr(), ns, k, bound, *(x.data_ptr() for x in outs), None), "sam_mapq_dev")
    torch.cuda.synchronize()
    got = np.stack([x.cpu().numpy() for x in outs], axis=1)
    want = np.array([S.list_fields(scores[c], keep[c], bound) for c in range(ns)])
    assert np.array_equal(got[:ns], want), np.argwhere(got[:ns] != want)[:5].tolist()
    assert (got[ns:] == -77).all(), "a row beyond ns was written"
    if k == 64:
        assert {0, 1, 2, 3} <= set(want[:, 1].tolist()) and want[:, 2].max() >= 10


# ---- 3. and 4. the entry points on the case of test_pair_map_gpu.py ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def case(torch_gpu):
    ref, reads1, reads2, kinds, _ = PM.make_case()
    rng = np.random.default_rng(7)
    extra = ACGT[rng.integers(4, size=(2, 6, PM.N))]      # four pairs of unrelated ends: both ends unmapped ...
    extra[0, 4] = ref[PM.COPIES[0] + 4: PM.COPIES[0] + 4 + PM.N]      # ... and two whose end 1 lies inside the repeated unit, on either strand
    extra[0, 5] = np.frombuffer(S.reverse_complement(ref[PM.COPIES[2] + 8: PM.COPIES[2] + 8 + PM.N].tobytes()), np.uint8)
    reads1, reads2 = np.concatenate((reads1, extra[0])), np.concatenate((reads2, extra[1]))
    names = [f"pair{c}/{kind}".encode() for c, kind in enumerate(list(kinds) + ["nowhere"] * 4 + ["in-the-repeat"] * 2)]
    quals = [bytes(rng.integers(33, 127, size=PM.N, dtype=np.uint8)) for _ in range(2 * len(names))]
    return dict(ref=ref, reference=ref.tobytes(), reads=(reads1, reads2), names=names, quals=(quals[::2], quals[1::2]),
                mapper=B.ReferenceMapper(ref, PM.W, PM.S))


def lines_of(records: B.SamRecords) -> list:
    text = records.text.tobytes()
    return [text[records.offsets[i]: records.offsets[i + 1]] for i in range(records.offsets.size - 1)]


def assert_records(got: B.SamRecords, want: tuple, what: str) -> None:
    lines, flag, pos, mapq, nm = want
    got_lines = lines_of(got)
    assert len(got_lines) == len(lines), what
    for i, (mine, theirs) in enumerate(zip(got_lines, lines)):
        assert mine == theirs, (what, i, mine, theirs)
    assert got.text.tobytes() == b"".join(lines)
    for name, column in (("flag", flag), ("pos", pos), ("mapq", mapq), ("nm", nm)):
        assert getattr(got, name).tolist() == column, (what, name)


def test_map_reads_sam_equals_the_model_on_the_existing_entry_points(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    seen = dict(forward=0, reverse=0, unmapped=0, repeated=0, sixty=0, between=0)
    for k_best in (2, 6):
        for seeded in (True, False):
            hits = mapper.map_reads_seeded(reads, k_best, PM.MAX_DISTANCE) if seeded else mapper.map_reads(reads, k_best, PM.MAX_DISTANCE)
            want = S.single_records(hits, reads, names, quals, case["reference"], RNAME, PM.MAX_DISTANCE if seeded else -1)
            got = mapper.map_reads_sam(reads, names, quals, RNAME, k_best=k_best, max_distance=PM.MAX_DISTANCE, seeded=seeded)
            assert_records(got, want, f"k_best {k_best}, seeded {seeded}")
            small = mapper.map_reads_sam(reads, names, quals, RNAME, k_best=k_best, max_distance=PM.MAX_DISTANCE, seeded=seeded, block_rows=7)
            assert small.text.tobytes() == got.text.tobytes() and np.array_equal(small.offsets, got.offsets), "block_rows changes the bytes"
            for c in range(reads.shape[0]):
                _, mapq, n1, _ = S.list_fields(hits.scores[c], hits.keep[c], PM.MAX_DISTANCE if seeded else -1)
                seen["forward"] += got.flag[c] == 0
                seen["reverse"] += got.flag[c] == 16
                seen["unmapped"] += got.flag[c] == 4
                seen["repeated"] += n1 >= 2 and got.mapq[c] == S.table(n1)
                seen["sixty"] += n1 == 1 and got.mapq[c] == 60
                seen["between"] += n1 == 1 and 3 < got.mapq[c] < 60
    assert all(seen.values()), seen
    plain = mapper.map_reads_sam(reads, k_best=2, max_distance=PM.MAX_DISTANCE)      # default names, no QUAL, the default reference name
    first = lines_of(plain)[0].split(b"\t")
    assert first[0] == b"r0" and first[10].rstrip(b"\n") == b"*" and first[2] in (b"ref", b"*")


def test_map_reads_sam_on_mixed_lengths(case):
    mapper, rng = case["mapper"], np.random.default_rng(24)
    cut = rng.integers(24, PM.N + 1, size=case["reads"][0].shape[0])
    cut[:2] = (24, PM.N)
    reads = [bytes(row[:n]) for row, n in zip(case["reads"][0], cut)]
    quals = [q[:n] for q, n in zip(case["quals"][0], cut)]
    for seeded in (True, False):
        entry = mapper.map_reads_seeded_ragged if seeded else mapper.map_reads_ragged
        hits = entry(reads, 2, PM.MAX_DISTANCE)
        want = S.single_records(hits, reads, case["names"], quals, case["reference"], RNAME, PM.MAX_DISTANCE if seeded else -1)
        got = mapper.map_reads_sam(reads, case["names"], quals, RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, seeded=seeded)
        assert_records(got, want, f"mixed lengths, seeded {seeded}")
        assert (got.flag != 4).sum() > 20


def test_map_pairs_sam_equals_the_model_on_map_pairs(case):
    mapper, (reads1, reads2), (quals1, quals2) = case["mapper"], case["reads"], case["quals"]
    args = dict(k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    paired = mapper.map_pairs(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, **args)
    want = S.pair_records(paired, reads1, reads2, case["names"], quals1, quals2, case["reference"], RNAME, (PM.RESCUE_DISTANCE,) * 2)
    got = mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, case["names"], quals1, quals2, RNAME, **args)
    assert_records(got, want, "pairs")
    small = mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, case["names"], quals1, quals2, RNAME, block_rows=7, **args)
    assert small.text.tobytes() == got.text.tobytes()
    mapped1, mapped2, proper = paired.slot1 >= 0, paired.slot2 >= 0, paired.proper == 1
    pairs = np.arange(proper.size)
    through = proper & (paired.rescued1[pairs, np.maximum(paired.slot1, 0)] | paired.rescued2[pairs, np.maximum(paired.slot2, 0)])
    kinds = dict(proper=proper.sum(), improper_both_mapped=(~proper & mapped1 & mapped2).sum(), one_unmapped=(mapped1 != mapped2).sum(),
                 both_unmapped=(~mapped1 & ~mapped2).sum(), proper_through_rescue=through.sum())
    assert all(kinds.values()), kinds
    flags = got.flag.reshape(-1, 2)
    assert ((flags[:, 0] & 64) == 64).all() and ((flags[:, 1] & 128) == 128).all() and (((flags & 2) == 2) == proper[:, None]).all()
    paired = mapper.map_pairs(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, seeded=False, **args)      # stage A exhaustive, blanked
    want = S.pair_records(paired, reads1, reads2, case["names"], quals1, quals2, case["reference"], RNAME, (PM.RESCUE_DISTANCE,) * 2)
    assert_records(mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, case["names"], quals1, quals2, RNAME, seeded=False, **args),
                   want, "pairs, stage A exhaustive")
    bare = mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, **args)
    assert lines_of(bare)[3].startswith(b"r1\t") and lines_of(bare)[3].split(b"\t")[10].rstrip(b"\n") == b"*"


def test_a_sam_call_leaves_no_state_behind(case):
    mapper, (reads1, reads2) = case["mapper"], case["reads"]

    def public():
        single = mapper.map_reads_seeded(reads1, 2, PM.MAX_DISTANCE)
        paired = mapper.map_pairs(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, k_best=1, max_distance=PM.MAX_DISTANCE,
                                  rescue_distance=PM.RESCUE_DISTANCE)
        return single, paired, dict(mapper.last_pair_stats)

    def same_hits(a, b):
        return all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a[:5] + (a.windows,), b[:5] + (b.windows,))) and a.cigars == b.cigars
    before = public()
    mapper.map_reads_sam(reads1, k_best=2, max_distance=PM.MAX_DISTANCE)
    mapper.map_reads_sam([bytes(r[: 24 + i % 9]) for i, r in enumerate(reads1)], k_best=2, max_distance=PM.MAX_DISTANCE, seeded=False)
    mapper.map_pairs_sam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, k_best=1, max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE)
    after = public()
    assert same_hits(before[0], after[0]) and same_hits(before[1].end1, after[1].end1) and same_hits(before[1].end2, after[1].end2)
    for x, y in zip(before[1][2:], after[1][2:]):
        assert x.dtype == y.dtype and np.array_equal(x, y)
    assert before[2] == after[2]

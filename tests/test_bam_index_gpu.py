"""Coordinate-sorted BAM and its BAI index on the MI355X: the key kernel on crafted records (one sequence and three contigs) and
the two index kernels on synthetic sorted coordinates, array for array against tests/bai_reference.py, with sentinels around
every output; then map_reads_bam / map_pairs_bam with sort=True — the records are the unsorted call's in key order, the index and
the .bai bytes are the model's, and region queries on the written files return exactly the records that overlap."""
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bai_reference as R  # noqa: E402
import bam_reference as M  # noqa: E402
import contig_reference as C  # noqa: E402
import test_bam_gpu as TB  # noqa: E402
import test_bam_index_cpu as TC  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402
from test_bam_gpu import case, crafted, torch_gpu  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

GUARD = 8             # sentinel entries in front of and behind every output array
INT64_MAX = 2 ** 63 - 1


class Fenced:
    """A device array of n entries between GUARD sentinel entries on either side."""

    def __init__(self, torch, n: int, dtype, fill=None):
        self.n, self.sent = n, -0x5A5A5A5 if fill is None else fill
        self.whole = torch.full((n + 2 * GUARD,), self.sent, dtype=dtype, device="cuda")
        self.ptr = self.whole.data_ptr() + GUARD * self.whole.element_size()

    def host(self) -> np.ndarray:
        host = self.whole.cpu().numpy()
        assert (host[:GUARD] == self.sent).all() and (host[GUARD + self.n:] == self.sent).all(), "an entry outside the output was written"
        return host[GUARD: GUARD + self.n]

    def set(self, value) -> None:
        self.whole[GUARD: GUARD + self.n] = value


# ---- 1. the key kernel on crafted records ------------------------------------------------------------------------------------------
BATCH_KEY = dict(strand="strand", rnext="rnext", pnext="pnext", ref_begin="begin", ref_end="end", flag="flag")


def key_records(records, contigs: bool) -> tuple:
    """(the records, {(field, i): value} making one record malformed per rule, the dicts as the model sees them)."""
    records = [dict(r) for r in (TB.as_contig_records(records) if contigs else records)]
    mapped = [i for i, r in enumerate(records) if r["strand"] >= 0]
    twin = dict(records[mapped[3]])                           # two records at one position on opposite strands, reverse first
    records += [dict(twin, flag=16, name=b"twin-r"), dict(twin, flag=0, name=b"twin-f")]
    mate = records[mapped[4]]                                 # an unmapped end beside its mate: it takes the mate's place
    records.append(dict(records[-3], name=b"beside", rnext=1, pnext=mate["begin"] + 1, flag=69))
    assert records[-1]["strand"] == -1
    unmapped = [i for i, r in enumerate(records) if r["strand"] < 0 and r["rnext"] == 1]
    victims = iter(mapped[5:])
    over = {("strand", next(victims)): 2, ("strand", next(victims)): -2, ("rnext", next(victims)): 2, ("rnext", next(victims)): -1,
            ("pnext", next(victims)): -1, ("ref_begin", next(victims)): -1, ("ref_end", next(victims)): TB.CRAFT_LEN + 1}
    i = next(victims)
    over[("ref_end", i)] = records[i]["begin"] - 1
    i = next(victims)
    over[("rnext", i)], over[("pnext", i)] = 1, 0             # rnext 1 with pnext < 1
    if contigs:
        i = next(victims)
        over[("ref_begin", i)] = 18_500                       # on padding
        i = next(victims)
        over[("ref_end", i)] = sum(TB.CONTIGS[TB.contig_of(records[i]["begin"])[0]][1:]) + 1      # beyond its contig
        over[("pnext", unmapped[0])] = 19_000 + 1             # the mate on padding
    else:
        over[("pnext", unmapped[0])] = 2 ** 29 + 1            # pos + 1 beyond a BAI's reach
        over[("pnext", unmapped[1])] = 2 ** 29                # ... and the last position inside it: well-formed
    seen = [dict(r) for r in records]
    for (field, i), value in over.items():
        seen[i][BATCH_KEY[field]] = value
    return records, over, seen


@pytest.mark.parametrize("contigs", (False, True))
def test_keys_and_coordinates_equal_the_model(torch_gpu, crafted, contigs):
    torch, L = torch_gpu, B.lib()
    _, mapper, records = crafted
    records, over, seen = key_records(records, contigs)
    table = [(start, n) for _, start, n in TB.CONTIGS] if contigs else None
    clean = [R.coordinates(r, TB.CRAFT_LEN, table) for r in records]
    want = [R.coordinates(r, TB.CRAFT_LEN, table) for r in seen]
    bad = {i for _, i in over} - ({i for (f, i), v in over.items() if f == "pnext" and v == 2 ** 29})
    assert [i for i, w in enumerate(want) if w == R.UNPLACED] == sorted(bad) and len(bad) == (12 if contigs else 10)
    assert all(c != R.UNPLACED for c in clean)
    assert {c[1] for c in clean} >= ({-1, 0, 1, 2} if contigs else {-1, 0})
    assert clean[-3][0] == clean[-2][0] + 1 and clean[-3][1:] == clean[-2][1:]      # the twins: one position, the reverse one's key + 1
    assert clean[-1][1:4] == (R.coordinates(records[[i for i, r in enumerate(records) if r["strand"] >= 0][4]], TB.CRAFT_LEN, table)[1:3] +
                              (clean[-1][2] + 1,))
    for use, expect, count in ((None, clean, 0), (over, want, len(bad))):
        batch = TB.Batch(torch, mapper, records, None, over=use)
        n = batch.n
        key = Fenced(torch, n, torch.int64)
        ref_id, pos, end, bin_ = (Fenced(torch, n, torch.int32) for _ in range(4))
        counter = Fenced(torch, 1, torch.int32)
        counter.set(0)
        call = (L.bgsa_hip_bam_coordinates_contigs_dev, (batch.struct, batch.table)) if contigs else (L.bgsa_hip_bam_coordinates_dev, (batch.struct,))
        B.check(call[0](*call[1], n, key.ptr, ref_id.ptr, pos.ptr, end.ptr, bin_.ptr, counter.ptr, None), "bam_coordinates_dev")
        torch.cuda.synchronize()
        got = list(zip(key.host().tolist(), ref_id.host().tolist(), pos.host().tolist(), end.host().tolist(), bin_.host().tolist()))
        for i, (g, w) in enumerate(zip(got, expect)):
            assert g == w, (contigs, i, g, w)
        assert counter.host().tolist() == [count]
    assert L.bgsa_hip_bam_coordinates_dev(batch.struct, 0, key.ptr, ref_id.ptr, pos.ptr, end.ptr, bin_.ptr, counter.ptr, None) == 0
    assert L.bgsa_hip_bam_coordinates_dev(batch.struct, n, key.ptr, None, pos.ptr, end.ptr, bin_.ptr, counter.ptr, None) == -1
    assert L.bgsa_hip_bam_coordinates_dev(batch.struct, -1, key.ptr, ref_id.ptr, pos.ptr, end.ptr, bin_.ptr, counter.ptr, None) == -1
    assert L.bgsa_hip_bam_coordinates_contigs_dev(batch.struct, None, n, key.ptr, ref_id.ptr, pos.ptr, end.ptr, bin_.ptr, counter.ptr, None) == -1
    torch.cuda.synchronize()
    assert counter.host().tolist() == [len(bad)] and key.host().tolist() == [w[0] for w in want]      # a refused call wrote nothing


# ---- 2. the index kernels on synthetic sorted coordinates --------------------------------------------------------------------------------
def run_index(torch, s: dict, P: int, block_offsets, ref_lens, payload_bytes=None, n_blocks=None) -> dict:
    """marks -> cumsum -> chunks on the coordinates s (ref_id, pos, end, bin, offsets), every output fenced."""
    L = B.lib()
    n = len(s["ref_id"])
    up = lambda x, dtype: torch.from_numpy(np.concatenate((np.asarray(x, dtype), np.zeros(1, dtype)))).cuda()      # noqa: E731  never empty
    d = [up(s[k], np.int32) for k in ("ref_id", "pos", "end", "bin")]
    offsets = torch.from_numpy(np.asarray(s["offsets"], np.int64)).cuda()
    payload_bytes = int(s["offsets"][-1]) if payload_bytes is None else payload_bytes
    n_blocks = -(-payload_bytes // P) if n_blocks is None else n_blocks
    blocks = None if block_offsets is None else torch.from_numpy(np.asarray(block_offsets, np.int64)).cuda()
    base = np.zeros(len(ref_lens) + 1, np.int64)
    windows = int(L.bgsa_hip_bam_index_windows(np.asarray(ref_lens, np.int64).ctypes.data, len(ref_lens), base.ctypes.data))
    d_base = torch.from_numpy(base).cuda()
    beg, end = Fenced(torch, n, torch.int64), Fenced(torch, n, torch.int64)
    starts = Fenced(torch, n, torch.int32)
    linear = Fenced(torch, windows, torch.int64)
    linear.set(INT64_MAX)
    refused = Fenced(torch, 2, torch.int32)
    refused.set(0)
    B.check(L.bgsa_hip_bam_index_marks_dev(*(x.data_ptr() for x in d), n, offsets.data_ptr(), payload_bytes, P,
                                           None if blocks is None else blocks.data_ptr(), n_blocks, d_base.data_ptr(), len(ref_lens), beg.ptr,
                                           end.ptr, starts.ptr, linear.ptr, refused.ptr, None), "bam_index_marks_dev")
    torch.cuda.synchronize()
    flags = starts.host().copy()
    out = dict(voff_beg=beg.host().tolist(), voff_end=end.host().tolist(), chunk_start=flags.tolist(), raw_linear=linear.host().tolist(),
               refused=refused.host().tolist(), sent=beg.sent)
    if out["refused"][0]:
        return out
    chunk_of = torch.cumsum(starts.whole[GUARD: GUARD + n], 0, dtype=torch.int64) if n else torch.zeros(1, dtype=torch.int64, device="cuda")
    n_chunks = int(chunk_of[-1].item()) if n else 0
    c_ref, c_bin = Fenced(torch, n_chunks, torch.int32), Fenced(torch, n_chunks, torch.int32)
    c_beg, c_end = Fenced(torch, n_chunks, torch.int64), Fenced(torch, n_chunks, torch.int64)
    B.check(L.bgsa_hip_bam_index_chunks_dev(d[0].data_ptr(), d[3].data_ptr(), beg.ptr, end.ptr, starts.ptr, chunk_of.data_ptr(), n, n_chunks,
                                            c_ref.ptr, c_bin.ptr, c_beg.ptr, c_end.ptr, refused.ptr + 4, None), "bam_index_chunks_dev")
    torch.cuda.synchronize()
    chunks = list(zip(c_ref.host().tolist(), c_bin.host().tolist(), c_beg.host().tolist(), c_end.host().tolist()))
    out.update(chunks=sorted(chunks, key=lambda x: x[:2]), refused=refused.host().tolist())      # Python's sort is stable
    return out


def assert_index_equals_the_model(got: dict, s: dict, P: int, block_offsets, ref_lens, what) -> None:
    want = R.build_index(s["ref_id"], s["pos"], s["end"], s["bin"], s["offsets"], P, block_offsets, ref_lens)
    assert got["refused"] == [0, 0], what
    for name in ("voff_beg", "voff_end", "chunk_start", "raw_linear", "chunks"):
        assert got[name] == want[name], (what, name)


def made_up_blocks(payload_bytes: int, P: int, seed: int) -> list:
    """A monotone array of n_blocks + 1 block offsets no framing ever gave."""
    sizes = np.random.default_rng(seed).integers(29, P + 32, size=-(-payload_bytes // P))
    return np.concatenate(([0], np.cumsum(sizes))).tolist()


@pytest.mark.parametrize("P", (61, 65280))
@pytest.mark.parametrize("made_up", (False, True))
def test_marks_and_chunks_equal_the_model(torch_gpu, P, made_up):
    s = TC.synthetic()
    k = len(s["ref_id"]) // 2                                 # one record ends exactly on a block boundary, and so does the payload
    lengths = np.diff(s["offsets"])
    lengths[k] += -int(s["offsets"][k + 1]) % P
    lengths[-1] += -int(lengths.sum()) % P
    s = dict(s, offsets=np.concatenate(([0], np.cumsum(lengths))))
    total = int(s["offsets"][-1])
    assert s["offsets"][k + 1] % P == 0 and total % P == 0 and s["ref_id"][k] >= 0
    blocks = made_up_blocks(total, P, P) if made_up else None
    assert_index_equals_the_model(run_index(torch_gpu, s, P, blocks, TC.REF_LENS), s, P, blocks, TC.REF_LENS, "synthetic")
    nowhere = {k: v[s["ref_id"] < 0] for k, v in s.items() if k != "offsets"}
    for name, part in (("n = 0", {k: v[:0] for k, v in nowhere.items()}), ("n = 1", {k: v[:1] for k, v in s.items() if k != "offsets"}),
                       ("every refID -1", nowhere), ("one reference", {k: v[s["ref_id"] == 1] for k, v in s.items() if k != "offsets"})):
        n = len(part["ref_id"])
        part = dict(part, offsets=np.arange(n + 1, dtype=np.int64) * P if n < 2 else np.concatenate(([0], np.cumsum(lengths[:n]))))
        some = made_up_blocks(int(part["offsets"][-1]), P, 5) if made_up else None
        got = run_index(torch_gpu, part, P, some, TC.REF_LENS)
        assert_index_equals_the_model(got, part, P, some, TC.REF_LENS, name)
        assert name != "every refID -1" or (got["chunks"] == [] and set(got["raw_linear"]) == {INT64_MAX} and n == 60)


def test_marks_refuses_what_is_out_of_order_or_out_of_range(torch_gpu):
    ref_lens, P = (100_000, 50_000), 256
    pos = np.array([10, 20_000, 40_000, 70_000, 5, 30_000])
    good = dict(ref_id=np.array([0, 0, 0, 0, 1, 1]), pos=pos, end=pos + 100, offsets=np.arange(7, dtype=np.int64) * 100)
    good["bin"] = np.array([M.reg2bin(int(p), int(p) + 100) for p in pos])
    assert_index_equals_the_model(run_index(torch_gpu, good, P, None, ref_lens), good, P, None, ref_lens, "well-formed")

    def changed(**over):
        out = {k: v.copy() for k, v in good.items()}
        for name, (i, value) in over.items():
            out[name][i] = value
        return out
    cases = {"an unsorted pair": (changed(pos=(2, 15_000), end=(2, 15_100)), 2), "refID = n_refs": (changed(ref_id=(5, 2)), 5),
             "a non-monotone offset": (changed(offsets=(3, 150)), 2), "refID < -1": (changed(ref_id=(5, -2)), 5),
             "end <= pos": (changed(end=(1, 20_000)), 1), "pos < 0": (changed(pos=(4, -1)), 4),
             "beyond the reference's windows": (changed(end=(5, 50_000 + 16_384)), 5), "an offset beyond the payload": (changed(offsets=(6, 601)), 5)}
    for what, (s, victim) in cases.items():
        payload = 600
        got = run_index(torch_gpu, s, P, None, ref_lens, payload_bytes=payload)
        assert got["refused"] == [1, 0], what
        assert got["chunk_start"][victim] == 0 and got["voff_beg"][victim] == got["sent"] and got["voff_end"][victim] == got["sent"], what
        window = int(R.windows(ref_lens)[good["ref_id"][victim]] + (good["pos"][victim] >> 14))      # only the victim covers it
        assert got["raw_linear"][window] == INT64_MAX, what
        others = [i for i in range(6) if i != victim]
        assert [got["voff_beg"][i] for i in others] == [R.virtual_offset(int(s["offsets"][i]), P) for i in others], what
    got = run_index(torch_gpu, good, P, None, ref_lens, n_blocks=1)      # the last record ends in block 600 // 256 = 2, beyond n_blocks
    assert got["refused"] == [1, 0] and got["voff_beg"][5] == got["sent"] and got["voff_beg"][4] == R.virtual_offset(400, P)


def test_chunks_refuses_a_scan_that_is_not_the_flags(torch_gpu):
    torch, L = torch_gpu, B.lib()
    ref_id = torch.tensor([0, 0, 0, -1], dtype=torch.int32, device="cuda")
    bins = torch.tensor([4681, 4681, 4682, 4680], dtype=torch.int32, device="cuda")
    voff = torch.arange(5, dtype=torch.int64, device="cuda") * 100
    starts = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device="cuda")
    chunk_of = torch.tensor([1, 1, 3, 3], dtype=torch.int64, device="cuda")      # record 2 names chunk 3 of 2
    outs = [Fenced(torch, 2, dtype) for dtype in (torch.int32, torch.int32, torch.int64, torch.int64)]
    refused = Fenced(torch, 1, torch.int32)
    refused.set(0)
    B.check(L.bgsa_hip_bam_index_chunks_dev(ref_id.data_ptr(), bins.data_ptr(), voff.data_ptr(), voff[1:].data_ptr(), starts.data_ptr(),
                                            chunk_of.data_ptr(), 4, 2, *(x.ptr for x in outs), refused.ptr, None), "bam_index_chunks_dev")
    torch.cuda.synchronize()
    assert refused.host().tolist() == [1]
    assert [x.host().tolist()[0] for x in outs] == [0, 4681, 0, 200] and all(x.host().tolist()[1] == x.sent for x in outs)


# ---- 3. the entry points ---------------------------------------------------------------------------------------------------------------
def block_starts(blocks: bytes) -> list:
    out, at = [0], 0
    while at < len(blocks):
        at += struct.unpack_from("<H", blocks, at + 16)[0] + 1
        out.append(at)
    return out


def grid(n: int) -> list:
    step = max(n // 7, 1)
    cuts = sorted({0, 1, n - 1, n, *range(0, n, step), *(x for x in (16_383, 16_384, 32_767, 32_768) if x < n)})
    return [(a, b) for a in cuts for b in cuts if a < b][:: max(1, len(cuts) // 6)] + [(0, n), (n - 1, n)]


def check_sorted(got, plain, mapper, ref_names, P: int, compress: bool, tmp_path, what: str) -> list:
    """Everything item 3 of the issue's GPU checks asks of one sort=True call against the sort=False call of the same reads."""
    assert isinstance(got, B.SortedBamRecords) and isinstance(plain, B.BamRecords), what
    blocks = got.blocks.tobytes()
    pieces = M.walk_blocks(blocks, stored=not compress)
    assert all(len(x) == P for x in pieces[:-1]) and 1 <= len(pieces[-1]) <= P, what
    records = M.split_records(b"".join(pieces))
    unsorted = M.split_records(b"".join(M.walk_blocks(plain.blocks.tobytes())))
    n = len(unsorted)
    assert sorted(got.order.tolist()) == list(range(n)) and got.order.dtype == np.int64, what
    assert records == [unsorted[i] for i in got.order], what                   # the same bytes per record
    assert got.offsets.tolist() == np.concatenate(([0], np.cumsum([len(x) for x in records]))).tolist(), what
    for name in ("flag", "pos", "mapq", "nm"):
        assert np.array_equal(getattr(got, name), getattr(plain, name)[got.order]) and getattr(got, name).dtype == getattr(plain, name).dtype, (what, name)
    decoded = [M.decode(x, ref_names) for x in records]
    coords = [R.decoded_coordinates(d) for d in decoded]
    keys = [c[0] for c in coords]
    assert all(a < b or (a == b and i < j) for a, b, i, j in zip(keys, keys[1:], got.order, got.order[1:])), what      # stable
    refs = [c[1] for c in coords]
    assert got.ref_id.tolist() == refs and got.ref_id.dtype == np.int32 and refs == sorted(refs, key=lambda r: (r < 0, r)), what
    assert [d["bin"] for d in decoded] == [c[4] & 0xffff for c in coords], what
    ref_lens = mapper.index_ref_lens().tolist()
    starts = block_starts(blocks)
    assert compress or starts == [min(b * (P + 31), len(blocks)) for b in range(len(starts))], what
    want = R.build_index(refs, [c[2] for c in coords], [c[3] for c in coords], [c[4] for c in coords], got.offsets, P,
                         starts if compress else None, ref_lens)
    index = got.index
    assert list(zip(index.chunk_ref.tolist(), index.chunk_bin.tolist(), index.chunk_beg.tolist(), index.chunk_end.tolist())) == want["chunks"], what
    assert index.window_base.tolist() == want["window_base"] and index.linear.tolist() == want["linear"] and index.n_intv.tolist() == want["n_intv"], what
    assert index.ref_lens.tolist() == ref_lens, what
    header = mapper.bam_header(ref_names[0], sort_order="coordinate")
    base = len(B.bgzf_blocks(header))
    flags = [d["flag"] for d in decoded]
    assert B.bai_bytes(index, got.flag, got.ref_id, base) == R.bai_bytes(want, flags, refs, base), what
    path = tmp_path / "sorted.bam"
    B.write_bam(path, header, got, index=True)
    data, bai = path.read_bytes(), (tmp_path / "sorted.bam.bai").read_bytes()
    assert bai == R.bai_bytes(want, flags, refs, base) and data == B.bgzf_blocks(header) + blocks + B.BGZF_EOF, what
    parsed = R.parse_bai(bai)
    assert parsed["n_no_coor"] == refs.count(-1), what
    of_record = dict(zip(records, coords))
    assert len(of_record) == n, what
    sizes = set()
    for ref, length in enumerate(ref_lens):
        for beg, end in grid(length):
            hit = [x for x in R.fetch(data, R.query(parsed, ref, beg, end)) if of_record[x][1] == ref and of_record[x][2] < end and of_record[x][3] > beg]
            assert hit == [records[i] for i in R.overlaps(refs, [c[2] for c in coords], [c[3] for c in coords], ref, beg, end)], (what, ref, beg, end)
            sizes.add(len(hit))
    assert len(sizes) >= 3 and max(sizes) >= 2, (what, sizes)      # the regions found nothing, something and more
    return decoded


def straddles(offsets, P: int) -> bool:
    """Whether some record lies in two blocks of P payload bytes."""
    return bool((offsets[:-1] // P != (offsets[1:] - 1) // P).any())


@pytest.fixture(scope="module")
def plain_calls(case):
    """The sort=False calls every sorted one is compared with, once."""
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    single = mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, k_best=2, max_distance=PM.MAX_DISTANCE)
    pairs = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                                 rescue_distance=PM.RESCUE_DISTANCE)
    return single, pairs


@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("small", (False, True))
def test_map_reads_bam_sorted(case, plain_calls, tmp_path, compress, small):
    mapper, reads, names, quals = case["mapper"], case["reads"][0], case["names"], case["quals"][0]
    plain = plain_calls[0]
    got = mapper.map_reads_bam(reads, names, quals, TB.RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, compress=compress, sort=True,
                               block_payload=61 if small else 65280)
    P = 61 if small else 65280
    assert not small or straddles(got.offsets, P)
    decoded = check_sorted(got, plain, mapper, [TB.RNAME], P, compress, tmp_path, f"single, {P}, compress={compress}")
    assert {d["flag"] for d in decoded} >= {0, 4, 16} and decoded[-1]["ref_id"] == -1 and decoded[0]["ref_id"] == 0


@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("small", (False, True))
def test_map_pairs_bam_sorted(case, plain_calls, tmp_path, compress, small):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    plain = plain_calls[1]
    P = 61 if small else 65280
    got = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                               rescue_distance=PM.RESCUE_DISTANCE, compress=compress, sort=True, block_payload=P)
    decoded = check_sorted(got, plain, mapper, [TB.RNAME], P, compress, tmp_path, f"pairs, {P}, compress={compress}")
    assert not small or straddles(got.offsets, P)
    beside = [i for i, d in enumerate(decoded) if d["flag"] & 4 and d["ref_id"] == 0]      # an unmapped end at its mate's position: next to it,
    assert beside and all(any(decoded[j]["name"] == decoded[i]["name"] and not decoded[j]["flag"] & 4 and decoded[j]["pos"] == decoded[i]["pos"]
                              for j in (i - 1, i + 1)) for i in beside)                     # behind a forward mate (a tie), in front of a reverse one
    assert any(decoded[i - 1]["name"] == decoded[i]["name"] and not decoded[i - 1]["flag"] & 20 for i in beside)
    assert sum(d["ref_id"] < 0 for d in decoded) >= 8 and all(d["ref_id"] < 0 for d in decoded[-8:])      # the four unmapped pairs, last


@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("small", (False, True))
def test_the_contig_form_sorted(torch_gpu, tmp_path, compress, small):
    F, Pr = C.FIXTURE, C.PAIRS
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=Pr["PADDING"])
    order = list(F["NAMES"])
    reads = np.array([list(read) for _, _, read in C.crafted(sequences)], dtype=np.uint8)
    args = dict(k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    plain = mapper.map_reads_bam(reads, **args)
    P = 61 if small else 65280
    got = mapper.map_reads_bam(reads, compress=compress, sort=True, block_payload=P, **args)
    decoded = check_sorted(got, plain, mapper, order, P, compress, tmp_path, f"contigs, single, {P}, compress={compress}")
    assert len({d["ref_id"] for d in decoded} - {-1}) >= 3
    pairs = C.crafted_pairs(sequences)
    reads1, reads2 = (np.array([list(x[e]) for x in pairs], dtype=np.uint8) for e in (1, 2))
    pair_args = dict(k_best=Pr["K_BEST"], max_distance=F["MAX_DISTANCE"])
    plain = mapper.map_pairs_bam(reads1, reads2, Pr["INSERT_MIN"], Pr["INSERT_MAX"], [b"proper", b"across", b"half"], **pair_args)
    got = mapper.map_pairs_bam(reads1, reads2, Pr["INSERT_MIN"], Pr["INSERT_MAX"], [b"proper", b"across", b"half"], compress=compress, sort=True,
                               block_payload=P, **pair_args)
    check_sorted(got, plain, mapper, order, P, compress, tmp_path, f"contigs, pairs, {P}, compress={compress}")


# ---- 4. a mapper-made record across a linear window ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", (False, True))
def test_reads_across_the_windows_of_a_longer_reference(torch_gpu, tmp_path, compress):
    rng = np.random.default_rng(40)
    ref = TB.ACGT[rng.integers(4, size=40_000)].copy()
    mapper = B.ReferenceMapper(ref, PM.W, PM.S)
    n, reads = 32, []
    for i in range(24):
        edge = (16_384, 32_768)[i % 2]
        begin = edge - (1, 5, n // 2, n - 1, n, 300)[i % 6] - (i // 12)
        read = ref[begin: begin + n].copy()
        reads.append(M.S.reverse_complement(read.tobytes()) if i % 3 == 0 else read.tobytes())
    reads = np.array([list(x) for x in reads], dtype=np.uint8)
    args = dict(k_best=2, max_distance=1)
    plain = mapper.map_reads_bam(reads, **args)
    got = mapper.map_reads_bam(reads, compress=compress, sort=True, block_payload=256, **args)
    decoded = check_sorted(got, plain, mapper, [b"ref"], 256, compress, tmp_path, f"40,000 bp, compress={compress}")
    coords = [R.decoded_coordinates(d) for d in decoded]
    assert all(not d["flag"] & 4 for d in decoded)
    assert sum(c[2] >> 14 != (c[3] - 1) >> 14 for c in coords) >= 8 and {585} <= {c[4] for c in coords}       # across a window: a level-4 bin
    assert got.index.n_intv.tolist() == [3] and {c[4] for c in coords} >= {4681, 4682}


# ---- 5. nothing moved ---------------------------------------------------------------------------------------------------------------------
def test_sort_false_is_the_call_without_the_argument(case, plain_calls):
    mapper, (reads1, reads2), (quals1, quals2), names = case["mapper"], case["reads"], case["quals"], case["names"]
    single = mapper.map_reads_bam(reads1, names, quals1, TB.RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, sort=False)
    pairs = mapper.map_pairs_bam(reads1, reads2, PM.INSERT_MIN, PM.INSERT_MAX, names, quals1, quals2, TB.RNAME, k_best=1, max_distance=PM.MAX_DISTANCE,
                                 rescue_distance=PM.RESCUE_DISTANCE, sort=False)
    for got, want in zip((single, pairs), plain_calls):
        assert type(got) is type(want) is B.BamRecords
        assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))
    with pytest.raises(B.BgsaHipError, match="sort 1 is not a bool"):
        mapper.map_reads_bam(reads1, names, k_best=2, max_distance=PM.MAX_DISTANCE, sort=1)

"""The merge of many calls' BAM records on the MI355X: the gather kernel on random bytes against tests/bam_merge_reference.py —
every window of a grid, with and without flags, sentinels around every output —; its refusals per record; then map_reads_bam /
map_pairs_bam with merge= in three unequal batches against ONE sort=True call on all reads — every field, the index arrays and the
files —, duplicates whose copies arrive in a later batch, the contig form, and the edges."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bai_reference as R  # noqa: E402
import bam_merge_reference as G  # noqa: E402
import bam_reference as M  # noqa: E402
import contig_reference as C  # noqa: E402
import markdup_reference as MD  # noqa: E402
import test_bam_gpu as TB  # noqa: E402
import test_bam_index_gpu as TI  # noqa: E402
import test_markdup_gpu as TM  # noqa: E402
import test_pair_map_gpu as PM  # noqa: E402
from test_bam_gpu import case, crafted, torch_gpu  # noqa: E402,F401  (fixtures)

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 4, 5, 19, 20, 21, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4099)
GAP = 8               # sentinel bytes between the images of two windows in one output buffer


# ---- 1. the kernel against the model ---------------------------------------------------------------------------------------------------
def layout(seed: int, lengths, repeats: int) -> dict:
    """About 200 records of the given lengths, shuffled, in a random order: the source bytes and both offset arrays."""
    rng = np.random.default_rng(seed)
    lens = np.concatenate([rng.permutation(np.asarray(lengths, dtype=np.int64)) for _ in range(repeats)])
    n = lens.size
    order = rng.permutation(n).astype(np.int64)
    src_offsets = np.concatenate(([0], np.cumsum(lens)))
    dst_offsets = np.concatenate(([0], np.cumsum(lens[order])))
    src = rng.integers(0, 256, size=int(src_offsets[-1]), dtype=np.uint8)
    assert set((src_offsets[:-1] % 16).tolist()) == set(range(16)) and set((dst_offsets[:-1] % 16).tolist()) == set(range(16))
    return dict(n=n, lens=lens, order=order, src_offsets=src_offsets, dst_offsets=dst_offsets, src=src, total=int(src_offsets[-1]))


def windows_of(s: dict) -> list:
    """The grid: the whole payload, windows of 1, 61 and 256 bytes, the cuts through a chosen record, an empty window."""
    total, dst = s["total"], s["dst_offsets"]
    chosen = int(np.flatnonzero(s["lens"][s["order"]] == 257)[1])      # an output record of 257 bytes in the middle of the payload
    d, d_end = int(dst[chosen]), int(dst[chosen + 1])
    out = [(0, total)]
    out += [(p, p + 1) for p in (0, total - 1, *range(d - 2, d + 24), *range(d_end - 3, d_end + 2))]
    out += [(lo, min(lo + 61, total)) for lo in range(0, total, 61)]
    out += [(lo, min(lo + 256, total)) for lo in range(0, total, 256)]
    for cut in (d + 1, d + 18, d + 19, d + 20, d_end):          # behind the record's byte 0, 17, 18, 19 and its last byte
        out += [(max(d - 100, 0), cut), (cut, min(d_end + 100, total))]
    out.append((d + 7, d + 7))                                 # an empty window
    return out


def records_of(s: dict, lo: int, hi: int) -> tuple:
    """(first, count) of the output records that intersect [lo, hi): what the driver passes."""
    first = int(np.searchsorted(s["dst_offsets"][1:], lo, side="right"))
    behind = int(np.searchsorted(s["dst_offsets"][:-1], hi, side="left"))
    return (first, max(behind - first, 0)) if hi > lo else (0, 0)


def run_windows(torch, s: dict, windows, flag, whole_range: bool) -> None:
    """Every window's image side by side in ONE fenced buffer, GAP sentinel bytes between two; compared with the model once."""
    L = B.lib()
    d_src, src_at = TB.fenced(torch, s["total"])                # the source at an odd address
    d_src[TB.LEAD: TB.LEAD + s["total"]] = torch.from_numpy(s["src"]).cuda()
    d = {k: torch.from_numpy(s[k]).cuda() for k in ("src_offsets", "order", "dst_offsets")}
    d_flag = None if flag is None else torch.from_numpy(np.asarray(flag, dtype=np.int32)).cuda()
    starts = np.concatenate(([0], np.cumsum([hi - lo + GAP for lo, hi in windows])))
    out, out_at = TB.fenced(torch, int(starts[-1]))
    refused = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = np.full(int(starts[-1]), TB.SENT, dtype=np.uint8)
    src_bytes = s["src"].tobytes()
    for (lo, hi), at in zip(windows, starts[:-1].tolist()):
        first, count = (0, s["n"]) if whole_range else records_of(s, lo, hi)
        B.check(L.bgsa_hip_bam_gather_dev(src_at, s["total"], d["src_offsets"].data_ptr(), s["n"], d["order"].data_ptr(), d["dst_offsets"].data_ptr(),
                                          s["n"], first, count, lo, hi, None if d_flag is None else d_flag.data_ptr(), out_at + at,
                                          refused.data_ptr(), None), "bam_gather_dev")
        written, bad = G.gather(src_bytes, s["src_offsets"], s["order"], s["dst_offsets"], *records_of(s, lo, hi), lo, hi, flag)
        assert bad == 0 and sorted(written) == list(range(lo, hi)), (lo, hi)       # the records tile the payload: the window's image is whole
        want[at: at + hi - lo] = [written[p] for p in range(lo, hi)]
    torch.cuda.synchronize()
    got = np.frombuffer(TB.unfenced(out, int(starts[-1])), dtype=np.uint8)
    assert int(refused.item()) == 0
    if not np.array_equal(got, want):
        p = int(np.flatnonzero(got != want)[0])
        w = int(np.searchsorted(starts, p, side="right")) - 1
        raise AssertionError(f"window {windows[w]}: byte {p - int(starts[w])} of its image is {got[p]:#x}, the model says {want[p]:#x}")


@pytest.mark.parametrize("with_flag", (False, True))
def test_the_gather_kernel_equals_the_model_on_every_window(torch_gpu, with_flag):
    lengths = [x for x in LENGTHS if x >= 20] if with_flag else LENGTHS
    s = layout(45 + with_flag, lengths, 16 if with_flag else 11)
    assert 190 <= s["n"] <= 210
    flag = None
    if with_flag:                                              # flags that differ from the source's two bytes, 0x0400 among them; bits above 16 are cut
        rng = np.random.default_rng(4)
        own = np.array([int(s["src"][a + 18]) | int(s["src"][a + 19]) << 8 for a in s["src_offsets"][:-1]])
        flag = (own ^ rng.integers(1, 1 << 16, size=s["n"])) | (rng.integers(0, 1 << 15, size=s["n"]) << 16)
        flag[int(s["order"][np.flatnonzero(s["lens"][s["order"]] == 257)[1]])] = 0x0400
        assert ((flag & 0xffff) != own).all() and (flag >> 16).any() and 0x0400 in flag.tolist()
    windows = windows_of(s)
    assert {hi - lo for lo, hi in windows} >= {0, 1, 61, 256, s["total"]}
    run_windows(torch_gpu, s, windows, flag, whole_range=False)
    few = [w for w in windows if w[1] - w[0] not in (61, 256)]       # the same with every record offered: the kernel clips by itself
    run_windows(torch_gpu, s, few, flag, whole_range=True)
    d = torch_gpu.zeros(8, dtype=torch_gpu.int64, device="cuda")
    out, out_at = TB.fenced(torch_gpu, 64)
    refused = torch_gpu.zeros(1, dtype=torch_gpu.int32, device="cuda")
    assert B.lib().bgsa_hip_bam_gather_dev(d.data_ptr(), 0, d.data_ptr(), 1, d.data_ptr(), d.data_ptr(), 1, 0, 0, 0, 64, None, out_at,
                                           refused.data_ptr(), None) == 0       # count == 0
    assert B.lib().bgsa_hip_bam_gather_dev(d.data_ptr(), 0, d.data_ptr(), 1, d.data_ptr(), d.data_ptr(), 1, 0, 2, 0, 64, None, out_at,
                                           refused.data_ptr(), None) == -1      # first + count > n: refused, nothing launched
    torch_gpu.cuda.synchronize()
    assert TB.unfenced(out, 64) == bytes([TB.SENT]) * 64 and int(refused.item()) == 0


# ---- 2. refusals per record ----------------------------------------------------------------------------------------------------------------
def test_refused_records_are_counted_and_write_nothing(torch_gpu):
    torch, L = torch_gpu, B.lib()
    rng = np.random.default_rng(46)
    lens = rng.integers(20, 90, size=72).astype(np.int64)
    lens[70] = 19                                              # with a flag: too short to hold one
    src_offsets = np.concatenate(([0], np.cumsum(lens)))
    src_offsets[41] = src_offsets[40] - 5                      # source record 40 is not monotone; record 41 is longer for it, and good
    n_src, true_bytes = 72, int(src_offsets[-1])
    src_bytes = true_bytes - 1                                 # source record 71, the last one, leaves src_bytes
    order = rng.permutation(n_src).astype(np.int64)[:70]
    order = np.concatenate((order[~np.isin(order, (40, 70, 71))], [40, 70, 71]))       # the three bad source records are there, once each
    order = order[rng.permutation(order.size)]
    n = order.size
    out_lens = np.diff(src_offsets)[order]
    beyond, below, longer = [int(i) for i in np.flatnonzero(~np.isin(order, (40, 41, 70, 71)))[[1, 20, 40]]]      # three more victims
    order[beyond], order[below] = n_src, -1                    # out of range, both signs
    out_lens[beyond], out_lens[below] = 33, 34
    out_lens[longer] += 3                                      # the two lengths differ
    out_lens[order == 40] = 30                                 # some room, never written
    dst_offsets = np.concatenate(([0], np.cumsum(out_lens)))
    total = int(dst_offsets[-1])
    src = rng.integers(0, 256, size=true_bytes, dtype=np.uint8)
    flag = rng.integers(0, 1 << 16, size=n_src).astype(np.int32)
    written, bad = G.gather(src.tobytes()[:src_bytes], src_offsets, order, dst_offsets, 0, n, 0, total, flag)
    assert bad == 6 and n - bad >= 64
    untouched = sorted(set(range(total)) - set(written))
    bad_records = [beyond, below, longer] + [int(np.flatnonzero(order == s)[0]) for s in (40, 70, 71)]
    assert untouched == sorted(p for i in bad_records for p in range(int(dst_offsets[i]), int(dst_offsets[i + 1])))
    d_src = torch.from_numpy(src).cuda()
    d = [torch.from_numpy(x).cuda() for x in (src_offsets, order, dst_offsets, flag)]
    out, out_at = TB.fenced(torch, total)
    refused = TI.Fenced(torch, 1, torch.int32)
    refused.set(0)
    B.check(L.bgsa_hip_bam_gather_dev(d_src.data_ptr(), src_bytes, d[0].data_ptr(), n_src, d[1].data_ptr(), d[2].data_ptr(), n, 0, n, 0, total,
                                      d[3].data_ptr(), out_at, refused.ptr, None), "bam_gather_dev")
    torch.cuda.synchronize()
    want = np.full(total, TB.SENT, dtype=np.uint8)
    want[sorted(written)] = [written[p] for p in sorted(written)]
    assert refused.host().tolist() == [6]
    assert TB.unfenced(out, total) == want.tobytes()           # the good ones written, the bad ones' room still the sentinel
    refused.set(0)                                             # without flags the 19 bytes are a record like any other
    B.check(L.bgsa_hip_bam_gather_dev(d_src.data_ptr(), src_bytes, d[0].data_ptr(), n_src, d[1].data_ptr(), d[2].data_ptr(), n, 0, n, 0, total,
                                      None, out_at, refused.ptr, None), "bam_gather_dev")
    torch.cuda.synchronize()
    assert refused.host().tolist() == [5]


# ---- 3. end to end -------------------------------------------------------------------------------------------------------------------------
PAD = {False: b"", True: b""}                                 # the copy's name: its length moves every record behind it (the hard places below)
SMALL = ((61, 1), (61, 3))


def reads_of(case, paired: bool) -> dict:
    """The case's reads (or pairs) and, at the end, read (pair) 0 again under another name: in another batch, with an equal key."""
    ends = case["reads"] if paired else case["reads"][:1]
    return dict(reads=[np.concatenate((rows, rows[:1])) for rows in ends], names=list(case["names"]) + [case["names"][0] + b"/again" + PAD[paired]],
                quals=[list(q) + [q[0]] for q in (case["quals"] if paired else case["quals"][:1])])


def cuts_of(n: int) -> list:
    """Three batches of unequal size, the middle one a single read or pair."""
    a = n // 3 + 2
    return [(0, a), (a, a + 1), (a + 1, n)]


def call(mapper, data: dict, paired: bool, lo: int, hi: int, **form):
    reads, names, quals = [x[lo:hi] for x in data["reads"]], data["names"][lo:hi], [q[lo:hi] for q in data["quals"]]
    if paired:
        return mapper.map_pairs_bam(reads[0], reads[1], PM.INSERT_MIN, PM.INSERT_MAX, names, quals[0], quals[1], TB.RNAME, k_best=1,
                                    max_distance=PM.MAX_DISTANCE, rescue_distance=PM.RESCUE_DISTANCE, **form)
    return mapper.map_reads_bam(reads[0], names, quals[0], TB.RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, **form)


def merged_of(mapper, data: dict, paired: bool, cuts, **form):
    merge = mapper.bam_merge(**form)
    for lo, hi in cuts:
        assert call(mapper, data, paired, lo, hi, merge=merge) == (hi - lo) * (2 if paired else 1)
    return merge


def concatenated(batches) -> B.BamRecords:
    """Per-batch sort=False calls as ONE BamRecords: the blocks one after the other, the columns joined."""
    offsets = np.concatenate(([0], np.cumsum(np.concatenate([np.diff(b.offsets) for b in batches]))))
    return B.BamRecords(np.concatenate([b.blocks for b in batches]), offsets, *(np.concatenate([getattr(b, name) for b in batches])
                                                                                for name in ("flag", "pos", "mapq", "nm")))


def assert_same_sorted(got, want, what) -> None:
    assert type(got) is type(want) is B.SortedBamRecords, what
    for name in B.SortedBamRecords._fields[:-1]:
        x, y = getattr(got, name), getattr(want, name)
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, name)
    for name, x, y in zip(B.BamIndex._fields, got.index, want.index):
        assert x.dtype == y.dtype and np.array_equal(x, y), (what, "index", name)


@pytest.fixture(scope="module")
def one_call(case):
    """The oracle, code the merge does not touch: ONE sort=True call on all reads, made once per form."""
    made = {}

    def get(paired: bool, **form):
        key = (paired, *sorted(form.items()))
        if key not in made:
            data = reads_of(case, paired)
            made[key] = call(case["mapper"], data, paired, 0, len(data["names"]), sort=True, **form)
        return made[key]
    return get


@pytest.fixture(scope="module")
def plain_batches(case):
    """The sort=False calls of the three batches, joined: what check_sorted compares a sorted result with."""
    made = {}

    def get(paired: bool):
        if paired not in made:
            data = reads_of(case, paired)
            made[paired] = concatenated([call(case["mapper"], data, paired, lo, hi) for lo, hi in cuts_of(len(data["names"]))])
        return made[paired]
    return get


def split_flag(offsets, span: int) -> bool:
    """Whether some record's bytes 18 | 19 lie in different segments of `span` payload bytes."""
    return bool(((offsets[:-1] + 18) % span == span - 1).any())


@pytest.mark.parametrize("paired", (False, True))
def test_the_inputs_reach_the_hard_places(case, one_call, paired):
    want = one_call(paired, compress=False, block_payload=61)
    per = 2 if paired else 1
    cuts = cuts_of(len(reads_of(case, paired)["names"]))
    assert cuts[1][1] - cuts[1][0] == 1 and len({hi - lo for lo, hi in cuts}) == 3
    assert all(TI.straddles(want.offsets, 61 * blocks) for _, blocks in SMALL)                # a record across a segment boundary
    assert any(split_flag(want.offsets, 61 * blocks) for _, blocks in SMALL), \
        [int(x) for x in (want.offsets[:-1] + 18) % 61][:400]                                  # the flag's two bytes in two segments
    batch = np.searchsorted([lo * per for lo, _ in cuts], want.order, side="right") - 1      # the batch of every output record
    records = M.split_records(b"".join(M.walk_blocks(want.blocks.tobytes())))
    keys = [R.decoded_coordinates(M.decode(x, [TB.RNAME]))[0] for x in records]
    assert any(a == b and s != t for a, b, s, t in zip(keys, keys[1:], batch, batch[1:]))      # equal keys from two batches, side by side


@pytest.mark.parametrize("paired", (False, True))
@pytest.mark.parametrize("compress", (False, True))
@pytest.mark.parametrize("block_payload,segment_blocks", SMALL + ((65280, 4096),))
def test_three_batches_equal_one_call(case, one_call, plain_batches, tmp_path, paired, compress, block_payload, segment_blocks):
    mapper, data = case["mapper"], reads_of(case, paired)
    what = f"paired={paired}, compress={compress}, {block_payload} x {segment_blocks}"
    want = one_call(paired, compress=compress, block_payload=block_payload)
    form = dict(block_payload=block_payload, compress=compress, segment_blocks=segment_blocks)
    cuts = cuts_of(len(data["names"]))
    merge = merged_of(mapper, data, paired, cuts, **form)
    assert merge.n == want.flag.size and merge.ends == (2 if paired else 1) and not merge.finished
    got = merge.finish()
    assert_same_sorted(got, want, what)
    assert merge.finished
    with pytest.raises(B.BgsaHipError, match="the merge is finished"):
        call(mapper, data, paired, 0, 1, merge=merge)
    header = mapper.bam_header(TB.RNAME, sort_order="coordinate")
    merged_of(mapper, data, paired, cuts, reserve_bytes=1 << 20, **form).write(tmp_path / "merged.bam", header)
    B.write_bam(tmp_path / "one.bam", header, want, index=True)
    B.write_bam(tmp_path / "finished.bam", header, got, index=True)
    for tail in ("", ".bai"):
        one = (tmp_path / ("one.bam" + tail)).read_bytes()
        assert (tmp_path / ("merged.bam" + tail)).read_bytes() == one and (tmp_path / ("finished.bam" + tail)).read_bytes() == one, (what, tail)
    decoded = TI.check_sorted(got, plain_batches(paired), mapper, [TB.RNAME], block_payload, compress, tmp_path, what)      # without the one-call path
    assert {d["flag"] & 4 for d in decoded} == {0, 4} and decoded[-1]["ref_id"] == -1


# ---- 4. duplicates across batches ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paired", (False, True))
def test_copies_in_a_later_batch_are_marked(case, paired):
    mapper = case["mapper"]
    reads, names, quals, picked = TM.copies(case, paired)
    data = dict(reads=reads, names=names, quals=quals)
    n, originals = len(names), len(case["names"])
    cuts = [(0, originals // 2), (originals // 2, originals), (originals, n)]      # every copy in a LATER batch than its original
    form = dict(block_payload=61)
    mapper.last_duplicate_stats = None
    want = call(mapper, data, paired, 0, n, sort=True, mark_duplicates=True, **form)
    want_stats, mapper.last_duplicate_stats = mapper.last_duplicate_stats, None
    merge = merged_of(mapper, data, paired, cuts, mark_duplicates=True, segment_blocks=3, **form)
    assert mapper.last_duplicate_stats is None                 # the adds ran the key kernel only
    got = merge.finish()
    assert_same_sorted(got, want, f"marked, paired={paired}")
    assert mapper.last_duplicate_stats == want_stats and want_stats["records_flagged"] == int(((got.flag & 1024) != 0).sum()) > 0
    mapper.last_duplicate_stats = "untouched"
    unmarked = merged_of(mapper, data, paired, cuts, mark_duplicates=False, segment_blocks=3, **form).finish()
    assert mapper.last_duplicate_stats == "untouched"
    per_batch = [call(mapper, data, paired, lo, hi) for lo, hi in cuts]
    emitted = np.concatenate([b.flag for b in per_batch])
    assert np.array_equal(unmarked.flag, emitted[unmarked.order]) and not (unmarked.flag & 1024).any()      # every flag as emitted
    assert np.array_equal(unmarked.order, got.order) and np.array_equal(unmarked.offsets, got.offsets)
    records = M.split_records(b"".join(M.walk_blocks(unmarked.blocks.tobytes())))
    lines = [None] * len(records)
    for i, x in zip(unmarked.order.tolist(), records):
        lines[i] = M.decode(x, [TB.RNAME])["line"]
    flagged, model_stats = MD.duplicates_of_sam(lines, paired)                  # the model on the unmarked records, in input order
    assert sorted(flagged) == sorted(got.order[(got.flag & 1024) != 0].tolist()) and model_stats == want_stats
    marked = M.split_records(b"".join(M.walk_blocks(got.blocks.tobytes())))
    for x, y, f in zip(marked, records, got.flag.tolist()):   # bytes 18 | 19 and nothing else
        assert x[:18] == y[:18] and x[20:] == y[20:] and G.flag_of(x) == f
    within = sum(int(((call(mapper, data, paired, lo, hi, mark_duplicates=True).flag & 1024) != 0).sum()) for lo, hi in cuts)
    assert within < want_stats["records_flagged"]              # marking batch by batch finds strictly fewer
    per = 2 if paired else 1
    late = got.order[(got.flag & 1024) != 0] >= originals * per
    assert late.any() and not late.all()                       # copies go, and originals behind a better copy


# ---- 5. the contig form ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", (False, True))
def test_the_contig_form_in_two_batches(torch_gpu, tmp_path, compress):
    F, Pr = C.FIXTURE, C.PAIRS
    sequences = C.contigs()
    mapper = B.ContigMapper([name.decode() for name in F["NAMES"]], sequences, F["W"], F["S"], contig_padding=Pr["PADDING"])
    reads = np.array([list(read) for _, _, read in C.crafted(sequences)], dtype=np.uint8)
    nowhere = TB.ACGT[np.random.default_rng(47).integers(4, size=(2, reads.shape[1]))]
    reads = np.concatenate((reads[: reads.shape[0] // 2], nowhere[:1], reads[reads.shape[0] // 2:], nowhere[1:]))
    args = dict(k_best=F["K_BEST"], max_distance=F["MAX_DISTANCE"])
    want = mapper.map_reads_bam(reads, compress=compress, sort=True, block_payload=61, **args)
    assert len(set(want.ref_id.tolist()) - {-1}) >= 3 and (want.ref_id < 0).sum() >= 2
    cut = reads.shape[0] // 2 + 1
    merge = mapper.bam_merge(block_payload=61, compress=compress, segment_blocks=2)
    assert mapper.map_reads_bam(reads[:cut], merge=merge, **args) == cut
    assert mapper.map_reads_bam(reads[cut:], [f"r{i}".encode() for i in range(cut, reads.shape[0])], merge=merge, **args) == reads.shape[0] - cut
    got = merge.finish()
    assert_same_sorted(got, want, f"contigs, compress={compress}")
    header = mapper.bam_header(sort_order="coordinate")
    merge.write(tmp_path / "merged.bam", header)               # a finished merge writes the same again
    B.write_bam(tmp_path / "one.bam", header, want, index=True)
    assert all((tmp_path / ("merged.bam" + t)).read_bytes() == (tmp_path / ("one.bam" + t)).read_bytes() for t in ("", ".bai"))
    assert R.parse_bai((tmp_path / "merged.bam.bai").read_bytes())["n_no_coor"] >= 2
    pairs = C.crafted_pairs(sequences)
    reads1, reads2 = (np.array([list(x[e]) for x in pairs], dtype=np.uint8) for e in (1, 2))
    pair_args = dict(k_best=Pr["K_BEST"], max_distance=F["MAX_DISTANCE"])
    names = [b"proper", b"across", b"half"]
    want = mapper.map_pairs_bam(reads1, reads2, Pr["INSERT_MIN"], Pr["INSERT_MAX"], names, compress=compress, sort=True, block_payload=61, **pair_args)
    merge = mapper.bam_merge(block_payload=61, compress=compress, segment_blocks=1)
    for lo, hi in ((0, 1), (1, 3)):
        assert mapper.map_pairs_bam(reads1[lo:hi], reads2[lo:hi], Pr["INSERT_MIN"], Pr["INSERT_MAX"], names[lo:hi], merge=merge, **pair_args) == 2 * (hi - lo)
    assert_same_sorted(merge.finish(), want, f"contigs, pairs, compress={compress}")


# ---- 6. edges ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("compress", (False, True))
def test_a_merge_without_a_record(case, tmp_path, compress):
    mapper = case["mapper"]
    got = mapper.bam_merge(compress=compress, mark_duplicates=True).finish()
    assert isinstance(got, B.SortedBamRecords) and got.blocks.size == 0 and got.blocks.dtype == np.uint8 and got.offsets.tolist() == [0]
    assert all(getattr(got, name).size == 0 for name in ("flag", "pos", "mapq", "nm", "ref_id", "order"))
    assert all(x.size == 0 for x in got.index[1:5]) and got.index.n_intv.tolist() == [0] and got.index.ref_lens.tolist() == [mapper.ref_len]
    assert mapper.last_duplicate_stats == dict.fromkeys(B.DUPLICATE_STATS, 0)
    empty = R.build_index([], [], [], [], [0], 65280, None, [mapper.ref_len])
    assert B.bai_bytes(got.index, got.flag, got.ref_id) == R.bai_bytes(empty, [], [])
    header = mapper.bam_header(TB.RNAME, sort_order="coordinate")
    mapper.bam_merge(compress=compress).write(tmp_path / "empty.bam", header)
    assert (tmp_path / "empty.bam").read_bytes() == B.bgzf_blocks(header) + B.BGZF_EOF
    parsed = R.parse_bai((tmp_path / "empty.bam.bai").read_bytes())
    assert parsed["n_no_coor"] == 0 and (tmp_path / "empty.bam.bai").read_bytes() == R.bai_bytes(empty, [], [], len(B.bgzf_blocks(header)))


def test_a_batch_of_unmapped_reads_only(case):
    mapper, reads, names, quals = case["mapper"], case["reads"][0][-4:], case["names"][-4:], case["quals"][0][-4:]
    args = dict(k_best=2, max_distance=PM.MAX_DISTANCE)
    want = mapper.map_reads_bam(reads, names, quals, TB.RNAME, sort=True, block_payload=61, **args)
    assert (want.flag == 4).all() and (want.ref_id == -1).all()
    merge = mapper.bam_merge(block_payload=61, segment_blocks=2, mark_duplicates=True)
    assert mapper.map_reads_bam(reads, names, quals, TB.RNAME, merge=merge, **args) == 4
    got = merge.finish()
    assert_same_sorted(got, want, "unmapped only")
    assert got.index.chunk_ref.size == 0 and got.index.n_intv.tolist() == [0] and got.order.tolist() == [0, 1, 2, 3]
    assert mapper.last_duplicate_stats == dict.fromkeys(B.DUPLICATE_STATS, 0)


def test_a_refused_add_leaves_the_merge_as_it_was(case):
    mapper, data = case["mapper"], reads_of(case, False)
    pairs = reads_of(case, True)
    merge, alone = mapper.bam_merge(block_payload=256), mapper.bam_merge(block_payload=256)
    for m in (merge, alone):
        assert call(mapper, data, False, 0, 9, merge=m) == 9
    state = (merge.n, merge.payload_bytes, merge.ends, {k: len(v) for k, v in merge.columns.items()})
    with pytest.raises(B.BgsaHipError, match="a paired batch into a merge of single-end ones"):
        call(mapper, pairs, True, 9, 12, merge=merge)
    with pytest.raises(B.BgsaHipError, match="sort beside merge="):
        call(mapper, data, False, 9, 12, merge=merge, sort=True)
    with pytest.raises(B.BgsaHipError, match="the merge belongs to another mapper"):
        call(B.ReferenceMapper(case["ref"], PM.W, PM.S), data, False, 9, 12, merge=merge)
    with pytest.raises(B.BgsaHipError):                        # a malformed batch: a QUAL string of another length than its read
        mapper.map_reads_bam(data["reads"][0][9:12], data["names"][9:12], [b"!!"] * 3, TB.RNAME, k_best=2, max_distance=PM.MAX_DISTANCE, merge=merge)
    assert state == (merge.n, merge.payload_bytes, merge.ends, {k: len(v) for k, v in merge.columns.items()}) and not merge.finished
    assert_same_sorted(merge.finish(), alone.finish(), "after the refused adds")


def test_a_batch_the_device_refuses_leaves_the_merge_as_it_was(torch_gpu, crafted):
    """The record passes refuse a batch on the device, behind the key kernels: the merge changes only after the last check."""
    _, mapper, records = crafted
    batch = TB.Batch(torch_gpu, mapper, records, None)
    fields = {key: value for key, value in batch.dev.items() if key != "runs_row"}
    names, offsets, rows = batch.keep[2].cpu().numpy(), batch.keep[3].cpu().numpy(), batch.keep[0].cpu().numpy()
    rname = np.frombuffer(TB.RNAME, np.uint8)
    want = mapper.sam_records("crafted", rows, None, names, offsets, rname, fields, batch.keep[5], fmt="bam", block_payload=61, sort=True,
                              mark_duplicates=True)
    merge = mapper.bam_merge(block_payload=61, segment_blocks=2, mark_duplicates=True)
    assert mapper.sam_records("crafted", rows, None, names, offsets, rname, fields, batch.keep[5], fmt="bam", merge=merge) == len(records)
    far = dict(fields, tlen=fields["tlen"].clone())
    far["tlen"][4] = 2 ** 33
    with pytest.raises(B.BgsaHipError, match="1 malformed records, the first the one of read 4"):
        mapper.sam_records("crafted", rows, None, names, offsets, rname, far, batch.keep[5], fmt="bam", merge=merge)
    with pytest.raises(B.BgsaHipError, match="merge= needs fmt 'bam'"):
        mapper.sam_records("crafted", rows, None, names, offsets, rname, fields, batch.keep[5], merge=merge)
    assert merge.n == len(records) and all(len(v) == 1 for v in merge.columns.values())
    assert_same_sorted(merge.finish(), want, "crafted")


def test_merge_none_is_the_call_without_the_argument(case):
    mapper = case["mapper"]
    for paired in (False, True):
        data = reads_of(case, paired)
        n = len(data["names"])
        for form in (dict(), dict(sort=True, compress=True, mark_duplicates=True, block_payload=256)):
            want, got = call(mapper, data, paired, 0, n, **form), call(mapper, data, paired, 0, n, merge=None, **form)
            assert type(got) is type(want)
            if form:
                assert_same_sorted(got, want, (paired, form))
            else:
                assert all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(got, want))

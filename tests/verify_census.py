"""The verify census — a helper, not a test: the ONE place that says which shapes launch every instance of
reference_verify_pairs_kernel<WB, Blocks, Lens> (bgsa_amd/csrc/seed_map.hip), the kernel every distance of seeded mapping comes
from.  tests/test_verify_census_cpu.py proves on the host that these shapes reach every kernel name the dispatch can produce,
at word_num == WB and wherever the ladder leaves a gap below WB, every tail of a column block and every size of the last block
of window rows; tests/test_verify_census_gpu.py launches them against a plain DP.

Which instance a word count launches is the library's own answer (bgsa_hip_reference_verify_kernel_name), never a width list
copied here: a width added to dispatch_verify changes the names, and the CPU test fails until the census reaches it.

The expectation is host work only: the windows are cut from the reference bytes with numpy (reverse ids reverse-complemented,
'N' stays 'N') and handed with the reads to oracle.dp_edit_semiglobal, the C DP of the semi-global scoring tests."""
import functools
import re
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))

import oracle as O  # noqa: E402
import reference_map_reference as M  # noqa: E402
import width_census as W  # noqa: E402
from test_place_pairs_banded_cpu import _edit  # noqa: E402

ACGT = np.frombuffer(b"ACGT", np.uint8)
A_, N_ = ord("A"), ord("N")

NAME_WORDS = 130                 # names are asked for 1 .. 130 words, as the width census asks
WORDS = list(range(1, 34))       # 17 .. 32: every tail of 1 .. 16 words behind a full column block; 33: a third block
STRIDE = 37                      # odd: the window starts 0, 37, 74, 111 take all four byte skews
ON_STRIDE = 4                    # windows 0 .. 3 on the stride, then the anchored one, one byte further
N_WINDOWS = ON_STRIDE + 1
N_IDS = 2 * N_WINDOWS            # both strands
N_READS = 70                     # with the 58 pad columns: two subject groups
SPARE = 8                        # reference bases behind a planted read's source: 8 deletions leave it all reference
MAX_EDITS = 8
HANG = 5                         # bases a hanging read has beyond the reference's end
SUBJECT_BASE = 1 << 33
# position in the pair list: (window id, subject without the base).  A slot nobody owns — the unused slot, the next bucket, below
# the base — and an owned slot that names no window; neither may be written.
NOBODY = {10: (3, -1), 11: (7, 128), 12: (0, -5)}
NO_WINDOW = {20: (-1, 5), 21: (N_IDS, 6), 22: (2 ** 31 - 1, 7), 23: (-2 ** 31, 8)}
THREADS = 16                     # of the DP: the largest case is under a gigacell
P = 0x10000                      # a non-null "device pointer" for calls that return before they look at it


# ---- which instance, which word counts ------------------------------------------------------------------------------------------
def kernel_names(L, lens, upto=NAME_WORDS):
    """bgsa_hip_reference_verify_kernel_name(w, lens) for w = 1 .. upto; names[w - 1] is the instance of w words."""
    return [L.bgsa_hip_reference_verify_kernel_name(w, int(lens)).decode() for w in range(1, upto + 1)]


def name_width(name):
    return int(re.search(r"<(\d+)", name).group(1))


def name_blocks(name):
    return re.search(r"<\d+, (true|false), (true|false)>", name).group(1) == "true"


def accepted(L, w):
    """Whether the verify calls take a bucket of w words: their checks pass (n_pairs == 0 launches nothing, so fake pointers do)."""
    n = 32 * w
    return [L.bgsa_hip_reference_verify_pairs_dev(P, 5000, n + 40, STRIDE, P, n, 64, w, P, P, 0, 0, P, P, 1 << 40, None),
            L.bgsa_hip_reference_verify_pairs_lens_dev(P, 5000, n + 40, STRIDE, P, P, n, 64, w, P, P, 0, 0, P, P, 1 << 40, None)] == [0, 0]


def read_lengths(w):
    """The widths of the equal-length cases of w words: a partial last word, a full one; the shortest read there is."""
    return ([1] if w == 1 else []) + [32 * w - 5, 32 * w]


def window_len(w, n):
    """n + 33 .. n + 64.  11 is odd, so over w = 1 .. 32 each of the two families of read_lengths takes all 32 residues of
    m mod 32: every size of the last block of window rows, the full one included.  The full-last-word family is 11 further
    on: m mod 32 is 28 + 11 w in one family and 12 + 11 w in the other, 16 apart, and what 16 consecutive w leave out in one
    family is 16 away from what they take — so the one-block instances (w = 1 .. 16) and the column blocks (17 .. 32) see all
    32 residues each."""
    return n + 33 + (11 * w + (11 if n % 32 == 0 else 0)) % 32


def ref_len(m):
    """The smallest reference with windows 0 .. 3 on the stride and an anchored last window off it."""
    return m + (ON_STRIDE - 1) * STRIDE + 1


def cases():
    """[(w, n, lens)]: the whole census."""
    return [(w, n, lens) for w in WORDS for n in read_lengths(w) for lens in (False, True)]


# ---- the lengths of a mixed-length bucket ----------------------------------------------------------------------------------------
def required_lengths(w):
    """What a Lens bucket of w words must hold: both edges of the last word and of the one before it; with column blocks a
    length whose own word lies in each block, the last bit of block 0 and the first bit of block 1."""
    need = {max(1, n) for n in (1, 32 * (w - 1), 32 * (w - 1) + 1, 32 * w - 5, 32 * w - 1, 32 * w)}
    if w > 16:
        need |= {512, 513} | {min(512 * b + 77, 32 * w) for b in range((w + 15) // 16)}
    return sorted(need)


def lens_lengths(w, width):
    """70 lengths up to `width` (of w words), the longest equal to it: width_census.lens_lengths(w), clipped to the width, with
    the lengths of required_lengths that it lacks written over entries of its cycle."""
    lens = [min(x, width) for x in W.lens_lengths(w)]
    lacking = [x for x in required_lengths(w) if x <= width and x not in lens]
    for i, x in enumerate(lacking):
        lens[11 + 7 * i] = x                         # the cycle of <= 6 edges fills entries 0 .. 63: every edge stays
    assert max(lens) == width and len(lens) == N_READS and min(lens) >= 1
    return lens


def own_block(n):
    """The column block (of 16 words) that holds the score column of a read of n bp."""
    return ((n - 1) >> 5) // 16


# ---- one case ----------------------------------------------------------------------------------------------------------------------
def cut_window(ref, m, wid):
    """Window id `wid` of the census geometry as ASCII: ids from N_WINDOWS on are the reverse complement."""
    start = M.window_start(ref.size, m, STRIDE, wid % N_WINDOWS)
    row = ref[start: start + m]
    return M.reverse_complement(row) if wid >= N_WINDOWS else row


def make_reads(rng, ref, m, lengths):
    """70 reads, read c of lengths[c] bp.  Every fifth is random; read 0 hangs off the reference's start (inside window 0), read 1
    off its end (inside the anchored window), read 2 is all 'A', read 3 holds an 'N' run; planted read j of the others comes
    from window id j % 10 — reverse-complemented for a reverse id — with j % 9 edits: 10 and 9 are coprime, so every id gets
    its reads with five or six different edit counts of 0 .. 8."""
    L = ref.size
    reads, planted = [], 0
    for c, n in enumerate(lengths):
        hang = min(HANG, n // 2)
        if c % 5 == 4:
            read = ACGT[rng.integers(4, size=n)]
        elif c == 0:
            read = np.concatenate([ACGT[rng.integers(4, size=hang)], ref[: n - hang]])
        elif c == 1:
            read = np.concatenate([ref[L - (n - hang):], ACGT[rng.integers(4, size=hang)]])
        elif c == 2:
            read = np.full(n, A_, np.uint8)
        else:
            wid, edits = planted % N_IDS, planted % (MAX_EDITS + 1)
            planted += 1
            start = M.window_start(L, m, STRIDE, wid % N_WINDOWS)
            begin = start + int(rng.integers(0, m - n - SPARE + 1))            # the source lies inside the window: m >= n + 33
            read = np.array(_edit(rng, list(ref[begin: begin + n + SPARE]), edits, ACGT)[:n], np.uint8)
            if wid >= N_WINDOWS:
                read = M.reverse_complement(read)
            if c == 3:
                read = read.copy()
                read[n // 3: n // 3 + max(1, n // 6)] = N_
        read = np.asarray(read, np.uint8)
        assert read.size == n, (c, n, read.size)
        reads.append(read)
    return reads


@functools.lru_cache(maxsize=8)
def case(w, n, lens):
    """Everything of case (w, n, lens), computed once and never modified:
    ref           the reference, ACGT with a dozen 'N'
    m             the window length; the reference has N_WINDOWS windows on the stride 37, the last one anchored
    reads         list of 70 arrays; lengths: their lengths (all n unless lens)
    windows, subjects   the pair list: every read against every window id in a shuffled order, with the seven slots of NOBODY
                  and NO_WINDOW put in between (`owned` is False there): 707 pairs; subjects without the base
    want          int64 per pair: the DP's distance (owned pairs only; -1 elsewhere)
    dist          int64 [N_IDS, 70]: the DP's distance of every read inside every window id"""
    assert (n + 31) // 32 == w
    rng = np.random.default_rng([w, n, int(lens)])
    m = window_len(w, n)
    L = ref_len(m)
    ref = ACGT[rng.integers(4, size=L)].copy()
    ref[rng.integers(L, size=12)] = N_
    assert M.window_count(L, m, STRIDE) == N_WINDOWS
    lengths = lens_lengths(w, n) if lens else [n] * N_READS
    reads = make_reads(rng, ref, m, lengths)

    rows = np.stack([cut_window(ref, m, wid) for wid in range(N_IDS)])
    dist = np.full((N_IDS, N_READS), -1, np.int64)
    for length in sorted(set(lengths)):                                          # every read at its own length
        cols = [c for c in range(N_READS) if lengths[c] == length]
        dist[:, cols] = -O.dp_edit_semiglobal(rows, np.stack([reads[c] for c in cols]), threads=THREADS).astype(np.int64)
    assert (dist >= 0).all() and (dist <= np.array(lengths)[None, :]).all()

    order = rng.permutation(N_IDS * N_READS)
    pairs = [(int(x) // N_READS, int(x) % N_READS) for x in order]               # (window id, read), lanes of a wave mix both
    for at, (wid, subject) in sorted({**NOBODY, **NO_WINDOW}.items()):
        pairs.insert(at, (wid, subject))
    windows = np.array([p[0] for p in pairs], np.int32)
    subjects = np.array([p[1] for p in pairs], np.int64)
    owned = np.ones(len(pairs), bool)
    owned[list(NOBODY) + list(NO_WINDOW)] = False
    assert len(pairs) % 64 != 0 and owned.sum() == N_IDS * N_READS
    want = np.where(owned, dist[np.where(owned, windows, 0), np.where(owned, subjects, 0)], -1)
    out = dict(ref=ref, m=m, reads=reads, lengths=lengths, windows=windows, subjects=subjects, owned=owned, want=want, dist=dist)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def device_subjects(subjects):
    """The pair list's subjects as the call takes them: the base added, the unused slot -1 left as it is."""
    return np.where(subjects == -1, -1, subjects + SUBJECT_BASE)


def assert_worth_launching(c, w, n, lens):
    """Conditions on the inputs of case c = case(w, n, lens), from the DP alone.  A distance never exceeds the read's length, so
    the two counts are asked of every case but n = 1, where a distance is 0 or 1."""
    windows, subjects, want = c["windows"][c["owned"]], c["subjects"][c["owned"]], c["want"][c["owned"]]
    L, m = c["ref"].size, c["m"]
    starts = [M.window_start(L, m, STRIDE, i) for i in range(N_WINDOWS)]
    assert [s % 4 for s in starts[:ON_STRIDE]] == [0, 1, 2, 3] and starts[-1] % STRIDE != 0 and starts[-1] + m == L
    assert (c["ref"] == N_).sum() >= 8
    counts = np.bincount(windows, minlength=N_IDS)
    assert (counts == N_READS).all(), "every read against every window id, both strands"
    assert windows.size == N_IDS * N_READS and {0, N_WINDOWS - 1, N_WINDOWS, N_IDS - 1} <= set(windows.tolist())
    assert (want >= 0).all() and (want <= np.array(c["lengths"])[subjects]).all()
    if n == 1:
        assert 0 in want and set(want.tolist()) <= {0, 1}
    else:
        assert (want <= MAX_EDITS).sum() >= 50, int((want <= MAX_EDITS).sum())
        assert (want > MAX_EDITS).sum() >= 100, int((want > MAX_EDITS).sum())
        for half in (windows < N_WINDOWS, windows >= N_WINDOWS):                 # planted reads are found on both strands
            assert (want[half] <= MAX_EDITS).sum() >= 20
    if lens:
        assert set(x for x in required_lengths(w) if x <= n) <= set(c["lengths"]) and max(c["lengths"]) == n
        assert {own_block(x) for x in c["lengths"]} == set(range((w + 15) // 16)), "a column block owns no lane"
    else:
        assert set(c["lengths"]) == {n}

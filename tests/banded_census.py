"""The banded census — a helper, not a test: the ONE place that says which lengths, inputs and knobs launch the banded filter
(bgsa_amd/csrc/banded.hip) at every threshold k = 1 .. 31.  tests/test_banded_census_cpu.py proves on the host that these shapes
reach every placement of a stream event the banded stream can produce, that the inputs stand where they claim to stand and that
the launches take every route a pair can take; tests/test_banded_census_gpu.py launches them against band_dp and oracle.banded64.

The census's own reference is band_dp below: a plain unit-cost DP over the diagonals j - i in [-(k + 1), k - 1] with
D[i][0] = i and D[0][j] = 0 for j <= k - 1; with last = len if len <= 64 else max(len - k, 64) a pair is rejected (127) iff
D[last][last - k - 1] > 2k + 1, and scores min over j >= len - k - 1 of D[len][j] otherwise.  It shares no structure with the
kernels (bit-parallel rows on match strings) nor with oracle.banded64 (the reference's sliding 64-bit word, restated literally).

Event-placement classes (stream_classes): per EVENT token of the packed stream (rows_ir.banded_stream_bytes on
rows_ir.banded_tokens(length, k, cut=banded_cut_rows(k))) the tuple
    (kernel form, merged event byte, whether the 7-token window in front of it was closed early,
     the regime of `last`: len <= 64 / 64 < len <= 64 + k (last = 64) / longer, whether len is a multiple of 32)
and per stream ("END at slot", form, the slot of the END token in its window, regime).

One launch per (k, length): 4 queries by 192 subjects = three subject groups, so the last wave of the two-group kernels (k <= 15)
holds one group and runs it twice.
  queries   0: a random read; 1: query 0 with 'A' at FOREIGN positions; 2: query 1 again, its mapped bytes at those positions
            overwritten with bytes above 4 on the device (must score as its twin 1); 3: a read over {A, C} only.
  group 0   every lane a near-duplicate of query 0 or 1 at 0 .. 2k + 5 edits: more than push_max lanes alive, the wave runs its
            own loop to the last row; pairs on both sides of the limit.
  group 1   random reads with 1 .. 3 near-duplicates of query 3 at random lanes: the regroup route.  On four lengths in eight of
            the period block the group holds exactly 8, 9, 32 or 33 copies of query 3 among reads over {G, T} (rejected against
            query 3 at every length: an error in every row): a push at exactly push_max lanes, a test at push_max + 1 that goes on.
  group 2   a lone near-duplicate of query 0 among 7 random reads, 8 reads over {G, T} and 48 reads of 'N' (rejected against every
            query): at most 16 lanes alive, so with every pair of the wave counted twice a push_max of 32 takes them at its first
            test; against query 3 the whole wave dies.

The flush launches (FLUSH_SHAPES, flush_launch): with the default push_max of 8 the survivor list passes 64 - 8 only after eight
pushes of eight lanes in front of a ninth query of the same tile, i.e. in a tile of 16.  pick_query_tile gives a launch this small
a tile of 16 where 8 x length x groups per wave < 512: with one group per wave (k >= 16) at every length below 64, and at
k = 16 .. 24 the tests at rows 48 and 56 (push_row_solid = k + 32 <= 56) lie before last = len there.  With two groups per wave
(k <= 15) a tile of 16 needs len < 32, below push_row_solid: those forms show the flush under dense_pass only.  A flush launch is
16 near-duplicate queries over {A, C} by 192 subjects: group 0 holds 8 near-duplicates among reads over {G, T} (the list is exactly
full, 64 pairs, in front of query 8, and again at the tile's end), group 1 nine (one too many: run to the end), group 2 four (56
pairs in front of query 14 do not pass the bound, 60 in front of query 15 do).
"""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))

import bgsa_amd as B  # noqa: E402
import oracle as O  # noqa: E402
import rows_ir as R  # noqa: E402

THRESHOLDS = range(1, 32)
BLOCK = 4                                # thresholds per GPU child: 1 .. 4, 5 .. 8, ..., 29 .. 31
MAX_LEN = 1100                           # the classes of every length up to here are reached
NQ, NS = 4, 192
FOREIGN = (5, 9, 65, 200, 255)           # bytes above 4 written over mapped query bytes (cycled over the positions)
N_FOREIGN = 3
PUSH_MAX_DEFAULT, PUSH_ROW_DEFAULT, PUSH_SOLID_DEFAULT = 8, 48, 32      # banded.hip: banded_push_max, _row_offset, _solid_offset
PLANTS = {1: 8, 2: 9, 3: 32, 4: 33}      # position in the period block mod 8 -> copies of query 3 in group 1
FLUSH_NQ = 16
# (k, length) of the flush launches: one group per wave, a query tile of 16, a test at or after row k + 32
FLUSH_SHAPES = ((16, 60), (20, 57), (20, 60), (24, 63))

KNOBS = ("BGSA_BANDED_IMPL", "BGSA_BANDED_GROUPS", "BGSA_BANDED_PAIR_LOOP", "BGSA_BANDED_DYNAMIC", "BGSA_BANDED_PUSH_MAX",
         "BGSA_BANDED_PUSH_ROW", "BGSA_BANDED_PUSH_SOLID", "BGSA_BANDED_SOLID_MARGIN", "BGSA_BANDED_LDS_PAD", "BGSA_DYNAMIC_TASKS",
         "BGSA_DYNAMIC_MIN_TASKS", "BGSA_DYNAMIC_TASK_TARGET", "BGSA_DYNAMIC_TASK_WORDS", "BGSA_TASK_TARGET", "BGSA_QUERY_TILE_MAX",
         "BGSA_PERSISTENT_PER_CU", "BGSA_HIP_LIB")

# name -> the knobs of the child process (every other knob of KNOBS is taken out of its environment)
CONFIGS = {
    "static": {},
    "counter": {"BGSA_DYNAMIC_MIN_TASKS": "1"},                        # the DYN instantiations
    "first_pass": {"BGSA_BANDED_PUSH_MAX": "0"},                       # no survivor queue: every score from the row loop's own walk
    "dense_pass": {"BGSA_BANDED_PUSH_MAX": "32", "BGSA_BANDED_PUSH_ROW": "0", "BGSA_BANDED_PUSH_SOLID": "0",
                   "BGSA_BANDED_SOLID_MARGIN": "0"},                   # survivors handed over at the first test with <= 32 alive
}


def child_env(config, environ):
    env = {k: v for k, v in environ.items() if k not in KNOBS}
    env.update(CONFIGS[config])
    return env


def blocks():
    return list(range((len(THRESHOLDS) + BLOCK - 1) // BLOCK))


def block_thresholds(block):
    return [k for k in THRESHOLDS if (k - THRESHOLDS[0]) // BLOCK == block]


# ---- the kernel a threshold runs ------------------------------------------------------------------------------------------------
def form(k):
    """banded.hip: banded_select without a knob."""
    cut = R.banded_cut_rows(k)
    return "cut16" if cut == 16 else "cut8" if cut == 8 else "funnel32" if k <= 15 else "funnel64"


def kernel_name(k):
    return {"cut16": "banded_cut_kernel<2>", "cut8": "banded_cut_kernel<2>", "funnel32": "banded_cut_kernel<2, funnel32>",
            "funnel64": "banded_cut_kernel<1, funnel64>"}[form(k)]


def groups_per_wave(k):
    return 1 if k > 15 else 2


def flush_shapes(block=None):
    return [(k, n) for k, n in FLUSH_SHAPES if block is None or k in block_thresholds(block)]


def query_tile(length, k, nq=NQ, n_groups=NS // 64):
    """bgsa_common.h: pick_query_tile as banded.hip: launch_rows asks it (q_max 32, 512 row-words at least, 16,384 tasks wanted)."""
    g = groups_per_wave(k)
    waves = (n_groups + g - 1) // g
    q_min = 1
    while q_min < 32 and q_min * length * g < 512:
        q_min <<= 1
    q_tile = 32
    while q_tile > q_min and ((nq + q_tile - 1) // q_tile) * waves < 16384:
        q_tile >>= 1
    return q_tile


def push_knobs(config, k):
    """(push_row, push_row_solid, solid_limit, push_max) as banded.hip: launch_rows passes them under the configuration's knobs."""
    env = CONFIGS[config]
    push_max = int(env.get("BGSA_BANDED_PUSH_MAX", PUSH_MAX_DEFAULT))
    assert 0 <= push_max <= 32
    push_row = k + int(env.get("BGSA_BANDED_PUSH_ROW", PUSH_ROW_DEFAULT))
    push_row_solid = min(push_row, k + int(env.get("BGSA_BANDED_PUSH_SOLID", PUSH_SOLID_DEFAULT)))
    margin = int(env["BGSA_BANDED_SOLID_MARGIN"]) if "BGSA_BANDED_SOLID_MARGIN" in env else (k + 2) // 2
    solid_limit = k + 1 - margin if k + 1 > margin else 0
    return push_row, push_row_solid, solid_limit, push_max


# ---- stream events --------------------------------------------------------------------------------------------------------------
def regime(length, k):
    return "len <= 64" if length <= 64 else "last = 64" if length <= 64 + k else "last = len - k"


@functools.lru_cache(maxsize=None)
def test_rows(length, k):
    """((rows done, event bits)) of every test of the stream, in order."""
    out, done = [], 0
    for kind, val in R.banded_tokens(length, k, cut=R.banded_cut_rows(k)):
        if kind == "row":
            done += 1
        elif val & 4:
            out.append((done, val))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stream_classes(length, k):
    """The event-placement classes of the packed stream of (length, k): see the module's docstring."""
    raw = R.banded_stream_bytes(length, k, np.zeros(length, np.uint8), cut=R.banded_cut_rows(k))
    f, reg, edge = form(k), regime(length, k), length % 32 == 0
    out, pos = set(), 0
    while True:
        b = raw[pos]
        if b == R.BANDED_EVENT:
            early = pos % 8 == 0 and pos >= 8 and raw[pos - 2] == R.BANDED_REFILL
            out.add((f, raw[pos + 1], early, reg, edge))
            pos += 2
        elif b == R.BANDED_END:
            out.add(("END at slot", f, pos % 8, reg))
            return frozenset(out)
        elif b == R.BANDED_REFILL:      # as the row loop: the next window (an early close leaves an END byte behind it)
            pos = (pos | 7) + 1
        else:
            pos += 1


def domain(k):
    return range(2 * k + 2, MAX_LEN + 1)


def sketch_lengths(k):
    """What the routes need whatever the classes say: the shortest lengths, both sides of 64 and of 64 + k, and one period of 32
    lengths above both 64 + k and k + 48 + 16, where the pushes from rows k + 32 and k + 48 can happen; and one length at which
    random pairs are dead at every late test even at the widest band."""
    lo = 2 * k + 2
    period = max(64 + k, k + 48 + 16) + 1
    want = set(range(lo, lo + 8)) | set(range(57, 73)) | set(range(64 + k - 2, 64 + k + 4)) | set(range(period, period + 32))
    want.add(96 + 6 * k)
    return sorted(x for x in want if x >= lo)


def period_block(k):
    lo = max(64 + k, k + 48 + 16) + 1
    return range(lo, lo + 32)


@functools.lru_cache(maxsize=None)
def lengths(k):
    """The census lengths of threshold k: the sketch, taken whatever it adds, and every further length at which a class shows that
    neither the sketch nor a shorter length of the domain has shown.  Sufficient — no class of the domain is left out —, not the
    smallest such set: most sketch lengths add no class of their own (they are there for the routes), and a longer length could
    stand for several of the added ones at the price of longer launches."""
    have = set()
    for n in sketch_lengths(k):
        have |= stream_classes(n, k)
    out = set(sketch_lengths(k))
    for n in domain(k):
        c = stream_classes(n, k)
        if not c <= have:
            out.add(n)
            have |= c
    return tuple(sorted(out))


def shapes(block=None):
    """[(k, length)] of the census (of one block of thresholds)."""
    ks = THRESHOLDS if block is None else block_thresholds(block)
    return [(k, n) for k in ks for n in lengths(k)]


# ---- the plain band DP ----------------------------------------------------------------------------------------------------------
def band_dp(q, s, k, rows=False):
    """q [nq, len], s [ns, len] uint8 (compared byte by byte) -> int8 [nq, ns]; rows: also int32 [nq, ns, len + 1], the error on
    the lowest diagonal after every row, D[i][i - k - 1] (rows i <= k: a large number)."""
    nq, length = q.shape
    ns = s.shape[0]
    assert s.shape[1] == length > 2 * k + 1
    width, inf = 2 * k + 1, 1 << 20
    t = np.arange(width, dtype=np.int32)
    pad = np.full((ns, length + 2 * k + 2), 255, np.uint8)       # column j - 1 at index j - 1 + k + 1
    pad[:, k + 1:k + 1 + length] = s
    prev = np.full((nq, ns, width), inf, np.int32)               # cell t of row i: column j = i + t - k - 1
    prev[..., k + 1:] = 0                                        # D[0][j] = 0, j = 0 .. k - 1
    low = np.full((nq, ns, length + 1), inf, np.int32) if rows else None
    last = R.banded_last_check(length, k)
    check = None
    for i in range(1, length + 1):
        c = prev + (q[:, i - 1][:, None, None] != pad[None, :, i - 1:i + 2 * k])
        np.minimum(c[..., :-1], prev[..., 1:] + 1, out=c[..., :-1])
        lo, hi = max(0, k + 1 - i), min(2 * k, length - i + k + 1)
        if lo > 0:
            c[..., :lo] = inf
        if i <= k + 1:
            c[..., k + 1 - i] = i                                # D[i][0] = i
        c -= t
        np.minimum.accumulate(c, axis=2, out=c)                  # the step from the left: D[i][j] <= D[i][j'] + j - j'
        c += t
        if lo > 0:
            c[..., :lo] = inf
        if hi < 2 * k:
            c[..., hi + 1:] = inf
        prev = c
        if rows and i >= k + 1:
            low[..., i] = c[..., 0]
        if i == last:
            check = c[..., 0].copy()
    best = prev[..., :k + 2].min(axis=2)
    out = np.where(check > 2 * k + 1, 127, best).astype(np.int8)
    return (out, low) if rows else out


# ---- which inputs ---------------------------------------------------------------------------------------------------------------
_AC, _GT = np.frombuffer(b"AC", np.uint8), np.frombuffer(b"GT", np.uint8)


def plant_count(k, length, index):
    """Near-duplicates of query 3 in group 1."""
    block = period_block(k)
    if length in block and (length - block[0]) % 8 in PLANTS:
        return PLANTS[(length - block[0]) % 8]
    return 1 + index % 3


@functools.lru_cache(maxsize=8)
def launch(k, length):
    """-> (queries [4, len] ASCII, subjects [192, len] ASCII, foreign: [(position, byte)] to write over row 2 of the mapped queries).
    The host references score the queries as they stand here: row 2 equals row 1."""
    index = lengths(k).index(length)
    seed = 100003 * k + 11 * length
    rng = np.random.default_rng(seed)
    q = np.empty((NQ, length), np.uint8)
    q[0] = O.gen_reads(seed + 1, 1, length)[0]
    at = np.sort(rng.choice(length, N_FOREIGN, replace=False))
    q[1] = q[0]
    q[1, at] = ord("A")
    q[2] = q[1]
    q[3] = _AC[rng.integers(0, 2, length)]
    s = O.gen_reads(seed + 2, NS, length)
    lane = np.arange(64)
    # group 0
    s[:64] = O.mutate(q[lane % 2], (lane + 7 * index) % (2 * k + 6), seed + 3)
    # group 1
    n = plant_count(k, length, index)
    where = 64 + rng.choice(64, n, replace=False)
    if n > 3:
        s[64:128] = _GT[rng.integers(0, 2, (64, length))]
        s[where] = q[3]
        for i in where[1::2]:      # every other copy one substitution away
            s[i, rng.integers(0, length)] = ord("G")
    else:
        s[where] = O.mutate(np.repeat(q[3:4], n, axis=0), rng.integers(0, k // 2 + 1, n), seed + 4)
    # group 2
    perm = 128 + rng.permutation(64)
    s[perm[0]] = O.mutate(q[0:1], [rng.integers(0, k // 2 + 1)], seed + 5)[0]
    s[perm[8:16]] = _GT[rng.integers(0, 2, (8, length))]
    s[perm[16:]] = ord("N")
    foreign = [(int(p), FOREIGN[(i + index) % len(FOREIGN)]) for i, p in enumerate(at)]
    return q, s, foreign


@functools.lru_cache(maxsize=8)
def flush_launch(k, length):
    """-> (queries [16, len], subjects [192, len], []): see the module's docstring."""
    assert (k, length) in FLUSH_SHAPES and groups_per_wave(k) == 1 and query_tile(length, k, FLUSH_NQ) == FLUSH_NQ
    seed = 700001 * k + 13 * length
    rng = np.random.default_rng(seed)
    base = _AC[rng.integers(0, 2, length)]
    q = np.repeat(base[None], FLUSH_NQ, axis=0)
    flip = {ord("A"): ord("C"), ord("C"): ord("A")}
    for i in range(1, FLUSH_NQ):      # query i: one substitution of its own
        at = (7 * i) % length
        q[i, at] = flip[int(q[i, at])]
    s = _GT[rng.integers(0, 2, (NS, length))]
    for group, n in enumerate((8, 9, 4)):
        where = 64 * group + rng.choice(64, n, replace=False)
        s[where] = base
        for i in where[1::2]:         # every other one a substitution away
            s[i, rng.integers(0, length)] = ord("G")
    return q, s, []


def cases(block=None):
    """(k, length, queries, subjects, foreign, kind) of every launch (of one block of thresholds): the census shapes, then the
    flush launches."""
    for k, length in shapes(block):
        yield (k, length) + launch(k, length) + ("census",)
    for k, length in flush_shapes(block):
        yield (k, length) + flush_launch(k, length) + ("flush",)


# ---- the route a (wave, query) takes --------------------------------------------------------------------------------------------
def waves(k, n_groups=NS // 64):
    """[(first group, groups the wave holds)]: the two-group kernels give the last wave of an odd count one group."""
    g = groups_per_wave(k)
    return [(w, min(g, n_groups - w)) for w in range(0, n_groups, g)]


def route(low, k, length, config):
    """low: [lanes of the wave's groups (64 or 128), len + 1], errors on the lowest diagonal after every row, for ONE query.
    -> ("dead", row) | ("push", row, alive as the wave counts them, lanes listed) | ("end",), and the counts every eligible test
    saw [(row, alive as counted)].  The alive lanes of both groups are added before they meet push_max; a two-group wave that
    holds one group runs it twice and counts every lane twice."""
    push_row, push_row_solid, solid_limit, push_max = push_knobs(config, k)
    twice = 2 if groups_per_wave(k) == 2 and low.shape[0] == 64 else 1
    seen = []
    for row, _bits in test_rows(length, k):
        since = low[:, row] - k                       # errors since row k
        alive = since <= k + 1
        if not alive.any():
            return ("dead", row), seen
        counted = twice * int(alive.sum())
        if row >= push_row_solid:
            seen.append((row, counted))
            if counted <= push_max and (row >= push_row or bool((since <= solid_limit).any())):
                return ("push", row, counted, int(alive.sum())), seen
    return ("end",), seen


def routes(k, length, config, low):
    """low: band_dp(..., rows=True)[1] of the launch -> {(wave, query): route}, {(wave, query): counts seen}, and the (wave, tile)s whose
    list passed 64 - push_max in the middle of the tile: [(wave, tile, query in front of which the dense pass ran, listed pairs)]."""
    push_max = push_knobs(config, k)[3]
    nq = low.shape[0]
    q_tile = query_tile(length, k, nq)
    out, seen, flushed = {}, {}, []
    for w, (g0, n) in enumerate(waves(k)):
        for q0 in range(0, nq, q_tile):
            listed = 0
            for qi in range(q0, min(q0 + q_tile, nq)):
                if listed > 64 - push_max:            # the top of banded_cut_kernel's query loop
                    flushed.append((w, q0 // q_tile, qi, listed))
                    listed = 0
                out[w, qi], seen[w, qi] = route(low[qi, 64 * g0:64 * (g0 + n)], k, length, config)
                if out[w, qi][0] == "push":
                    listed += out[w, qi][3]
                    assert listed <= 64
    return out, seen, flushed

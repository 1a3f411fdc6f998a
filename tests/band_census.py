"""The band census — a helper, not a test: the ONE place that says which shapes, knobs and inputs launch the certified diagonal
band of the Myers global kernels at every subject length of 65 .. 256 bp.  tests/test_band_census_cpu.py proves
on the host that these shapes reach every placement of a stream event the band stream can produce and that the inputs stand
where they claim to stand; tests/test_band_census_gpu.py launches them against the DP.

Whether the band is on for a shape is the library's own answer (bgsa_hip_myers_band_half), never a rule copied here.  The
inputs come from oracle/band_edge.py: per query ONE bucket of its own, a wave (or two-group wave) in which every lane is
within B of the query, with the rungs at B - 1 and B and on the band's outermost diagonals, and a wave with exactly one lane
above B; a query is scored against its own bucket only, so what a (query, wave) does is decided by that query's ladders."""
import functools
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))

import bgsa_amd as B  # noqa: E402
import oracle as O  # noqa: E402
import rows_ir as R  # noqa: E402
from oracle import band_edge as E  # noqa: E402

LENGTHS = range(65, 257)                 # every subject length with windowed bodies: 3 .. 8 words
# m = n + d: both signs, the rescue's limit kRescueMaxDelta, one larger skew each way
DELTAS = (0, -3, 3, -11, 17)
RESCUE_DELTAS = (0, -3, 3)
# Added for the stream events (tests/test_band_census_cpu.py names what is lost without them): at +18 a window gains a word on
# either side in the same row at 6 and at 8 words; per subject length the first and the last n - m at which the library still
# bands (extreme_deltas) reach the one-word windows, the full-width window and the fewest and the most 8-byte windows.
EVENT_DELTAS = (18,)
EXTREMES = True
PAIR_MAX_LEN = 160                       # the two-group band kernels: 3 .. 5 words
BLOCK = 32                               # subject lengths per GPU test: 65 .. 96, 97 .. 128, ...
NEAR = 4
LANES = (0, 31, 32, 63)                  # where the one lane above B sits, by the shape's index
RESCUE_MAX_LANES = 8                     # myers_band.h: kRescueMaxLanes
SHARED_QUERIES = 24
SHARED_DEPTHS = [2, 3]
LARGE_BUCKET = (2000, 200000)            # (queries, subjects) of a launch that carries two groups and rescues by default

KNOBS = ("BGSA_MYERS_BAND", "BGSA_MYERS_BAND_GROUPS", "BGSA_MYERS_BAND_RESCUE", "BGSA_MYERS_BAND_RESCUE_POOL",
         "BGSA_MYERS_PREFIX_SHARE", "BGSA_TASK_TARGET", "BGSA_DYNAMIC_TASK_TARGET", "BGSA_DYNAMIC_TASKS", "BGSA_DYNAMIC_MIN_TASKS",
         "BGSA_DYNAMIC_TASK_WORDS")
_PIN = {"BGSA_MYERS_BAND_GROUPS": "2", "BGSA_MYERS_BAND_RESCUE": "1"}
# as tests/test_myers_band_rescue_gpu.py: the largest tile (sharing needs 16 queries per task) and the depths 2, 3 for every launch
_SHARE = {"BGSA_TASK_TARGET": "1", "BGSA_DYNAMIC_TASK_TARGET": "1", "BGSA_MYERS_PREFIX_SHARE": "2,3"}

# name -> knobs (every other knob of KNOBS is taken out of the child's environment), groups per wave where the band is on,
# whether the launch rescues, whether it shares prefixes, the longest subject, the deltas
CONFIGS = {
    "default": dict(env={}, groups=1, rescue=False, share=False, max_len=256, deltas=DELTAS),
    "two groups": dict(env={"BGSA_MYERS_BAND_GROUPS": "2"}, groups=2, rescue=False, share=False, max_len=PAIR_MAX_LEN, deltas=DELTAS),
    "rescue": dict(env=_PIN, groups=2, rescue=True, share=False, max_len=PAIR_MAX_LEN, deltas=RESCUE_DELTAS),
    # (+-3 beside 0: at n = m alone the streams in segments miss ('slot group', 5, 0, 4) and their fewest and most windows)
    "default shared": dict(env=_SHARE, groups=1, rescue=False, share=True, max_len=256, deltas=RESCUE_DELTAS),
    "rescue shared": dict(env=dict(_PIN, **_SHARE), groups=2, rescue=True, share=True, max_len=PAIR_MAX_LEN, deltas=RESCUE_DELTAS),
}


def child_env(config, environ):
    env = {k: v for k, v in environ.items() if k not in KNOBS}
    env.update(CONFIGS[config]["env"])
    return env


# ---- which shapes -------------------------------------------------------------------------------------------------------------
def band_on(m, n):
    return B.lib().bgsa_hip_myers_band_half(m, n) > 0


def rescues_by_default(m, n):
    """myers_band.h: band_rescue_lengths, asked of the library: a launch of LARGE_BUCKET rescues at these lengths without a knob
    (in a process that sets none: the CPU test asks in a child)."""
    return B.lib().bgsa_hip_myers_band_rescue(m, n, *LARGE_BUCKET) > 0


@functools.lru_cache(maxsize=None)
def extreme_deltas(n):
    """The smallest and the largest d at which the library runs (n + d) x n on the band."""
    on = [d for d in range(1 - n, 2 * n) if band_on(n + d, n)]
    return (on[0], on[-1])


@functools.lru_cache(maxsize=None)
def shapes(config, block=None):
    """[(m, n)] of the configuration, band on or off; block: the subject lengths 65 + 32 block .. 96 + 32 block only."""
    c = CONFIGS[config]
    lengths = [n for n in LENGTHS if n <= c["max_len"] and (block is None or (n - LENGTHS[0]) // BLOCK == block)]
    out = []
    for n in lengths:
        ds = c["deltas"] + (EVENT_DELTAS + (extreme_deltas(n) if EXTREMES else ()) if c["deltas"] is DELTAS else ())
        out += [(n + d, n) for d in dict.fromkeys(ds)]
    if c["rescue"]:      # a shape without the band has no two-group kernel to rescue on
        out = [x for x in out if band_on(*x)]
    return out


def blocks(config):
    return list(range((min(CONFIGS[config]["max_len"], LENGTHS[-1]) - LENGTHS[0]) // BLOCK + 1))


def half(config, m, n):
    """The half-width the configuration's launch runs (m, n) on; 0: band off, full rows."""
    if not band_on(m, n):
        return 0
    return B.lib().bgsa_hip_myers_band_rescue_half(max(m, n)) if CONFIGS[config]["rescue"] else B.lib().bgsa_hip_myers_band_half(m, n)


def groups(config, m, n):
    return CONFIGS[config]["groups"] if band_on(m, n) else 1


def depths(config, m, n):
    """What bgsa_hip_myers_prefix_depths must answer: the forced depths where the shape qualifies (the first three rows on words 0..1)."""
    h = half(config, m, n)
    if not CONFIGS[config]["share"] or h == 0:
        return []
    return SHARED_DEPTHS if R.myers_band_segments(np.zeros(m, np.uint8), m, n, h, (n + 31) // 32, SHARED_DEPTHS) is not None else []


# ---- which inputs -------------------------------------------------------------------------------------------------------------
def dist(q, s):
    """oracle.dp_edit as distances, once per distinct subject: a bucket's fill is 32 rows, cycled."""
    first = {}
    back = [first.setdefault(r.tobytes(), i) for i, r in enumerate(s)]
    at = {i: k for k, i in enumerate(first.values())}
    return -O.dp_edit(q, s[list(first.values())]).astype(np.int64)[:, [at[i] for i in back]]


def base_queries(m):
    return [E.three_run_query(m), E.seeded_runs_query(m, 1), E.seeded_runs_query(m, 2)]


def shared_queries(m):
    """24 queries that share their first rows, as tests/test_myers_band_rescue_gpu.py builds them: the three-run query with
    i % 6 substitutions behind row 12."""
    q0 = E.three_run_query(m)
    q = np.repeat(q0[None], SHARED_QUERIES, axis=0)
    for i in range(SHARED_QUERIES):
        for j in range(i % 6):
            at = 12 + ((7 * i + 11 * j) % (m - 14))
            q[i, at] = {ord("A"): ord("C"), ord("C"): ord("T"), ord("T"): ord("A")}[int(q[i, at])]
    return np.ascontiguousarray(q)


def case(config, m, n, index):
    """-> (queries [k, m], buckets, h, B): query i is scored against buckets[i] alone — except under prefix sharing, where the 24
    queries go through buckets[0], the bucket of the three-run query, in ONE launch.  index: the shape's position in
    its block of subject lengths (cases), which rotates the lane (and group) of the one pair above B.  A shape without the band gets the buckets of
    the default half-width of its lengths."""
    c = CONFIGS[config]
    h = half(config, m, n)
    g = groups(config, m, n)
    build_h = h or R.myers_band_half(max(m, n))
    queries = base_queries(m)[:1] if c["share"] else base_queries(m)
    buckets = []
    for i, q in enumerate(queries):
        k = index + i
        s, _, _ = E.band_edge_two_waves(q, n, build_h, dist, O.mutate, O.gen_reads, 7000 + 3 * n + i, groups=g,
                                        lane=LANES[k % 4], group=(k // 4) % g, near=NEAR)
        buckets.append(s)
    q = shared_queries(m) if c["share"] else np.stack(queries)
    return q, buckets, h, 2 * build_h + 1


def cases(config, block=None):
    """(m, n, queries, buckets, h, B) of every shape of the configuration (of one block of subject lengths)."""
    for index, (m, n) in enumerate(shapes(config, block)):
        yield (m, n) + case(config, m, n, index)


def launch_shape(config, m, n):
    """(queries, subjects) of one launch, as the selection functions of the library are asked."""
    return (SHARED_QUERIES if CONFIGS[config]["share"] else 1), 128 * groups(config, m, n)


def expected(config, q, buckets, h):
    """Per launch (want scores [k, ns] as int16 negated distances, over [k, groups]: lanes above B per 64-subject group):
    one launch per query, or one for all under prefix sharing."""
    limit = 2 * h + 1
    out = []
    if CONFIGS[config]["share"]:
        launches = [(q, buckets[0])]
    else:
        launches = [(q[i:i + 1], s) for i, s in enumerate(buckets)]
    for qq, s in launches:
        d = dist(qq, s)
        out.append(((-d).astype(np.int16), (d > limit).reshape(len(qq), -1, 64).sum(axis=2)))
    return out


def statistics(config, over, h):
    """((redone, banded), (rescued, forced)) one launch must add to the library's counts: units of (64-subject group, query)."""
    if h == 0:
        return (0, 0), (0, 0)
    if CONFIGS[config]["rescue"]:
        assert over.max() <= RESCUE_MAX_LANES
        return (0, over.size), (int(over.sum()), 0)
    return (int((over > 0).sum()), over.size), (0, 0)


# ---- stream events ------------------------------------------------------------------------------------------------------------
def _classify(stream, nw, start, into):
    """Walk one stream (or one segment) as the row loop walks it and add its event classes to `into`."""
    windows = [(a, b) for a in range(nw) for b in range(a, nw)]
    pos, before, cur = 0, start, None
    while True:
        c = stream[pos]
        if c == 5:
            into.add(("END at byte", pos & 7))
            return
        if c == 6:
            into.add(("REFILL at byte", pos & 7))
            pos, before = (pos | 7) + 1, "a REFILL"
        elif c == 7:
            into.add(("SETWIN at byte", pos & 7))
            into.add(("SETWIN behind", before))
            a, b = windows[stream[pos + 1]]
            assert R.myers_window_index(nw, a, b) == stream[pos + 1]
            into.add(("slot group", nw, a, b))
            if cur is not None and (a, b) != cur:
                into.add(("transition", nw, a - cur[0], b - cur[1]))
            cur, pos, before = (a, b), pos + 2, "a SETWIN"
        else:
            pos, before = pos + 1, "a row code"


def stream_events(m, n, h, share=()):
    """The event classes of the band stream of an m-row query against n columns at half-width h — where each SETWIN stands in
    its 8-byte window and what stands in front of it, early (byte 6) and late REFILLs, window transitions and slot groups per
    word count, where END lands — and its number of 8-byte windows.  share: the depths of a stream in segments."""
    nw = (n + 31) // 32
    codes = np.zeros(m, dtype=np.uint8)
    into = set()
    if share:
        stream, offsets = R.myers_band_segments(codes, m, n, h, nw, share)
        for j in range(len(offsets) - 1):
            _classify(stream[offsets[j]:offsets[j + 1]], nw, "the stream's start" if j == 0 else "a segment's start", into)
    else:
        stream = R.myers_band_stream(codes, m, n, h, nw)
        _classify(stream, nw, "the stream's start", into)
    return into, len(stream) // 8

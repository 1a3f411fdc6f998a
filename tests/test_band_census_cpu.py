"""The band census on the host (tests/band_census.py): what tests/test_band_census_gpu.py launches stands where it claims to.

  * Input conditions, with oracle.dp_edit only, at EVERY shape of every configuration: among the shape's queries a pair at exactly
    B and one at exactly B + 1; every lane of a query's first wave within B, exactly one lane of its second wave above B, at the
    lane and group the census rotates it to; never more than kRescueMaxLanes lanes of a group above the limit — under prefix
    sharing for each of the 24 query variants.
  * Stream events: the census reaches every placement of a band-stream event that the domain reaches — every subject length with
    every query length at which the library runs the band.  Enumerating the whole domain (63,080 shapes) took 13.4 s here against
    0.95 s of the slowest test of tests/test_myers_band_cpu.py, so the domain's n - m are strided by 29, offset by the subject
    length (2,174 shapes, 0.5 s; the test that runs first pays 1.3 s more for the helper's own scan of the first and last banded n - m).  Measured once: the strided domain reaches the same 102 classes as the whole one; of the fewest
    and most windows per word count it reaches all but the exact extremes, which the census takes from the library's first and
    last banded n - m and which are pinned below.
  * Teeth: the four broken window schedules of tests/test_myers_band_cpu.py each change the score of a certified census pair.
  * Selection: under each configuration's knobs the library names the instantiation the census claims to launch.
"""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import band_census as C  # noqa: E402
import test_myers_band_cpu as T  # noqa: E402

ROOT = C.ROOT
R = C.R

# the lengths at which a large launch rescues without a knob (myers_band.h: band_rescue_lengths)
DEFAULT_RESCUE_LENGTHS = [68, 75, 79, 82, 86, 89, 93, 96, 100, 107, 111, 114, 118, 121, 125, 128, 132, 139, 143, 146, 150, 153, 157, 160]
BAND_OFF = [(82, 93), (85, 96)]


# ---- which shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_no_shape_is_left_out(config):
    c = C.CONFIGS[config]
    shapes = C.shapes(config)
    lengths = [n for n in C.LENGTHS if n <= c["max_len"]]
    assert lengths == list(range(65, c["max_len"] + 1))
    want = {(n + d, n) for n in lengths for d in ((0, -3, 3) if c["share"] or c["rescue"] else (0, -3, 3, -11, 17))}
    assert want <= set(shapes) and len(set(shapes)) == len(shapes)
    assert sorted(x for block in C.blocks(config) for x in C.shapes(config, block)) == sorted(shapes)
    off = [x for x in shapes if not C.band_on(*x)]
    assert off == (BAND_OFF if c["deltas"] is C.DELTAS else [])
    if c["rescue"]:
        assert {n for m, n in shapes if abs(n - m) <= 3} >= set(DEFAULT_RESCUE_LENGTHS)
    if c["deltas"] is C.DELTAS:      # the first and the last banded n - m: one step further the library answers "off"
        for n in lengths:
            lo, hi = C.extreme_deltas(n)
            assert lo < -3 and hi > 18 and (n + lo, n) in shapes and (n + hi, n) in shapes and not C.band_on(n + lo - 1, n) and not C.band_on(n + hi + 1, n)


# ---- input conditions -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config,block", [(c, b) for c in C.CONFIGS for b in C.blocks(c)], ids=lambda x: str(x))
def test_input_conditions(config, block):
    c = C.CONFIGS[config]
    n_shapes = 0
    for index, (m, n, q, buckets, h, limit) in enumerate(C.cases(config, block)):
        what = f"{config}, {m} x {n}"
        g = C.groups(config, m, n)
        assert (h > 0) == C.band_on(m, n) and limit == 2 * (h or R.myers_band_half(max(m, n))) + 1, what
        launches = C.expected(config, q, buckets, (limit - 1) // 2)
        seen = set()
        for i, (want, over) in enumerate(launches):
            d = -want.astype(np.int64)
            assert d.shape == (len(q) if c["share"] else 1, 128 * g) and over.shape == (d.shape[0], 2 * g), what
            seen |= set((d - limit).ravel().tolist())
            # the query the bucket was built for: its first wave certified, exactly one lane of its second wave above B
            lane, group = C.LANES[(index + i) % 4], ((index + i) // 4) % g
            assert over[0, :g].sum() == 0 and over[0].sum() == 1 and d[0, 64 * (g + group) + lane] > limit, (what, i, over[0])
            assert (d[0, :64 * g] >= limit - 1).sum() >= 1, what                  # a rung at B - 1 or B rides in the certified wave
            assert over.max() <= C.RESCUE_MAX_LANES, (what, i, over.max(axis=1))  # sharing: every one of the 24 variants
            if h:
                C.statistics(config, over, h)
        assert {0, 1} <= seen, (what, sorted(x for x in seen if abs(x) < 6))
        assert len(launches) == (1 if c["share"] else 3)
        n_shapes += 1
    assert n_shapes == len(C.shapes(config, block)) > 0


# ---- stream events --------------------------------------------------------------------------------------------------------------
DOMAIN_STRIDE = 29


def _reach(items):
    """(event classes, {word count: (fewest, most) 8-byte windows}) of [(m, n, h, depths)]."""
    classes, windows = set(), {}
    for m, n, h, share in items:
        events, n_windows = C.stream_events(m, n, h, share)
        classes |= events
        nw = (n + 31) // 32
        lo, hi = windows.get(nw, (n_windows, n_windows))
        windows[nw] = (min(lo, n_windows), max(hi, n_windows))
    return classes, windows


def _missing(census, domain):
    (have, have_windows), (want, want_windows) = _reach(census), _reach(domain)
    gone = sorted(want - have, key=str)
    for nw, (lo, hi) in want_windows.items():
        if nw not in have_windows or have_windows[nw][0] > lo:
            gone.append(("fewest windows", nw, lo))
        if nw not in have_windows or have_windows[nw][1] < hi:
            gone.append(("most windows", nw, hi))
    return gone, have


def _census_streams(config):
    return [(m, n, C.half(config, m, n), tuple(C.depths(config, m, n))) for m, n in C.shapes(config) if C.band_on(m, n)]


@pytest.mark.parametrize("config", ["default", "two groups"])
def test_default_band_reaches_every_stream_event_of_the_domain(config):
    """(a) over 65 .. 256 bp and (b), whose kernels are others, over its own 65 .. 160 bp.  Lost without a delta of the helper (shown
    by hand): without +18, ('transition', 6, 1, 1) and ('transition', 8, 1, 1); without the extremes, fourteen slot groups — the
    one-word windows (4, 3, 3), (5, 0, 0), ..., the full window (8, 0, 7) — and the fewest and most windows of every word count."""
    L = C.B.lib()
    longest = C.CONFIGS[config]["max_len"]
    domain = []
    for n in range(65, longest + 1):
        lo, hi = C.extreme_deltas(n)
        for d in range(lo + (n - lo) % DOMAIN_STRIDE, hi + 1, DOMAIN_STRIDE):
            h = L.bgsa_hip_myers_band_half(n + d, n)
            if h > 0:
                domain.append((n + d, n, h, ()))
    assert len(domain) > (2000 if longest == 256 else 500)
    gone, have = _missing(_census_streams(config), domain)
    assert not gone, f"no census shape reaches {gone}"
    # what the census is known to reach, so that a domain that lost its reach cannot make it look complete
    assert {("SETWIN at byte", k) for k in range(6)} | {("REFILL at byte", 6), ("REFILL at byte", 7)} | {("END at byte", k) for k in range(7)} <= have
    assert {("SETWIN behind", x) for x in ("the stream's start", "a row code", "a REFILL")} <= have
    for nw in range(3, (longest + 31) // 32 + 1):      # (3 and 4 words: no window gains a word on either side in one row)
        assert {("transition", nw, 0, 1), ("transition", nw, 1, 0)} | ({("transition", nw, 1, 1)} if nw >= 5 else set()) <= have
    assert len(have) == (102 if longest == 256 else 47)


@pytest.mark.parametrize("config", ["rescue", "default shared", "rescue shared"])
def test_narrow_and_shared_streams_reach_every_stream_event_of_their_domain(config):
    """The domain of the rescue band is |n - m| <= 3 (kRescueMaxDelta), and the streams in segments are held to the same one.  At
    n = m alone the shared streams miss ('slot group', 5, 0, 4) and the fewest and most windows of 3, 4, 6 and 7 words (shown by
    hand), which is why the helper runs them at +-3 too."""
    c = C.CONFIGS[config]
    domain = []
    for n in range(65, c["max_len"] + 1):
        for d in range(-3, 4):
            if C.band_on(n + d, n):
                domain.append((n + d, n, C.half(config, n + d, n), tuple(C.depths(config, n + d, n))))
    census = _census_streams(config)
    gone, have = _missing(census, domain)
    assert not gone, f"no census shape reaches {gone}"
    if c["share"]:
        assert ("SETWIN behind", "a segment's start") in have and sum(1 for x in census if x[3]) >= 3 * 96


# ---- teeth ----------------------------------------------------------------------------------------------------------------------
# one shape per word count and sign of n - m, from (a); the rescue band at 3 .. 5 words, from (c)
TEETH = [("default", n + d, n) for n in (70, 100, 150, 181, 210, 256) for d in (-11, 0, 17)] + \
        [("rescue", n + d, n) for n, d in ((68, 0), (100, 3), (150, -3))]


@pytest.mark.parametrize("config,m,n", TEETH, ids=lambda x: str(x))
def test_census_inputs_see_a_broken_window_schedule(oracle, monkeypatch, config, m, n):
    """_assert_teeth of tests/test_myers_band_cpu.py on the census buckets: it reads its corpus from that module's cache."""
    index = C.shapes(config, (n - C.LENGTHS[0]) // C.BLOCK).index((m, n))      # as cases() counts: within the block
    q, buckets, h, limit = C.case(config, m, n, index)
    assert h > 0
    corpus = [(q[i], s, C.dist(q[i:i + 1], s)[0]) for i, s in enumerate(buckets)]
    monkeypatch.setitem(T._corpus_cache, (m, n, h, False), corpus)
    T._assert_teeth(oracle, monkeypatch, m, n, h)


# ---- selection ------------------------------------------------------------------------------------------------------------------
CHILD = r"""
import json, sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import ctypes
import band_census as C
L = C.B.lib()
L.bgsa_hip_kernel_name.restype = ctypes.c_char_p
config = sys.argv[2]
out = {"names": [L.bgsa_hip_kernel_name(C.B.ALGO_MYERS, nw).decode() for nw in range(3, 9)], "shapes": [], "default_rescue": []}
for m, n in C.shapes(config):
    nq, ns = C.launch_shape(config, m, n)
    nw = (n + 31) // 32
    d = (ctypes.c_int * 8)()
    k = L.bgsa_hip_myers_prefix_depths(nw, ns, m, n, nq, 0, d, 8)
    out["shapes"].append([int(L.bgsa_hip_myers_band_groups(nw, ns, m, n, 0)), int(L.bgsa_hip_myers_band_rescue(m, n, nq, ns)), [int(d[j]) for j in range(k)]])
    if sys.argv[3] == "large" and m == n:
        if C.rescues_by_default(m, n):
            out["default_rescue"].append(n)
print("RESULT " + json.dumps(out))
"""


def _child(config, large):
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), config, "large" if large else "-"], capture_output=True, text=True,
                       timeout=300, env=C.child_env(config, os.environ))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


@pytest.mark.parametrize("config", list(C.CONFIGS))
def test_selection_under_the_knobs_of_the_configuration(config):
    c = C.CONFIGS[config]
    r = _child(config, large=False)
    assert r["names"] == [f"myers_global_asm_kernel<{nw}, 1>" for nw in range(3, 9)]       # (the name is the small-bucket kernel's)
    shapes = C.shapes(config)
    assert len(r["shapes"]) == len(shapes)
    for (m, n), (groups, rescue_half, depths) in zip(shapes, r["shapes"]):
        what = (config, m, n, groups, rescue_half, depths)
        assert groups == C.groups(config, m, n), what
        assert rescue_half == (C.half(config, m, n) if c["rescue"] else 0), what
        assert depths == C.depths(config, m, n), what
        if c["rescue"]:
            assert rescue_half == R.myers_band_rescue_half(max(m, n)) > 0
    if c["share"]:      # sharing is live wherever the first three rows stay on words 0..1: up to 199 bp on the default band
        assert sum(1 for (m, n), x in zip(shapes, r["shapes"]) if m == n and x[2] == C.SHARED_DEPTHS) == (135 if config == "default shared" else 96)


def test_the_default_rescue_lengths_are_all_in_the_census():
    """Without a knob, at a bucket that carries two groups and rescues by its size: the 24 lengths, each in (c) with |n - m| <= 3."""
    env = {k: v for k, v in os.environ.items() if k not in C.KNOBS}
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), "rescue", "large"], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
    assert r["default_rescue"] == DEFAULT_RESCUE_LENGTHS
    assert all(x == [1, 0, []] for x in r["shapes"])            # ... and a bucket of 256 subjects does none of this by itself
    census = set(C.shapes("rescue"))
    assert all({(n, n), (n - 3, n), (n + 3, n)} <= census for n in DEFAULT_RESCUE_LENGTHS)

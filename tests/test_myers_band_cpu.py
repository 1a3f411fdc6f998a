"""The certified diagonal band of the Myers global kernels, on the CPU.

The windowed row bodies (rows_ir.py: myers_window_body) are interpreted over the band stream exactly as the generated loop
(myers_band_rows_asm) walks it, and checked against the oracle:
  * with the band off (every SETWIN picks the full window) the scores equal the DP,
  * with the band on the score D' is never below the distance D, and D' <= B = 2h + 1 implies D' = D —
    for equal and unequal lengths, 'N' bases, lengths that are not a multiple of 32, similar, random and far pairs.
The library's band stream (bgsa_hip_myers_band_stream) is walked like the loop walks it: bounds, budget, SETWIN placement.

Random and lightly mutated pairs keep their paths near the main diagonal and their distances far below B, so they see neither
the outer word of a window, nor the row at which a window gains or loses a word, nor the comparison with B.  The band-edge
pairs (oracle/band_edge.py) do: low-entropy queries against shifted copies behind a filler run, one path on every diagonal of
the band and distances on both sides of B.  On them the band is exact BOTH ways (D <= B implies D' = D; D > B implies
D' > B), and the corpus is held to having teeth: four deliberately broken window schedules must each change the score of a
certifiable pair at every shape.  The on/off rule and the stream of the library are compared with the restatement over
every subject length of 65..256 bp at the boundary values of n - m.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B
from oracle import band_edge as E

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import gen_rows_asm as G  # noqa: E402

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v


def _band_scores(q, s, h, band=True):
    """Scores of every subject in s against query q through the band stream; returns (scores, word-rows)."""
    qlen, slen = len(q), s.shape[1]
    nw = (slen + 31) // 32
    stream = R.myers_band_stream(CODE[q], qlen, slen, h, nw)
    assert stream is not None
    peq = R.build_peq32(s, nw)
    st = R.myers_init_state(nw, 1, s.shape[0])
    rows = R.run_band_stream(nw, st, peq, stream, band=band, schedule=G.ilp)   # the bodies as the generator emits them
    return -R.myers_score(st, nw, qlen, slen).astype(np.int64), rows


def _pairs(oracle, seed, qlen, slen, n=48):
    q = oracle.gen_reads(seed, 3, qlen)
    s = oracle.gen_reads(seed + 1, n, slen)
    m = min(qlen, slen)
    k = n // 3
    s[:k, :m] = oracle.mutate(q[np.arange(k) % 3][:, :m], np.arange(k) % 12, seed)   # similar pairs, 0..11 edits
    s[k, : slen // 2] = ord("N")                                                     # 'N' bases
    s[k + 1] = ord("A")                                                              # a far pair
    return q, s


SHAPES = [(150, 150), (100, 100), (96, 97), (150, 140), (140, 150), (200, 190), (256, 256), (70, 65), (181, 200)]


@pytest.mark.parametrize("qlen,slen", SHAPES)
def test_full_rows_on_the_band_stream_equal_the_oracle(oracle, qlen, slen):
    h = R.myers_band_half(max(qlen, slen))
    q, s = _pairs(oracle, 700 + qlen + slen, qlen, slen)
    want = -oracle.myers64(q, s).astype(np.int64)
    assert np.array_equal(want, -oracle.dp_edit(q, s).astype(np.int64))
    for i in range(q.shape[0]):
        got, rows = _band_scores(q[i], s, h, band=False)
        assert np.array_equal(got, want[i])
        assert rows == qlen * ((slen + 31) // 32)


@pytest.mark.parametrize("qlen,slen", SHAPES)
@pytest.mark.parametrize("shrink", [0, 20])
def test_band_is_an_upper_bound_and_exact_when_certified(oracle, qlen, slen, shrink):
    """shrink > 0: a narrower band than the default, so that random pairs fail the certificate too."""
    h = R.myers_band_half(max(qlen, slen)) - shrink
    nw = (slen + 31) // 32
    assert R.myers_band_windows(qlen, slen, h, nw) is not None
    q, s = _pairs(oracle, 900 + qlen + slen, qlen, slen)
    q[2, : qlen // 2] = ord("A")                                                     # far pairs: a half poly-A query
    want = -oracle.dp_edit(q, s).astype(np.int64)
    certified = failed = 0
    for i in range(q.shape[0]):
        got, rows = _band_scores(q[i], s, h)
        assert (got >= want[i]).all()
        ok = got <= 2 * h + 1
        assert np.array_equal(got[ok], want[i][ok])
        certified += int(ok.sum())
        failed += int((~ok).sum())
        assert rows < qlen * nw
    assert certified > 0 and failed > 0


def test_default_band_shapes():
    assert R.myers_band_half(150) == 48
    w = R.myers_band_windows(150, 150, 48, 5)
    assert sum(b - a + 1 for a, b in w) == 492          # of 750 word-rows
    assert w[0] == (0, 1) and w[16] == (0, 2) and w[-1] == (3, 4)
    assert R.myers_band_windows(150, 150, 48, 2) is None                  # no windowed bodies below three words
    assert R.myers_band_windows(300, 300, 90, 10) is None                 # ... nor above eight
    assert R.myers_band_windows(100, 250, 30, 8) is None                  # |n - m| > B
    assert R.myers_band_windows(150, 150, 0, 5) is None                   # BGSA_MYERS_BAND=0
    assert R.myers_band_windows(96, 96, 60, 3) is None                    # saves less than a fifth


def test_default_half_width_covers_random_pairs():
    """B = 2h + 1 lies more than four standard deviations above the mean distance of random ACGT pairs."""
    rng = np.random.default_rng(11)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for length in (65, 150, 256):
        nw = (length + 31) // 32
        body = R.myers_body(nw)
        d = []
        for _ in range(4):
            q = acgt[rng.integers(0, 4, length)]
            s = acgt[rng.integers(0, 4, (256, length))]
            st = R.myers_init_state(nw, 1, 256)
            R.run_rows(body, st, R.build_peq32(s, nw), q)
            d.append(-R.myers_score(st, nw, length, length).astype(np.int64))
        d = np.concatenate(d)
        assert 2 * R.myers_band_half(length) + 1 >= d.mean() + 4 * d.std()


# ---- the library's band stream ---------------------------------------------------------------------------

@pytest.fixture(scope="module")
def L():
    return B.lib()


def _lib_stream(L, row, slen):
    n = L.bgsa_hip_myers_band_stream(row.ctypes.data, len(row), slen, None, 0)
    if n == 0:
        return None
    buf = np.full(n + 64, 0xEE, dtype=np.uint8)
    assert L.bgsa_hip_myers_band_stream(row.ctypes.data, len(row), slen, buf.ctypes.data, n) == n
    assert (buf[n:] == 0xEE).all()
    return buf[:n]


def band_stride(qlen):   # myers_band.h: band_stream_stride = stream_stride(qlen + 3 * 16)
    return ((qlen + 48) // 7 + 2) * 8


def walk(raw, stride, nw):
    """The loop's walk of a band stream under the budget of `stride`: (rows, budget left, last byte loaded)."""
    n_groups = nw * (nw + 1) // 2
    padded = bytes(raw) + bytes([5]) * (stride - len(raw))
    budget = stride // 8 - 2
    ptr, touched = 0, 16
    win, nxt = list(padded[0:8]), list(padded[8:16])
    rows = 0
    while True:
        assert win, "ran off a window without REFILL"
        code = win.pop(0) & 7
        if code < 5:
            rows += 1
        elif code == 5:
            return rows, budget, touched
        elif code == 6:
            budget -= 1
            assert budget >= 0
            ptr += 8
            win, nxt = nxt, list(padded[ptr + 8:ptr + 16])
            touched = max(touched, ptr + 16)
        else:
            assert win, "SETWIN without its window byte"
            assert win.pop(0) < n_groups


@pytest.mark.parametrize("qlen,slen", SHAPES + [(1, 100), (7, 100), (300, 250), (250, 256)])
def test_library_stream_matches_the_restatement_and_its_bounds(L, qlen, slen):
    rng = np.random.default_rng(qlen * 1000 + slen)
    row = rng.integers(0, 5, qlen).astype(np.uint8)
    raw = _lib_stream(L, row, slen)
    nw = (slen + 31) // 32
    h = L.bgsa_hip_myers_band_half(qlen, slen)
    want = R.myers_band_stream(row, qlen, slen, R.myers_band_half(max(qlen, slen)), nw)
    if want is None:
        assert raw is None and h == 0
        return
    assert h == R.myers_band_half(max(qlen, slen))
    assert bytes(raw) == want
    stride = band_stride(qlen)
    assert len(raw) <= stride and len(raw) % 8 == 0
    rows, left, touched = walk(raw, stride, nw)
    assert rows == qlen and left >= 0 and touched <= stride
    for nq in (1, 3, 100):
        assert L.bgsa_hip_workspace_bytes(B.ALGO_MYERS, qlen, slen, nq) >= nq * stride
    # SETWIN and its byte never straddle a window: byte 7 of every window is REFILL or END
    assert all(raw[i] in (5, 6) for i in range(7, len(raw), 8))


def test_library_stream_far_more_switches_than_rows(L):
    """Short queries against wide subjects: every row may open a new window; the stride still holds the stream."""
    for qlen in range(1, 40):
        row = np.zeros(qlen, dtype=np.uint8)
        raw = _lib_stream(L, row, 256)
        if raw is not None:
            assert len(raw) <= band_stride(qlen)
            assert walk(raw, band_stride(qlen), 8)[0] == qlen


# ---- band-edge pairs: optimal paths along the outer diagonals, distances around B ---------------------------------------

# (query length, subject length): all widths 3..8, both signs of n - m, small and large |n - m|
EDGE_SHAPES = [(65, 65), (70, 70), (96, 97), (100, 97), (128, 128), (97, 129), (150, 150), (140, 150), (150, 140), (90, 150),
               (129, 160), (160, 129), (170, 181), (180, 190), (192, 192), (200, 210), (224, 220), (215, 224), (240, 230),
               (150, 240), (240, 150), (160, 256), (225, 256), (256, 225), (256, 256)]
# the three-run query and the seeded-runs query of seed 1; (240, 150) needs seed 2 for the upper-word-late mutant
EDGE_SEEDS = {(240, 150): (1, 2)}
NARROW_SHAPES = [(150, 150), (100, 97), (240, 256)]

_corpus_cache = {}


def _edge_corpus(oracle, qlen, slen, h, narrow=False):
    """[(query, subjects, distances)]: the full ladders and the near-B rungs of every query of the shape."""
    key = (qlen, slen, h, narrow)
    if key not in _corpus_cache:
        if narrow:   # a band this narrow: random reads are far enough apart for the shifted alignment to be optimal
            q = oracle.gen_reads(77 + qlen, 1, qlen)[0].copy()
            q[q == E.FILLER] = ord("T")
            queries = [q]
        else:
            queries = [E.three_run_query(qlen)] + [E.seeded_runs_query(qlen, s) for s in EDGE_SEEDS.get((qlen, slen), (1,))]
        out = []
        for q in queries:
            s, _ = E.band_edge_pairs(q, slen, h)
            out.append((q, s, -oracle.dp_edit(q[None], s).astype(np.int64)[0]))
        _corpus_cache[key] = out
    return _corpus_cache[key]


def _assert_exact_both_ways(oracle, qlen, slen, h, narrow=False):
    limit = 2 * h + 1
    assert R.myers_band_windows(qlen, slen, h, (slen + 31) // 32) is not None
    seen = set()
    for q, s, want in _edge_corpus(oracle, qlen, slen, h, narrow):
        got, rows = _band_scores(q, s, h)
        assert rows < qlen * ((slen + 31) // 32)
        assert (got >= want).all()
        inside = want <= limit
        assert np.array_equal(got[inside], want[inside])           # the optimal path lies inside the band
        assert (got[~inside] > limit).all()                        # ... and nothing above B is let through
        seen |= set((want - limit).tolist())
    # the input condition: a path on both sides of the certificate, one exactly at B and one at B + 1
    assert set(range(-2, 4)) <= seen, sorted(seen)


@pytest.mark.parametrize("qlen,slen", EDGE_SHAPES)
def test_band_edge_pairs_are_exact_both_ways(oracle, qlen, slen):
    _assert_exact_both_ways(oracle, qlen, slen, R.myers_band_half(max(qlen, slen)))


@pytest.mark.parametrize("qlen,slen", NARROW_SHAPES)
@pytest.mark.parametrize("h", [12, 20])
def test_band_edge_pairs_are_exact_both_ways_narrow_band(oracle, qlen, slen, h):
    _assert_exact_both_ways(oracle, qlen, slen, h, narrow=True)


def _window_mutant(kind):
    """myers_band_windows, broken on purpose: the upper word one row late, the lower word dropped one row early, windows one
    word short on the upper / on the lower side."""
    orig = R.myers_band_windows

    def windows(m, n, h, nw):
        w = orig(m, n, h, nw)
        if w is None:
            return None
        a, b = [x[0] for x in w], [x[1] for x in w]
        if kind == "upper word one row late":
            b = [b[0]] + b[:-1]
        elif kind == "lower word one row early":
            a = a[1:] + [a[-1]]
        elif kind == "one word short on the upper side":
            b = [max(x, y - 1) for x, y in zip(a, b)]
        else:
            assert kind == "one word short on the lower side"
            a = [min(y, x + 1) for x, y in zip(a, b)]
        assert all(x <= y for x, y in zip(a, b)) and list(zip(a, b)) != w
        return list(zip(a, b))

    return windows


MUTANTS = ["upper word one row late", "lower word one row early", "one word short on the upper side",
           "one word short on the lower side"]


def _assert_teeth(oracle, monkeypatch, qlen, slen, h, narrow=False):
    limit = 2 * h + 1
    corpus = _edge_corpus(oracle, qlen, slen, h, narrow)
    for kind in MUTANTS:
        with monkeypatch.context() as mp:
            mp.setattr(R, "myers_band_windows", _window_mutant(kind))
            wrong = sum(int(((_band_scores(q, s, h)[0] != want) & (want <= limit)).sum()) for q, s, want in corpus)
        assert wrong > 0, f"{qlen} x {slen}, h = {h}: no certifiable band-edge pair sees the schedule with the {kind}"


@pytest.mark.parametrize("qlen,slen", EDGE_SHAPES)
def test_band_edge_pairs_see_a_broken_window_schedule(oracle, monkeypatch, qlen, slen):
    """A condition on the inputs, checked with the DP and the interpreter only: each broken schedule changes the score of at
    least one pair with D <= B — the pairs an exact band must get right."""
    _assert_teeth(oracle, monkeypatch, qlen, slen, R.myers_band_half(max(qlen, slen)))


@pytest.mark.parametrize("qlen,slen", NARROW_SHAPES)
@pytest.mark.parametrize("h", [12, 20])
def test_band_edge_pairs_see_a_broken_window_schedule_narrow_band(oracle, monkeypatch, qlen, slen, h):
    _assert_teeth(oracle, monkeypatch, qlen, slen, h, narrow=True)


def test_band_edge_shapes_cover_every_width():
    widths = [(slen + 31) // 32 for _, slen in EDGE_SHAPES]
    assert all(widths.count(nw) >= 2 for nw in range(3, 9))


# ---- schedule sweep: the library's on/off rule and stream against the restatement ------------------------------------------

def _sweep_query_lengths(slen):
    """m = n - delta for delta in {0, +-1, +-31, +-32, +-33, +-(B - 1), +-B, +-(B + 1)}, B by the longer of the two lengths."""
    out = set()
    for qlen in range(1, slen + 400):
        d = abs(slen - qlen)
        if d in (0, 1, 31, 32, 33) or abs(d - (2 * R.myers_band_half(max(qlen, slen)) + 1)) <= 1:
            out.add(qlen)
    return sorted(out)


def test_sweep_reaches_both_sides_of_the_on_off_rule():
    for slen in (65, 150, 256):
        ds = {slen - m - (2 * R.myers_band_half(max(m, slen)) + 1) for m in _sweep_query_lengths(slen) if m < slen}
        assert {-1, 0, 1} <= ds
        ds = {m - slen - (2 * R.myers_band_half(max(m, slen)) + 1) for m in _sweep_query_lengths(slen) if m > slen}
        assert {-1, 0, 1} <= ds


@pytest.mark.parametrize("slen0", range(65, 257, 16))
def test_library_schedule_sweep_matches_the_restatement(L, slen0):
    on = off = 0
    for slen in range(slen0, min(slen0 + 16, 257)):
        nw = (slen + 31) // 32
        for qlen in _sweep_query_lengths(slen):
            h = R.myers_band_half(max(qlen, slen))
            row = ((np.arange(qlen) * 7 + slen) % 5).astype(np.uint8)
            want = R.myers_band_stream(row, qlen, slen, h, nw)
            got_h = L.bgsa_hip_myers_band_half(qlen, slen)
            assert (got_h > 0) == (want is not None), (qlen, slen)
            raw = _lib_stream(L, row, slen)
            if want is None:
                assert raw is None and got_h == 0, (qlen, slen)
                off += 1
                continue
            on += 1
            assert got_h == h and bytes(raw) == want, (qlen, slen)
            stride = band_stride(qlen)
            assert len(raw) <= stride and len(raw) % 8 == 0
            rows, left, touched = walk(raw, stride, nw)
            assert rows == qlen and left >= 0 and touched <= stride, (qlen, slen)
            assert all(raw[i] in (5, 6) for i in range(7, len(raw), 8)), (qlen, slen)
    assert on > 0 and off > 0

"""Early leave of the certified Myers band (myers_band.h, LABNOTES §37), on the CPU.

A launch that rescues lets the low words of the window leave before the static band does — behind a cut (row r, word w) the
window begins at word w + 1 — and certifies every lane against min(B, M), M = D'[r][j_r] + (r - j_r), j_r = 32 (w + 1).

Checked here, without a GPU: the schedule (460 against 474 word-rows at 150 x 150, h = 45) on the library's stream and on the
restatement, byte for byte, whole and in the segments of prefix sharing; every length of the table; the selection
(bgsa_hip_myers_band_early) on both sides of each condition and under both knobs; and the host model — the rows_ir interpreter
on the early-leave stream with the per-lane limit (rows_ir.run_band_early) — against oracle.dp_edit: for every pair either
D' > limit or D' = D, never certified and wrong.

The rotations s = q[k:] + q[:k], k = 30 .. 45: their path along diagonal -k enters the dropped region from k = 35 on (row 131,
column 131 - k <= 96).  Where that path is the optimum (D = 2k: k = 35 .. 41 with the seeds used here) the lane cannot come out
below its limit, since such a path costs at least M: k = 35 .. 40 come out above it, k = 41 exactly on it (D' = D = M = 82),
certified and right.  For k <= 34 the path stays in computed cells and for k >= 42 a cheaper alignment exists elsewhere
(D = 84, 84, 84, 83 < 2k), so those lanes are certified with D' = D — which is what the invariant asks of them.
"""
import ctypes
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bgsa_amd as B
from oracle import band_edge as E

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "bgsa_amd" / "csrc"))
import rows_ir as R  # noqa: E402
import gen_rows_asm as G  # noqa: E402

CODE = np.zeros(256, dtype=np.uint8)
for _c, _v in zip(b"ACGTN", range(5)):
    CODE[_c] = _v
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

KNOBS = ("BGSA_MYERS_BAND", "BGSA_MYERS_BAND_GROUPS", "BGSA_MYERS_BAND_RESCUE", "BGSA_MYERS_BAND_RESCUE_POOL", "BGSA_MYERS_BAND_EARLY",
         "BGSA_MYERS_PREFIX_SHARE")
MODEL_LENGTHS = (150, 100, 68)      # five words, and the shortest four- and three-word lengths of the table


def _ints(values):
    return (ctypes.c_int * len(values))(*values)


def _library_stream(mapped, length, h, cuts, depths=()):
    L = B.lib()
    rows, words = _ints([r for r, _ in cuts]), _ints([w for _, w in cuts])
    d = _ints(list(depths)) if depths else None
    off = (ctypes.c_int * (len(depths) + 2))()
    args = (mapped.ctypes.data_as(ctypes.c_void_p), length, h, rows, words, len(cuts), d, len(depths))
    n = L.bgsa_hip_myers_band_early_segments(*args, None, 0, off)
    if n <= 0:
        return None, None
    buf = (ctypes.c_ubyte * n)()
    assert L.bgsa_hip_myers_band_early_segments(*args, buf, n, off) == n
    return bytes(buf), list(off)


def _word_rows(stream, nw):
    """Word-rows of a band stream, walked as the row loop walks it."""
    windows = [(a, b) for a in range(nw) for b in range(a, nw)]
    pos, rows, words, width = 0, 0, 0, None
    while stream[pos] != 5:
        c = stream[pos]
        if c == 6:
            pos = (pos | 7) + 1
        elif c == 7:
            a, b = windows[stream[pos + 1]]
            width = b - a + 1
            pos += 2
        else:
            rows, words, pos = rows + 1, words + width, pos + 1
    return rows, words


def test_schedule_at_150_is_460_of_474_word_rows_byte_for_byte():
    L = B.lib()
    cuts = R.myers_band_early_cuts(150, 45)
    assert cuts == ((106, 1), (130, 2))
    rows, words = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
    assert L.bgsa_hip_myers_band_early_cuts(150, 45, rows, words) == 2 and list(zip(rows, words)) == list(cuts)
    assert L.bgsa_hip_myers_band_early_cuts(150, 48, rows, words) == 0 and R.myers_band_early_cuts(150, 48) == ()
    win = R.myers_band_windows(150, 150, 45, 5, cuts)
    assert sum(b - a + 1 for a, b in R.myers_band_windows(150, 150, 45, 5)) == 474
    assert sum(b - a + 1 for a, b in win) == 460
    assert win[105] == (1, 4) and win[106] == (2, 4) and win[129] == (2, 4) and win[130] == (3, 4)      # 0-based rows
    assert set(win[106:]) == {(2, 4), (3, 4)}
    rng = np.random.default_rng(150)
    for mapped in (np.zeros(150, dtype=np.uint8), rng.integers(0, 5, 150).astype(np.uint8)):
        got, off = _library_stream(mapped, 150, 45, cuts)
        assert got == R.myers_band_stream(mapped, 150, 150, 45, 5, cuts) and off == [0, len(got)]
        assert _word_rows(got, 5) == (150, 460)
        assert _word_rows(R.myers_band_stream(mapped, 150, 150, 45, 5), 5) == (150, 474)
        # in the segments of prefix sharing: the depths lie in front of every cut
        got, off = _library_stream(mapped, 150, 45, cuts, (2, 3, 6))
        want, offsets = R.myers_band_segments(mapped, 150, 150, 45, 5, (2, 3, 6), cuts)
        assert got == want and off == offsets
        assert sum(_word_rows(got[o:], 5)[1] for o in offsets[:-1]) == 460
    # the static stream's answers for today's arguments: untouched by the table (default half-width 48)
    plain = (ctypes.c_ubyte * 512)()
    mapped = np.zeros(150, dtype=np.uint8)
    n = L.bgsa_hip_myers_band_stream(mapped.ctypes.data_as(ctypes.c_void_p), 150, 150, plain, 512)
    assert bytes(plain[:n]) == R.myers_band_stream(mapped, 150, 150, R.myers_band_half(150), 5)


def test_cuts_that_are_no_schedule_are_refused():
    mapped = np.zeros(150, dtype=np.uint8)
    for bad in (((130, 2), (106, 1)), ((106, 2), (130, 1)), ((60, 1), (130, 2)), ((106, 1), (150, 2)), ((106, 4),), ((106, 1), (130, 1))):
        assert R.myers_band_windows(150, 150, 45, 5, bad) is None, bad
        assert _library_stream(mapped, 150, 45, bad) == (None, None), bad
    # a cut that only repeats the static rule changes nothing
    assert R.myers_band_windows(150, 150, 45, 5, ((109, 1), (141, 2))) == R.myers_band_windows(150, 150, 45, 5)


def test_every_table_length():
    L = B.lib()
    seen = []
    for length in range(65, 161):
        h, nw = R.myers_band_rescue_half(length), (length + 31) // 32
        rows, words = (ctypes.c_int * 2)(), (ctypes.c_int * 2)()
        n = L.bgsa_hip_myers_band_early_cuts(length, h, rows, words)
        cuts = R.myers_band_early_cuts(length, h)
        assert list(zip(rows[:n], words[:n])) == list(cuts), length
        if not cuts:
            continue
        seen.append(length)
        assert (9 * length + 192) % 32 < 8                                  # myers_band.h: band_rescue_lengths
        base, win = R.myers_band_windows(length, length, h, nw), R.myers_band_windows(length, length, h, nw, cuts)
        assert win is not None and all(0 <= a <= b < nw for a, b in win)    # the generator emits every window a <= b < nw
        assert all(w[1] == v[1] and w[0] >= v[0] for w, v in zip(win, base))
        saved = sum(b - a + 1 for a, b in base) - sum(b - a + 1 for a, b in win)
        assert 50 * saved >= sum(b - a + 1 for a, b in base), length         # at least 2 % of the word-rows
        assert 1 + sum(1 for x, y in zip(win, win[1:]) if x != y) <= 16     # myers_band.h: kBandMaxSwitches
        mapped = np.full(length, 3, dtype=np.uint8)
        got, off = _library_stream(mapped, length, h, cuts)
        assert got == R.myers_band_stream(mapped, length, length, h, nw, cuts)
        assert len(got) <= len(R.myers_band_stream(mapped, length, length, h, nw)) + 8      # a REFILL may move by a window; the stride has 3 bytes per switch
        got, off = _library_stream(mapped, length, h, cuts, (1, 2, 3, 4, 5))
        want, offsets = R.myers_band_segments(mapped, length, length, h, nw, (1, 2, 3, 4, 5), cuts)
        assert got == want and off == offsets and len(got) <= len(R.myers_band_stream(mapped, length, length, h, nw)) + 8 + 16 * 5
    assert 150 in seen and set(MODEL_LENGTHS) <= set(seen)
    assert min(x for x in seen if x > 96) == 100 and min(seen) == 68


CHILD = r"""
import ctypes, json, sys
sys.path.insert(0, sys.argv[1])
import bgsa_amd as B
L = B.lib()
out = []
for case in json.loads(sys.argv[2]):
    rows = (ctypes.c_int * 2)()
    n = int(L.bgsa_hip_myers_band_early(*case, rows))
    out.append(list(rows[:n]))
print("RESULT " + json.dumps(out))
"""


def _early(cases, **env_extra):
    """bgsa_hip_myers_band_early(ref_len, read_len, n_queries, read_count) per case, in a process of its own: the knobs are read once."""
    env = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env.update(env_extra)
    p = subprocess.run([sys.executable, "-c", CHILD, str(ROOT), json.dumps(cases)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])


def test_selection_on_both_sides_of_its_conditions():
    cases = [
        (150, 150, 2000, 200000),                              # rescues by the default rule, n = m, a length with cuts
        (150, 150, 999, 200000), (150, 150, 1000, 200000),     # the rescue's own conditions: queries ...
        (150, 150, 2000, 64 * 1953),                           # ... and the bucket
        (150, 147, 2000, 200000), (147, 150, 2000, 200000),    # n != m rescues, and keeps the static schedule
        (75, 75, 2000, 200000),                                # a rescue length without cuts
        (100, 100, 2000, 200000), (68, 68, 2000, 200000), (160, 160, 2000, 200000),
        (161, 161, 2000, 200000),
    ]
    assert _early(cases) == [[106, 130], [], [106, 130], [], [], [], [], [62, 85], [51], [106, 129], []]


def test_selection_knobs():
    cases = [(150, 150, 2000, 200000), (150, 150, 100, 200000), (150, 150, 100, 192), (75, 75, 2000, 200000), (150, 149, 2000, 200000)]
    assert _early(cases, BGSA_MYERS_BAND_EARLY="0") == [[], [], [], [], []]
    # forced rescue alone leaves it off: the tests that force rescue count the lanes of the plain rescue band
    assert _early(cases, BGSA_MYERS_BAND_RESCUE="1") == [[], [], [], [], []]
    # forced on: every rescuing launch with a table entry — which a launch is by the default rule, or by the rescue's knob
    assert _early(cases, BGSA_MYERS_BAND_EARLY="1") == [[106, 130], [], [], [], []]
    assert _early(cases, BGSA_MYERS_BAND_EARLY="1", BGSA_MYERS_BAND_RESCUE="1") == [[106, 130], [106, 130], [], [], []]
    assert _early(cases, BGSA_MYERS_BAND_EARLY="1", BGSA_MYERS_BAND_RESCUE="1", BGSA_MYERS_BAND_GROUPS="2") == [[106, 130], [106, 130], [106, 130], [], []]
    assert _early(cases, BGSA_MYERS_BAND_EARLY="1", BGSA_MYERS_BAND_RESCUE="0") == [[], [], [], [], []]
    # the table's rows belong to the rescue half-width: another band has no cuts
    assert _early(cases, BGSA_MYERS_BAND_EARLY="1", BGSA_MYERS_BAND_RESCUE="1", BGSA_MYERS_BAND="40") == [[], [], [], [], []]


# ---- the host model against the DP ---------------------------------------------------------------------------------------------

def _edits(q, rng, count):
    """A copy of q with `count` random edits, brought back to q's length at its end."""
    s = list(q)
    for _ in range(count):
        kind, at = int(rng.integers(0, 3)), int(rng.integers(0, len(s)))
        if kind == 0:
            s[at] = int(ACGT[(int(np.where(ACGT == s[at])[0][0]) + 1 + int(rng.integers(0, 3))) % 4]) if s[at] in ACGT else int(ACGT[0])
        elif kind == 1:
            s.insert(at, int(rng.choice(ACGT)))
        else:
            del s[at]
    s = s[:len(q)] + [int(c) for c in rng.choice(ACGT, max(0, len(q) - len(s)))]
    return np.array(s, dtype=np.uint8)


def _model(q, s, h, cuts):
    length, nw = len(q), (len(q) + 31) // 32
    score, limit, rows = R.run_band_early(nw, R.build_peq32(s, nw), CODE[q], length, h, cuts, schedule=G.ilp)   # the bodies as the generator emits them
    assert rows == sum(b - a + 1 for a, b in R.myers_band_windows(length, length, h, nw, cuts))
    return score[0], limit[0]


def _check(oracle, q, s, h, cuts):
    """The invariant on every lane; returns (D', limit, D)."""
    got, limit = _model(q, s, h, cuts)
    want = -oracle.dp_edit(q[None], s).astype(np.int64)[0]
    assert (limit <= 2 * h + 1).all() and (got >= want).all()
    certified = got <= limit
    assert np.array_equal(got[certified], want[certified]), "certified and wrong"
    return got, limit, want


@pytest.mark.parametrize("length", MODEL_LENGTHS)
def test_model_is_never_certified_and_wrong(oracle, length):
    h = R.myers_band_rescue_half(length)
    B_ = 2 * h + 1
    cuts = R.myers_band_early_cuts(length, h)
    assert cuts and (length, h, cuts) in ((150, 45, ((106, 1), (130, 2))), (100, 31, ((62, 0), (85, 1))), (68, 22, ((51, 0),)))
    rng = np.random.default_rng(length)
    q = rng.choice(ACGT, length)
    # random subjects
    got, limit, want = _check(oracle, q, rng.choice(ACGT, (1024, length)), h, cuts)
    assert (got > limit).sum() >= (want > B_).sum()
    # identical and 1 .. 5 edits: all certified
    near = np.stack([_edits(q, rng, e) for e in range(6) for _ in range(8)])
    got, limit, want = _check(oracle, q, near, h, cuts)
    assert want[0] == 0 and (got <= limit).all() and (want <= 10).all()
    if length == 150:
        assert limit[0] == 68                                               # an identical pair: M = 42 + 42 behind row 106, 34 + 34 behind row 130
    # rotations: the path on diagonal -k crosses the dropped region from some k on (module docstring)
    ks = list(range(30, 46)) if length == 150 else list(range(h - 15, h + 1))
    rot = np.stack([np.concatenate([q[k:], q[:k]]) for k in ks])
    got, limit, want = _check(oracle, q, rot, h, cuts)
    crosses = np.array([any(r + 1 - k <= 32 * (w + 1) for r, w in cuts) for k in ks])
    on_diagonal = want == 2 * np.array(ks)
    must = crosses & on_diagonal & (want <= B_)
    # an optimal path through the dropped region costs at least M: such a lane cannot lie below its limit, and it lies above it
    # unless D' = D = M exactly
    assert (got[must] >= limit[must]).all(), (got.tolist(), limit.tolist(), want.tolist())
    above = must & (got > limit)
    assert above.sum() >= (4 if length > 96 else 2), (ks, got.tolist(), limit.tolist(), want.tolist())      # the input condition (68 bp: only k = 20 .. 22 cross and stay within B)
    if length == 150:
        assert [k for k, m in zip(ks, must) if m] == list(range(35, 42)) and [k for k, m in zip(ks, above) if m] == list(range(35, 41))
    # the band-edge families, a path on every diagonal of the band
    seen_over, seen_cut = 0, 0
    for qe in (E.three_run_query(length), E.seeded_runs_query(length, 1)):
        s, _ = E.band_edge_pairs(qe, length, h)
        got, limit, want = _check(oracle, qe, s, h, cuts)
        seen_over += int((want > B_).sum())
        seen_cut += int(((got > limit) & (want <= B_)).sum())
        assert (got[want > B_] > limit[want > B_]).all()
    assert seen_over > 0 and seen_cut > 0                                   # both kinds of uncertified lane occur

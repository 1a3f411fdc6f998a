"""The width census on the MI355X: every BitPAl instantiation of every compiled score set (static grid and counter grid,
global and semi-global), every length-aware (LENS) width of Myers and BitPAl, and every align_pairs / align_pairs_banded width
is launched on the shapes of tests/width_census.py and compared bit for bit with the DP oracle (scores) or the canonical
traceback (edit scripts).  tests/test_width_census_cpu.py proves on the host that those shapes reach every kernel name the
dispatch can produce."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402
import oracle as O  # noqa: E402
import width_census as W  # noqa: E402
from test_align_pairs_banded_gpu import assert_banded_exact  # noqa: E402
from test_align_pairs_gpu import SENT, _aligner, _np, _sentinels, assert_pairs_exact  # noqa: E402
from test_ragged_gpu import _refused, by_class, equal_length_path, ragged_scores  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = Path(B.__file__).resolve().parent.parent
DEFAULT_FLAVOUR_SETS = {(2, -3, -5), (1, -1, -2), (1, -4, -2), (10, -9, -15), (0, -1, -1)}
EDIT_SET = (0, -1, -1)   # global mode runs on the Myers body (capi.hip make_plan): test_every_listed_myers_width_is_launched


def _sets():
    """The compiled score sets of the loaded library; under BGSA_TEST_SETS=ab_only (the child pytest of
    test_bitpal_sets_of_the_ab_flavour, which loads libbgsa_hip_ab.so) only those the default flavour does not carry."""
    if not B.LIB_PATH.exists():
        return []
    sets = B.score_sets()
    if os.environ.get("BGSA_TEST_SETS") == "ab_only":
        sets = [x for x in sets if x not in DEFAULT_FLAVOUR_SETS]
    return sets


def _bitpal_modes():
    return [(scores, semi) for scores in _sets() for semi in (False, True) if (scores, semi) != (EDIT_SET, False)]


def _ids(x):
    return "/".join(map(str, x)) if isinstance(x, tuple) else {True: "semi-global", False: "global"}.get(x, str(x))


def _names(scores, semi):
    L = B.lib()
    names = W.bitpal_names(L, scores, semi)
    B.check(L.bgsa_hip_select_algorithm(B.ALGO_MYERS), "select_algorithm")     # the process-global selection as it was
    B.check(L.bgsa_hip_select_alignment(0), "select_alignment")
    return names


# ---- BitPAl: every census case of one (score set, mode) ---------------------------------------------------------------------------
def score_bitpal_census(scores, semi):
    """Returns the number of cases; raises on the first mismatch, naming set, mode, word count, shape and kernel."""
    names = _names(scores, semi)
    cases = W.scoring_cases(names, semi)
    for w, qlen, slen in cases:
        q, s = W.scoring_case(w, qlen, slen, semi)
        got = B.align_all_pairs(q, s, algo=B.ALGO_BITPAL, scores=scores, semi_global=semi)
        want = (O.dp_semiglobal if semi else O.dp_nw)(q, s, *scores)
        what = f"BitPAl {_ids(scores)} {_ids(semi)}, {w} words, {qlen} x {slen} bp, {names[w - 1]}"
        assert got.shape == want.shape and got.dtype == np.int16, what
        assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} of {want.size} scores differ from the DP, first at " \
                                          f"(query, subject) {tuple(int(x) for x in np.argwhere(got != want)[0])}"
        if scores == (2, -3, -5) and not semi:
            assert np.array_equal(got, O.bitpal(q, s)), f"{what}: differs from the restated reference kernel"
    assert B.lib().bgsa_hip_stream_faults(1) == 0, B.lib().bgsa_hip_last_error().decode()
    return len(cases)


def score_every_bitpal_census():
    return sum(score_bitpal_census(scores, semi) for scores, semi in _bitpal_modes())


@pytest.mark.parametrize("scores,semi", _bitpal_modes(), ids=_ids)
def test_bitpal_static_grid(scores, semi):
    assert score_bitpal_census(scores, semi) >= 3 * 18
    assert B.lib().bgsa_hip_stream_faults(1) == 0


_COUNTER_CHILD = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
                  "import oracle, test_width_census_gpu as T\n"
                  "oracle.lib(); print('bitpal census ok:', T.score_every_bitpal_census(), 'cases')\n")


def test_bitpal_counter_grid():
    """The same cases in a child with BGSA_DYNAMIC_MIN_TASKS=1, where every launch that has a counter (DYN) instantiation takes
    it (the grid helper's persistent branch), as test_every_listed_myers_width_is_launched does for Myers."""
    p = subprocess.run([sys.executable, "-c", _COUNTER_CHILD, str(ROOT)], env=dict(os.environ, BGSA_DYNAMIC_MIN_TASKS="1"),
                       capture_output=True, text=True, timeout=300, cwd=str(ROOT))
    assert p.returncode == 0 and "bitpal census ok:" in p.stdout, p.stdout[-2000:] + p.stderr[-3000:]
    assert int(p.stdout.split("bitpal census ok:")[1].split()[0]) == sum(len(W.scoring_cases(_names(*m), m[1])) for m in _bitpal_modes())


def test_bitpal_sets_of_the_ab_flavour():
    """1/-3/-2 and 5/-4/-10 ship in the A/B flavour only: their static-grid and counter-grid census runs against that library,
    in a child pytest."""
    assert B.LIB_AB_PATH.exists(), "libbgsa_hip_ab.so is not built"
    env = dict(os.environ, BGSA_HIP_LIB=str(B.LIB_AB_PATH), BGSA_TEST_SETS="ab_only")
    p = subprocess.run([sys.executable, "-m", "pytest", str(ROOT / "tests" / "test_width_census_gpu.py"), "-m", "gpu", "-x", "-q", "-k",
                        "test_bitpal_static_grid or test_bitpal_counter_grid"],
                       env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
    assert " passed" in p.stdout and " failed" not in p.stdout
    n = int(p.stdout.strip().splitlines()[-1].split(" passed")[0].split()[-1])
    assert n == 2 * 2 + 1, p.stdout[-500:]          # two sets x (global, semi-global) + the counter grid: nothing deselected in silence


# ---- LENS: mixed-length buckets ---------------------------------------------------------------------------------------------------
def _lens_check(w, algo, scores, reference, sign=1):
    q, subjects = W.lens_bucket(w)
    want = sign * by_class(reference, q, subjects)
    assert B.word_num(algo, q.shape[1], max(x.size for x in subjects)) == w
    what = f"LENS {'Myers' if algo == B.ALGO_MYERS else 'BitPAl'} {scores}, {w} words"
    got = ragged_scores(q, subjects, algo, scores)      # asserts that the bucket carries per-subject lengths
    assert np.array_equal(got, want), f"{what}: {int((got != want).sum())} scores differ from the DP on the unpadded subjects"
    assert np.array_equal(got, equal_length_path(q, subjects, algo, scores)), f"{what}: differs from the equal-length path"


@pytest.mark.parametrize("w", W.LENS_WORDS_MYERS)
def test_lens_myers(w):
    _lens_check(w, B.ALGO_MYERS, None, O.dp_edit)
    if w in (2, 13, 32):                            # +distance: the pair rows, a middle width, the widest
        _lens_check(w, B.ALGO_MYERS, (0, 1, 1), O.dp_edit, sign=-1)


@pytest.mark.parametrize("scores", [x for x in _sets() if x != EDIT_SET], ids=_ids)
def test_lens_bitpal(scores):
    plain = W.max_plain(_names(scores, False))
    assert plain >= 4
    for w in range(1, plain + 1):
        _lens_check(w, B.ALGO_BITPAL, scores, lambda q, rows: O.dp_nw(q, rows, *scores))
    # the first word count beyond the register-resident kernel: refused, nothing written
    q, subjects = W.lens_bucket(plain + 1)
    a = B.DeviceAligner(B.ALGO_BITPAL, "cuda:0", 0, scores)
    a.set_queries(q)
    a.set_subjects_ragged(subjects)
    assert a.wn == plain + 1
    _refused(a, f"reaches {plain} words, the bucket has {plain + 1}")


# ---- align_pairs: every word count 1 .. 32 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", W.PAIR_WORDS)
def test_align_pairs(w):
    import torch
    for m, n in W.pair_shapes(w):
        q, s = W.pair_case(m, n)
        want = A.canonical(q, s)
        a = _aligner(q, s)
        assert a.wn == w
        pairs, cap = q.shape[0], m + n
        idx = torch.arange(pairs, device="cuda")
        got = _np(a.align_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))          # one call, the default workspace
        scores = a.score().cpu().numpy()[np.arange(pairs), np.arange(pairs)]
        a.check_faults()
        assert_pairs_exact(got, want, cap, q, s, scores, f"(align_pairs, {w} words, {m} x {n})")   # validates every script too


# ---- align_pairs_banded: every window width 1 .. 32 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("v", W.BAND_WORDS)
def test_align_pairs_banded(v):
    import torch
    m, n, bound = W.band_triples()[v]
    assert B.lib().bgsa_hip_align_pairs_band_words(m, n, bound) == v
    q, s = W.band_case(m, n, bound)
    want = A.canonical(q, s)
    inside = np.array([d <= bound for d, _ in want])
    assert inside.any() and not inside.all()
    a = _aligner(q, s)
    pairs, cap = q.shape[0], m + n
    idx = torch.arange(pairs, device="cuda")
    full = _np(a.align_pairs(idx, idx, into=_sentinels(torch, pairs, cap)))
    band = _np(a.align_pairs_banded(idx, idx, bound, into=_sentinels(torch, pairs, cap)))
    a.check_faults()                                                                    # BGSA_HIP_FAULT_BAND included
    what = f"(align_pairs_banded, window of {v} words, {m} x {n}, B = {bound})"
    for x, y in zip(full, band):
        assert x[inside].tobytes() == y[inside].tobytes(), f"pairs within the bound differ from align_pairs {what}"
    assert (band[0][~inside] == B.DISTANCE_BEYOND).all() and (band[1][~inside] == 0).all() and (band[2][~inside] == SENT).all(), what
    assert_banded_exact(band, want, bound, cap, q, s, what=what)

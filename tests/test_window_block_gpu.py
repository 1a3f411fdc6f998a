"""The windowed block of 32 rows on the MI355X where both of its users run the same small shape: 128 pairs of a 33 bp read
against 64 bp queries through bgsa_hip_myers_place_pairs_banded_dev and bgsa_hip_myers_align_pairs_banded_dev.  33 bp are two
window words; the placement's virtual rows (33 + B) are two blocks, the second partial, and at B = 0 its window starts at word 1
(the low edge crosses a word); the global band of 64 rows exists only at B = 33 (|n - m| = 31): at B = 0 and 3 the global call
launches its beyond kernel alone, so one of its three cases runs the forward kernel.  Every output against the integer
models tests/place_reference.py and tests/banded_align_reference.py, which restate the row (myers_word, the class masks), the
windows and the score of the stored state."""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import align_reference as A  # noqa: E402
import banded_align_reference as G  # noqa: E402
import bgsa_amd as B  # noqa: E402
import place_reference as P  # noqa: E402
from test_place_pairs_banded_gpu import ACGT, SENT, plant  # noqa: E402

pytestmark = pytest.mark.gpu

M, N, PAIRS = 64, 33, 128
BOUNDS = (0, 3, 33)
BEYOND = -2


@pytest.fixture(scope="module")
def torch_gpu():
    import torch
    assert torch.cuda.is_available(), "no GPU visible"
    B.lib()
    B.check(B.lib().bgsa_hip_set_device(0), "set_device")
    return torch


@functools.lru_cache(maxsize=None)
def case():
    """The pairs and both models' answers at every bound, computed once: reads planted mid-query (every start, so every
    alignment of the read's two words to the query's rows), hanging off its start and its end, with 0..4 edits, and unrelated."""
    rng = np.random.default_rng(6433)
    q = ACGT[rng.integers(4, size=(PAIRS, M))]
    s = np.empty((PAIRS, N), np.uint8)
    for p in range(PAIRS):
        kind = ("mid", "mid", "start", "end", "mid", "unrelated")[p % 6]
        s[p] = plant(rng, q[p], N, kind, (p // 6) % 5, at=p % (M - N + 1), hang=1 + p % 4)
    return q, s, {b: P.place_rows(q, s, b) for b in BOUNDS}, {b: G.align_rows(q, s, b) for b in BOUNDS}


def _aligner(q, s, semi_global):
    a = B.DeviceAligner(B.ALGO_MYERS, "cuda:0", semi_global=semi_global)
    a.set_queries(q)
    a.set_subjects(s)
    return a


def _full(torch, *shape):
    return torch.full(shape, SENT, dtype=torch.int32, device="cuda")


def _runs(cigar_row, n_ops):
    return A.unpack(cigar_row.view(np.uint32)[:n_ops])


def test_the_inputs_reach_every_branch():
    _, _, placed, aligned = case()
    assert P.band_words(N, 0) == 1 and P.band_words(N, 3) == 2 and P.block_windows(N, 0)[1][0] == 1    # the low edge crosses a word
    assert G.band_words(M, N, 0) == G.band_words(M, N, 3) == 0 and G.band_words(M, N, 33) == 2
    assert sum(w[2] is not None for w in placed[0]) >= 10 and sum(w[2] is None for w in placed[0]) >= 60
    assert sum(w[2] is not None for w in placed[3]) >= 40 and sum(w[2] is None for w in placed[3]) >= 20
    assert all(w[2] is not None for w in placed[33])
    assert sum(w[0] is not None for w in aligned[33]) >= 30 and sum(w[0] is None for w in aligned[33]) >= 20
    assert any(w[3] and w[3][0][1] == A.OP_D for w in placed[3]) and any(w[1] == M for w in placed[3])   # off the start, at the last row


@pytest.mark.parametrize("bound", BOUNDS)
def test_placement_equals_the_integer_model(torch_gpu, bound):
    torch = torch_gpu
    q, s, placed, _ = case()
    a = _aligner(q, s, True)
    idx = np.arange(PAIRS)
    cap = M + N
    into = (_full(torch, PAIRS), _full(torch, PAIRS, 4), _full(torch, PAIRS), _full(torch, PAIRS, cap))
    distance, span, n_ops, cigar = (t.cpu().numpy() for t in a.place_pairs_banded(idx, idx, bound, into=into))
    a.check_faults()
    for p, (dstar, e, q_begin, runs, _) in enumerate(placed[bound]):
        assert distance[p] == dstar, f"pair {p}: distance {distance[p]}, the model {dstar}"
        if q_begin is None:
            assert span[p].tolist() == [-1, e, 0, N] and n_ops[p] == 0 and (cigar[p] == SENT).all(), f"pair {p} beyond B = {bound}"
        else:
            assert span[p].tolist() == [q_begin, e, 0, N], f"pair {p}: span {span[p].tolist()}, the model {(q_begin, e, 0, N)}"
            assert n_ops[p] == len(runs) and _runs(cigar[p], n_ops[p]) == runs, f"pair {p}: {A.to_string(_runs(cigar[p], n_ops[p]))} != {A.to_string(runs)}"
            assert (cigar[p, n_ops[p]:] == SENT).all(), f"pair {p}: a slot behind the runs was written"


@pytest.mark.parametrize("bound", BOUNDS)
def test_global_band_equals_the_integer_model(torch_gpu, bound):
    torch = torch_gpu
    q, s, _, aligned = case()
    a = _aligner(q, s, False)
    idx = np.arange(PAIRS)
    cap = M + N
    into = (_full(torch, PAIRS), _full(torch, PAIRS), _full(torch, PAIRS, cap))
    distance, n_ops, cigar = (t.cpu().numpy() for t in a.align_pairs_banded(idx, idx, bound, into=into))
    a.check_faults()
    for p, (dist, runs, _) in enumerate(aligned[bound]):
        if dist is None:
            assert distance[p] == BEYOND and n_ops[p] == 0 and (cigar[p] == SENT).all(), f"pair {p} beyond B = {bound}: {distance[p]} / {n_ops[p]}"
        else:
            assert distance[p] == dist, f"pair {p}: distance {distance[p]}, the model {dist}"
            assert n_ops[p] == len(runs) and _runs(cigar[p], n_ops[p]) == runs, f"pair {p}: {A.to_string(_runs(cigar[p], n_ops[p]))} != {A.to_string(runs)}"
            assert (cigar[p, n_ops[p]:] == SENT).all(), f"pair {p}: a slot behind the runs was written"

"""Pair alignment without a GPU: the reference traceback of tests/align_reference.py against the oracle's DP, and the C
ABI's argument checks (they come before any HIP call), `n_pairs == 0`, and the workspace sizes."""
import ctypes
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import align_reference as A  # noqa: E402
import bgsa_amd as B  # noqa: E402

EINVAL, EUNSUPPORTED = -1, -2
P = 0x10000   # a non-null "device pointer": every call below must return before it is looked at


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists():
        B.build_library()
    return B.lib()


# ---- the reference traceback itself ---------------------------------------------------------------------------------
def _check_pairs(oracle, pairs):
    for q, s in pairs:
        q, s = np.frombuffer(q, np.uint8) if isinstance(q, bytes) else q, np.frombuffer(s, np.uint8) if isinstance(s, bytes) else s
        (distance, runs), = A.canonical(q[None, :], s[None, :])
        A.validate(q, s, distance, runs)
        assert distance == -int(oracle.dp_edit(q[None, :], s[None, :])[0, 0]), (q.tobytes(), s.tobytes())
        assert A.from_string(A.to_string(runs)) == runs and A.unpack(A.pack(runs)) == runs


def test_reference_traceback_is_valid_and_as_far_as_the_oracle_says(oracle):
    rng = np.random.default_rng(0xA11C)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    pairs = []
    for t in range(300):
        m, n = int(rng.integers(1, 201)), int(rng.integers(1, 201))
        q = acgt[rng.integers(0, 4, m)]
        if t % 3 == 0:                                  # unrelated reads of unequal lengths
            s = acgt[rng.integers(0, 4, n)]
        else:                                           # a mutated copy, cut or extended to n: m != n among them
            s = oracle.mutate(q[None, :], [int(rng.integers(0, 12))], 1000 + t)[0]
            s = np.concatenate([s, acgt[rng.integers(0, 4, max(0, n - s.size))]])[:n]
        pairs.append((q, s))
    assert sum(q.size != s.size for q, s in pairs) > 100
    q = acgt[rng.integers(0, 4, 90)]
    pairs += [(b"A" * 70, b"A" * 70), (b"A" * 70, b"A" * 50), (b"A" * 20, b"A" * 33),         # every cell a tie
              (q, np.concatenate([acgt[[1]], q[:-1]])), (q, np.concatenate([acgt[rng.integers(0, 4, 33)], q])[:90]),   # shifted copies
              (b"A" * 64, b"C" * 64), (b"A" * 40, b"C" * 65)]                                   # all mismatch
    _check_pairs(oracle, pairs)


def test_reference_tie_breaks_are_the_contracts():
    def script(q, s):
        (d, runs), = A.canonical(np.frombuffer(q, np.uint8)[None, :], np.frombuffer(s, np.uint8)[None, :])
        return d, A.to_string(runs)
    assert script(b"AAAA", b"AAAA") == (0, "4=")
    assert script(b"AAAA", b"AA") == (2, "2I2=")          # walking back: the diagonal first, so the gap lands at the front
    assert script(b"AA", b"AAAA") == (2, "2D2=")
    assert script(b"ACGT", b"TGCA") == (4, "4X")
    assert script(b"ACGT", b"CGT") == (1, "1I3=")
    assert script(b"AC", b"CA") == (2, "2X")                # a mismatch diagonal is preferred to I + D of the same cost
    assert script(b"ANNA", b"ANxA") == (1, "2=1X1=")        # 'N' is a class of its own; a foreign byte is class 0 = 'A'
    assert script(b"AxA", b"AAA") == (0, "3=")


def test_reference_classes_are_the_librarys_mapping_table(L):
    L.init_mapping_table()
    table = (ctypes.c_uint32 * 128).in_dll(L, "mapping_table")
    assert A.class_table()[:128].tolist() == list(table) and not A.class_table()[128:].any()


# ---- the C ABI, before any HIP call ---------------------------------------------------------------------------------
def _call(L, content=P, peq=P, ref_len=150, read_len=150, read_count=640, word_num=5, pq=P, ps=P, n_pairs=100, n_queries=10,
          base=0, dist=P, n_ops=P, cigar=P, cap=300, ws=None, ws_bytes=0):
    return L.bgsa_hip_myers_align_pairs_dev(content, peq, ref_len, read_len, read_count, word_num, pq, ps, n_pairs, n_queries, base,
                                            dist, n_ops, cigar, cap, ws, ws_bytes, None)


def test_symbols_are_declared_and_exported(L):
    names = B.declared_symbols()
    for fn in ("bgsa_hip_align_pairs_workspace_bytes", "bgsa_hip_align_pairs_min_workspace_bytes", "bgsa_hip_myers_align_pairs_dev"):
        assert fn in names and hasattr(L, fn)
    header = B.INCLUDE.read_text()
    assert "#define BGSA_HIP_FAULT_PAIR 4" in header and "BGSA_HIP_ALIGN_PAIRS_MAX_WORKSPACE ((size_t)1 << 30)" in header


def test_argument_checks_come_before_any_hip_call(L):
    for name in ("content", "peq", "pq", "ps", "dist", "n_ops", "cigar"):
        assert _call(L, **{name: None}) == EINVAL, name
    assert b"NULL" in L.bgsa_hip_last_error()
    assert _call(L, n_pairs=-1) == EINVAL
    assert _call(L, ref_len=0) == EINVAL and _call(L, ref_len=-7) == EINVAL
    assert _call(L, read_len=0, word_num=0) == EINVAL and _call(L, read_len=-1, word_num=0) == EINVAL
    assert _call(L, n_queries=0) == EINVAL and _call(L, n_queries=-2) == EINVAL
    assert _call(L, cap=0) == EINVAL and _call(L, cap=-1) == EINVAL
    for rc in (0, -64, 1, 63, 65, 100):
        assert _call(L, read_count=rc) == EINVAL, rc
    assert b"multiple of 64" in L.bgsa_hip_last_error()
    for wn in (0, 4, 6, 32):
        assert _call(L, word_num=wn) == EINVAL, wn
    assert _call(L, read_len=128, word_num=5) == EINVAL and _call(L, read_len=161, word_num=5) == EINVAL
    need = L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150)
    assert _call(L, ws=P, ws_bytes=need - 1) == EINVAL and _call(L, ws=P, ws_bytes=0) == EINVAL
    assert b"workspace" in L.bgsa_hip_last_error()
    # the errors also win over an empty list
    assert _call(L, n_pairs=0, peq=None) == EINVAL and _call(L, n_pairs=0, word_num=4) == EINVAL


def test_subjects_beyond_1024_bp_are_unsupported(L):
    for read_len in (1025, 1056, 4000):
        wn = L.bgsa_hip_word_num(B.ALGO_MYERS, 150, read_len, 0)
        assert wn > 32 and _call(L, read_len=read_len, word_num=wn) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()
    assert _call(L, read_len=1025, word_num=32) == EINVAL          # a word_num that is not the layout's comes first
    assert _call(L, read_len=1024, word_num=32, n_pairs=0) == 0    # the widest covered subject passes the checks


def test_an_empty_pair_list_is_ok_and_launches_nothing(L):
    assert _call(L, n_pairs=0) == 0
    need = L.bgsa_hip_align_pairs_min_workspace_bytes(150, 150)
    assert _call(L, n_pairs=0, ws=P, ws_bytes=need) == 0            # every pointer is fake: nothing may look at them


def test_workspace_bytes_are_monotone_between_the_minimum_and_the_cap(L):
    f, fmin = L.bgsa_hip_align_pairs_workspace_bytes, L.bgsa_hip_align_pairs_min_workspace_bytes
    cap = 1 << 30
    assert f(0, 150, 10) == 0 and f(150, 0, 10) == 0 and f(150, 150, -1) == 0 and fmin(0, 150) == 0 and fmin(150, -1) == 0
    lens = [1, 2, 31, 32, 33, 64, 65, 150, 151, 1000, 1023, 1024]
    pairs = [0, 1, 63, 64, 65, 200, 10_000, 100_000, 1_000_000, 1 << 40]
    table = np.array([[[f(m, n, k) for k in pairs] for n in lens] for m in lens], dtype=np.float64)
    mins = np.array([[fmin(m, n) for n in lens] for m in lens], dtype=np.float64)
    assert (mins > 0).all() and (mins % 256 == 0).all()
    assert (np.diff(mins, axis=0) >= 0).all() and (np.diff(mins, axis=1) >= 0).all()
    for axis in range(3):
        assert (np.diff(table, axis=axis) >= 0).all(), axis
    assert (table >= mins[:, :, None]).all() and (table <= cap).all()
    assert (table[:, :, :3] == mins[:, :, None]).all()              # up to 64 pairs: one wave
    assert (table[:, :, -1] == cap).all()                           # 2^40 pairs: the cap, for every shape here
    # the history is two vectors per row and word: 8 * word_num bytes per row and pair, plus one op byte per step
    assert fmin(150, 150) == 64 * (150 * 8 * 5 + 300) and f(150, 150, 100_000) == 1563 * fmin(150, 150)
    assert fmin(1000, 1000) == 64 * (1000 * 8 * 32 + 2000)
    assert f(1000, 1000, 10_000) == cap                             # 2.6 GB in one pass: the call walks it in chunks
    # a query so long that 64 pairs alone pass the cap: the minimum still holds
    assert f(1 << 20, 1024, 1) == fmin(1 << 20, 1024) > cap

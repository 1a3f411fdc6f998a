"""The verify census (tests/verify_census.py) proves its own completeness on the host: every instance of
reference_verify_pairs_kernel the dispatch of either library flavour can name is reached by a census word count — at word_num ==
WB, at every word count below WB that the ladder leaves to it, the column blocks at every tail of 1 .. 16 words —, the window
lengths leave every size of the last block of rows, and the census inputs are worth launching: the DP alone finds planted reads
on both strands and unrelated ones.  No GPU: names, word counts and refusals are host logic, the conditions are the oracle's."""
import ctypes
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import verify_census as C  # noqa: E402

FLAVOURS = ["libbgsa_hip.so", "libbgsa_hip_ab.so"]
EUNSUPPORTED = -2

# The ladder of dispatch_verify as it stands: {WB: the word counts it serves}, then column blocks of 16 words.  A width added
# to the ladder changes this table; whoever updates it sees below whether the census reaches the new instance.
LADDER = {1: [1], 2: [2], 3: [3], 4: [4], 5: [5], 6: [6], 8: [7, 8], 12: [9, 10, 11, 12], 16: [13, 14, 15, 16]}
BLOCK_WORDS = 16


@pytest.fixture(scope="module")
def L():
    if not B.LIB_PATH.exists() or not B.LIB_AB_PATH.exists():
        B.build_library()
    return B.lib()


def flavour_names(flavour, lens):
    lib = ctypes.CDLL(str(B.HERE / flavour))
    lib.bgsa_hip_reference_verify_kernel_name.restype = ctypes.c_char_p
    return C.kernel_names(lib, lens)


def served(names):
    """{name: the word counts of 1 .. 130 it is named for}."""
    out = {}
    for w, name in enumerate(names, start=1):
        out.setdefault(name, []).append(w)
    return out


# ---- names ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [False, True])
@pytest.mark.parametrize("flavour", FLAVOURS)
def test_every_verify_instance_is_reached_by_a_census_word_count(L, flavour, lens):
    names = flavour_names(flavour, lens)
    assert len(names) == C.NAME_WORDS and all(n.endswith(", true>" if lens else ", false>") for n in names)
    reached = {names[w - 1] for w in C.WORDS}
    assert set(names) == reached, f"no census word count reaches {sorted(set(names) - reached)}"
    blocked = 0
    for name, words in served(names).items():
        wb = C.name_width(name)
        if C.name_blocks(name):
            blocked += 1
            census = [w for w in C.WORDS if w in words]
            assert words == list(range(wb + 1, C.NAME_WORDS + 1))                    # one block width behind the whole ladder
            assert {(w - 1) % wb + 1 for w in census if -(-w // wb) == 2} == set(range(1, wb + 1)), "a tail of the second block is missing"
            assert any(-(-w // wb) == 3 for w in census), "no census word count has a third block"
        else:
            assert max(words) == wb and wb in C.WORDS, name                          # reached at word_num == WB ...
            assert set(words) <= set(C.WORDS), name                                  # ... and at every word count below it
    assert blocked == 1


@pytest.mark.parametrize("lens", [False, True])
def test_the_ladder_is_the_one_the_census_was_written_for(L, lens):
    names = C.kernel_names(L, lens)
    tail = "true" if lens else "false"
    want = {f"reference_verify_pairs_kernel<{wb}, false, {tail}>": words for wb, words in LADDER.items()}
    want[f"reference_verify_pairs_kernel<{BLOCK_WORDS}, true, {tail}>"] = list(range(BLOCK_WORDS + 1, C.NAME_WORDS + 1))
    assert served(names) == want
    partial = sorted(w for words in LADDER.values() for w in words[:-1])
    assert partial == [7, 9, 10, 11, 13, 14, 15] and set(partial) <= set(C.WORDS)      # word_num < WB: the `w < wb` guard is live


def test_what_the_calls_launch_and_what_they_refuse(L):
    """Word counts 1 .. 32 pass the checks of both calls.  33 — the census's third column block — is named by the dispatch and
    refused by the calls (BGSA_HIP_EUNSUPPORTED, include/bgsa_hip.h): no call can launch three blocks, and the GPU file asserts
    the refusal there.  Raising the limit makes this test fail, and the GPU file then launches the case."""
    assert [w for w in C.WORDS if C.accepted(L, w)] == list(range(1, 33))
    n = 32 * 33
    assert L.bgsa_hip_reference_verify_pairs_dev(C.P, 5000, n + 40, C.STRIDE, C.P, n, 64, 33, C.P, C.P, 0, 0, C.P, C.P, 1 << 40, None) == EUNSUPPORTED
    assert b"1,024" in L.bgsa_hip_last_error()


# ---- shapes ---------------------------------------------------------------------------------------------------------------------
def test_the_shapes_of_the_census(L):
    cases = C.cases()
    assert len(cases) == 2 * (2 * len(C.WORDS) + 1) == 134 and len(set(cases)) == len(cases)
    for w, n, lens in cases:
        m = C.window_len(w, n)
        assert B.word_num(B.ALGO_MYERS, m, n) == w and n + 33 <= m <= n + 64
        assert C.M.window_count(C.ref_len(m), m, C.STRIDE) == C.N_WINDOWS
        assert C.M.window_start(C.ref_len(m), m, C.STRIDE, C.N_WINDOWS - 1) % C.STRIDE == 1
        assert (L.bgsa_hip_reference_verify_workspace_bytes(m, n, 707) > 0) == (w > 16)
        assert (L.bgsa_hip_reference_verify_workspace_bytes(m, n, 0) > 0) == (w > 16)
    for w in C.WORDS:
        assert [n for n in C.read_lengths(w) if n > 1] == [32 * w - 5, 32 * w]
    assert C.read_lengths(1)[0] == 1


@pytest.mark.parametrize("lens", [False, True])
def test_every_size_of_the_last_block_of_rows(L, lens):
    names = C.kernel_names(L, lens)
    launched = [w for w in C.WORDS if C.accepted(L, w)]
    for family in (-2, -1):                                    # the partial and the full last word, each over all word counts
        assert {C.window_len(w, C.read_lengths(w)[family]) % 32 for w in launched} == set(range(32))
    for blocks in (False, True):                               # the one-block instances together, and the column blocks
        words = [w for w in launched if C.name_blocks(names[w - 1]) == blocks]
        assert {C.window_len(w, n) % 32 for w in words for n in C.read_lengths(w)} == set(range(32)), blocks


@pytest.mark.parametrize("w", C.WORDS)
def test_lens_lengths(w):
    for n in C.read_lengths(w):
        lens = C.lens_lengths(w, n)
        assert len(lens) == C.N_READS and max(lens) == n and min(lens) >= 1
        assert {x for x in C.required_lengths(w) if x <= n} <= set(lens)
        assert {C.own_block(x) for x in lens} == set(range((w + 15) // 16))
    if w > 16:
        assert {512, 513} <= set(C.required_lengths(w)) and C.own_block(512) == 0 and C.own_block(513) == 1
        assert {C.own_block(x) for x in C.required_lengths(w) if x not in (512, 513)} >= set(range((w + 15) // 16))


# ---- the DP alone on the inputs: the three smallest and the three largest word counts (the GPU file asserts the same of every case)
@pytest.mark.parametrize("w", C.WORDS[:3] + C.WORDS[-3:])
def test_census_inputs_are_worth_launching(oracle, w):
    for n in C.read_lengths(w):
        for lens in (False, True):
            c = C.case(w, n, lens)
            assert len(c["reads"]) == C.N_READS and [r.size for r in c["reads"]] == c["lengths"]
            assert c["windows"].size == 707 == c["subjects"].size and c["owned"].sum() == 700
            C.assert_worth_launching(c, w, n, lens)

"""The BGZF deflate stage without a GPU: the host model of tests/deflate_reference.py against zlib — every block inflates to its
payload, the dynamic form is chosen exactly where it is shorter, the code lengths are limited to 15 and complete, matching
contributes — and the three C symbols' refusals through ctypes with fake pointers."""
import ctypes
import heapq
import sys
import zlib
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import bgsa_amd as B  # noqa: E402
import bam_reference as M  # noqa: E402
import deflate_reference as D  # noqa: E402

NAMES = sorted(D.payloads())


# ---- 0. the model's own arithmetic ----------------------------------------------------------------------------------------------------------
def test_symbol_arithmetic_equals_the_tables_of_rfc_1951():
    for length in range(3, 259):
        symbol, extra, value = D.length_symbol(length)
        assert D.LENGTH_BASE[symbol - 257] + value == length and D.LENGTH_EXTRA[symbol - 257] == extra == D.litlen_extra(symbol), length
        assert value < 1 << extra
    for dist in range(1, 32769):
        symbol, extra, value = D.dist_symbol(dist)
        assert D.DIST_BASE[symbol] + value == dist and D.DIST_EXTRA[symbol] == extra == D.dist_extra(symbol) and value < 1 << extra, dist


def test_the_payloads_hold_what_they_are_for():
    P = D.payloads()
    tokens = {name: D.parse(P[name][:D.FULL]) for name in NAMES if not name.startswith("bam_")}
    dists = {name: {d for _, n, d in toks if n} for name, toks in tokens.items()}
    lengths = {name: [n for _, n, _ in toks if n] for name, toks in tokens.items()}
    assert lengths["zeros"] == [258] * 253 + [5] and dists["zeros"] == {1}                      # 1 + 253 * 258 + 5 = 65,280
    assert len(D.de_bruijn(16, 3)) == 4096 and not lengths["debruijn"] and len(set(P["debruijn"])) == 16
    grams = [P["debruijn"][i: i + 3] for i in range(4094)]
    assert len(set(grams)) == len(grams)
    # the table keeps the greatest position per hash, so a later position of another 4-gram may have taken the entry of the repeat's
    # first bytes: the repeat is then picked up a few bytes in, and found it is
    assert any(d == 32768 and n >= 32 and 32868 <= p < 32900 for p, n, d in tokens["dist32768"])
    assert not any(n >= 32 for _, n, _ in tokens["dist32769"]) and max(dists["dist32769"]) <= 32768
    assert (3000, 258, 2500) in tokens["avail258"] and (3000, 258, 2500) in tokens["avail259"]
    # 2 or 3 equal bytes with another 4th byte hash differently: the table does not offer them (a length 3 comes from runs only)
    assert all(p != 3000 for p, n, _ in tokens["avail2"] if n) and all(p != 3000 for p, n, _ in tokens["avail3"] if n)
    assert D.parse(b"abbbbc")[:3] == [(0, 0, 0), (1, 0, 0), (2, 3, 1)] and D.parse(b"abbbc")[2] == (2, 0, 0)
    assert tokens["avail259"][[p for p, _, _ in tokens["avail259"]].index(3000) + 1][0] == 3258      # the rest: the next token
    assert (2960, 40, 2760) == tokens["ends_on_last"][-1]                                        # ends on the block's last byte
    assert (1500, 32, 600) in tokens["previous_tile"] and all(p != 1500 for p, n, _ in tokens["same_tile"] if n)
    whole = D.parse(P["boundary"])
    assert any(n and p >= 4096 and d == 4096 for p, n, d in whole)                               # one block of 8,192: the halves match
    for block in D.modelled("boundary", 4096):                                                  # two blocks: they cannot
        assert D.is_dynamic(block)
    assert D.modelled("boundary", 4096)[0][18:-8] == D.modelled("boundary", 4096)[1][18:-8]


# ---- 1. and 2. every block inflates; the form is the shorter one --------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_the_models_blocks_inflate_to_the_payload_and_take_the_shorter_form(name):
    data = D.payloads()[name]
    for P in D.BLOCK_PAYLOADS:
        blocks = D.modelled(name, P)
        assert len(blocks) == -(-len(data) // P)
        pieces = M.walk_blocks(b"".join(blocks), stored=False)
        assert b"".join(pieces) == data, (name, P)
        assert all(len(x) == P for x in pieces[:-1]) and 1 <= len(pieces[-1]) <= P
        if P in (1, 61):
            assert not any(D.is_dynamic(b) for b in blocks) and b"".join(blocks) == M.frame(data, P)      # stored: today's bytes
            continue
        for piece, block in zip(pieces, blocks):
            assert len(block) <= len(piece) + 31
            dynamic = D._dynamic_once(piece)
            assert zlib.decompress(dynamic, -15) == piece
            assert D.is_dynamic(block) == (len(dynamic) < len(piece) + 5), (name, P, len(dynamic), len(piece))
            assert block[18:-8] == (dynamic if D.is_dynamic(block) else D.stored_block(piece))


def test_short_and_random_blocks_come_out_stored_and_the_rest_dynamic():
    stored = {name for name in NAMES if not any(D.is_dynamic(b) for b in D.modelled(name, D.FULL))}
    assert stored == {"same1", "same2", "same3", "same4", "random"}
    for regime in ("constant", "binned", "uniform"):                     # one full block, then a tail of 61 bytes
        first, tail = D.modelled(f"bam_{regime}", D.FULL)
        assert D.is_dynamic(first) and not D.is_dynamic(tail) and len(tail) == 61 + 31
    assert D.deflate_block(b"") == D.stored_block(b"")
    # without a match the distance code is empty: all 30 lengths 0, and zlib takes it
    lengths = D.code_lengths(D.histograms(D.payloads()["debruijn"], D.parse(D.payloads()["debruijn"]))[1])
    assert lengths == [0] * 30 and D.is_dynamic(D.modelled("debruijn", D.FULL)[0])
    # one used distance symbol: length 1
    assert D.code_lengths(D.histograms(bytes(D.FULL), D.parse(bytes(D.FULL)))[1]) == [1] + [0] * 29


# ---- 3. length limiting ----------------------------------------------------------------------------------------------------------------------
def kraft(lengths) -> Fraction:
    return sum(Fraction(1, 2 ** n) for n in lengths if n)


def tallest_huffman_depth(counts) -> int:
    """The depth of a Huffman tree of the counts, by the textbook heap, with every tie between equal weights going to the taller
    subtree: among the optimal trees a tall one."""
    heap = [(c, 0) for c in counts]
    heapq.heapify(heap)
    while len(heap) > 1:
        (a, x), (b, y) = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a + b, -(max(-x, -y) + 1)))
    return -heap[0][1]


def test_code_lengths_are_limited_to_15_and_complete():
    """Literal counts 1, 1, 2, 3, 5, ... over 20 symbols, 17,710 shuffled bytes.  The model's own parse finds matches in any order
    of these bytes (deflate_reference.fibonacci_literals says why), so the block is coded here as literals alone — the counts are
    then exactly the sequence — through the model's code construction and bit writer.  Every merge of this sequence is a tie, and
    an unlimited Huffman code of it is as deep as the ties are broken: the textbook heap with ties to the taller subtree gives 20,
    Moffat and Katajainen's rule, which the model and the kernel use, prefers the leaf and gives 11.  So the limit is shown to bind
    on deep_literals(), whose counts have no ties at the bottom: 17 deep by the model's own rule."""
    data = D.fibonacci_literals()
    assert len(data) == 17710
    literals = [(p, 0, 0) for p in range(len(data))]
    litlen, dist = D.histograms(data, literals)
    assert sorted(c for c in litlen[:256] if c) == [1, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987, 1597, 2584, 4181, 6765]
    assert tallest_huffman_depth([c for c in litlen if c]) == 20 > 15             # an unlimited code of them is deeper than deflate allows
    lengths = D.code_lengths(litlen)
    assert max(lengths) == max(D.huffman_depths(sorted(c for c in litlen if c))) == 11
    assert max(lengths) <= 15 and kraft(lengths) == 1 and [n > 0 for n in lengths] == [c > 0 for c in litlen]
    assert D.code_lengths(dist) == [0] * 30
    assert zlib.decompress(D.dynamic_block(data, literals), -15) == data
    assert zlib.decompress(D.dynamic_block(data), -15) == data                  # and under the model's own parse
    # the payload that needs the limit under the model's own parse: no match, 31 counts, 17 deep
    data = D.payloads()["deep_code"]
    tokens = D.parse(data)
    assert len(tokens) == len(data) == 13979 and not any(n for _, n, _ in tokens)
    litlen, dist = D.histograms(data, tokens)
    assert max(D.huffman_depths(sorted(c for c in litlen if c))) == 17 > 15
    lengths = D.code_lengths(litlen)
    assert max(lengths) == 15 and kraft(lengths) == 1 and [n > 0 for n in lengths] == [c > 0 for c in litlen]
    block = D.dynamic_block(data)
    assert zlib.decompress(block, -15) == data and D.deflate_block(data) == block
    # the counts alone: 1, 1, 2, 3, 5, ... over 24 symbols
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    assert max(D.huffman_depths(fib)) == 23
    lengths = D.code_lengths(fib + [0] * 262)
    assert max(lengths) == 15 and kraft(lengths) == 1
    assert lengths[23] == 1 and lengths[0] == 15                                 # the shortest code to the greatest count


# ---- 4. the compressor does something ---------------------------------------------------------------------------------------------------------
def huffman_only(data: bytes) -> int:
    z = zlib.compressobj(6, zlib.DEFLATED, -15, 8, zlib.Z_HUFFMAN_ONLY)
    return len(z.compress(data) + z.flush())


def test_equal_bytes_come_out_under_512_bytes():
    block, = D.modelled("zeros", D.FULL)
    assert D.is_dynamic(block) and len(block) < 512


@pytest.mark.parametrize("regime", ("constant", "binned", "uniform"))
def test_matching_beats_zlibs_huffman_only_deflate_on_bam_like_blocks(regime):
    """Measured with this model (bytes of deflate data per block of 65,280; the margin to Z_HUFFMAN_ONLY):
    constant 12,482 against 27,647 (55 %), binned 21,835 against 35,837 (39 %), uniform 38,347 against 47,660 (20 %)."""
    data = D.payloads()[f"bam_{regime}"][:D.FULL]
    ours = len(D.modelled(f"bam_{regime}", D.FULL)[0]) - 26
    print(regime, ours, huffman_only(data))
    assert ours < huffman_only(data)


# ---- 5. the C symbols -------------------------------------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_and_exported():
    L = B.lib()
    for name in ("bgsa_hip_bgzf_deflate_workspace_bytes", "bgsa_hip_bgzf_deflate_dev", "bgsa_hip_bgzf_pack_dev"):
        assert name in B.declared_symbols() and hasattr(L, name)
    assert L.bgsa_hip_bgzf_deflate_workspace_bytes.restype is ctypes.c_int64


def test_workspace_bytes_is_monotone_and_refuses_bad_arguments():
    L = B.lib()
    room = L.bgsa_hip_bgzf_deflate_workspace_bytes
    assert room(0, 65280) == 0
    for bad in ((-1, 256), (2 ** 62, 256), (100, 0), (100, 65281), (100, -5)):
        assert room(*bad) == -1
    sizes = (0, 1, 163, 164, 65279, 65280, 65281, 10 ** 9, 2 ** 58 - 1)
    for P in (1, 61, 256, 65280):
        got = [room(n, P) for n in sizes]
        assert all(x >= 0 for x in got) and got == sorted(got)
    for n in sizes:
        got = [room(n, P) for P in (1, 2, 61, 256, 4096, 65280)]
        assert got == sorted(got)


def test_deflate_and_pack_refuse_bad_arguments_before_any_launch():
    L = B.lib()
    fake = 0x1000                                           # never dereferenced: every call here is refused on the host
    P, n = 256, 1000
    blocks = 4
    slots, room = blocks * (P + 31), L.bgsa_hip_bgzf_deflate_workspace_bytes(n, P)
    good = [fake, n, P, fake, slots, fake, fake, room, None]
    for at, value, why in ((0, None, b"NULL"), (3, None, b"NULL"), (5, None, b"NULL"), (6, None, b"NULL"), (2, 0, b"block_payload"),
                           (2, 65281, b"block_payload"), (1, -1, b"payload_bytes"), (1, 2 ** 62, b"payload_bytes"), (4, slots - 1, b"slots_bytes"),
                           (4, slots + 1, b"slots_bytes"), (4, n + 31 * blocks, b"slots_bytes"), (7, room - 1, b"workspace_bytes"),
                           (7, 0, b"workspace_bytes"), (6, fake + 2, b"aligned")):
        args = list(good)
        args[at] = value
        assert L.bgsa_hip_bgzf_deflate_dev(*args) == -1 and why in L.bgsa_hip_last_error(), (at, value, L.bgsa_hip_last_error())
    assert L.bgsa_hip_bgzf_deflate_dev(fake, 0, P, fake, 0, fake, fake, 0, None) == 0           # an empty payload: no block, nothing launched
    good = [fake, P, blocks, fake, fake, 1000, fake, None]
    for at, value, why in ((0, None, b"NULL"), (3, None, b"NULL"), (4, None, b"NULL"), (6, None, b"NULL"), (1, 0, b"block_payload"),
                           (1, 65281, b"block_payload"), (2, -1, b"n_blocks"), (2, 2 ** 31, b"n_blocks"), (5, -1, b"out_bytes")):
        args = list(good)
        args[at] = value
        assert L.bgsa_hip_bgzf_pack_dev(*args) == -1 and why in L.bgsa_hip_last_error(), (at, value, L.bgsa_hip_last_error())
    assert L.bgsa_hip_bgzf_pack_dev(fake, P, 0, fake, fake, 0, fake, None) == 0


def test_check_bam_call_refuses_a_compress_that_is_no_bool():
    lens = np.full(2, 10, dtype=np.int32)
    for good in (True, False):
        assert len(B.check_bam_call("t", lens, None, None, "ref", 256, good)) == 4
    for bad in (1, 0, "yes", None):
        with pytest.raises(B.BgsaHipError, match="compress"):
            B.check_bam_call("t", lens, None, None, "ref", 256, bad)
    import inspect
    for cls in (B.ReferenceMapper, B.ContigMapper):
        assert inspect.signature(B.ReferenceMapper.map_reads_bam).parameters["compress"].default is False
        assert inspect.signature(B.ReferenceMapper.map_pairs_bam).parameters["compress"].default is False
        assert hasattr(cls, "bgzf_deflated")

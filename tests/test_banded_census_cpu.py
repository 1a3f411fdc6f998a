"""The banded census on the host (tests/banded_census.py): what tests/test_banded_census_gpu.py launches stands where it claims to.

Per threshold k = 1 .. 31, over every census launch (computed once per k, shared by the tests below):
  * the plain band DP equals oracle.banded64 exactly, on every census shape and input.  (banded64, the literal restatement of the
    reference, stays normative: were they ever to differ the DP's domain would be narrowed here, with the reason.)
  * rows_ir.banded_simulate equals both, in the form the threshold runs by default: cut = banded_cut_rows(k) with two groups for
    k <= 12, the sliding forms otherwise.
  * the census lengths reach every event-placement class that any length up to 1,100 reaches.
  * the route model (banded_census.routes: the DP's error on the lowest diagonal at the stream's test rows, under the launcher's
    push_row, push_row_solid, solid_limit and push_max) shows: no push under first_pass; under dense_pass a push in every shape
    that has a test before `last`; under static each of the three routes (stopped dead, pushed, run to the end); under every
    configuration with a queue a push that finds exactly push_max lanes alive and a test that finds push_max + 1 and goes on; under
    dense_pass a (wave, tile) whose list passes 64 - push_max and is flushed in the middle of the tile.
    With push_max = 8 a list passes 56 only after eight pushes of eight lanes in front of a ninth query of the tile: a tile of
    16, which pick_query_tile gives a launch this small where 8 x length x groups per wave < 512.  With two groups per wave
    (k <= 15) that is len < 32, below push_row_solid = k + 32: for those forms the flush is dense_pass's alone.  With one group
    per wave it is every length below 64, and at k = 16 .. 24 a test at or after row k + 32 lies before last = len there: the
    flush launches of the census (16 near-duplicate queries) fill the list exactly, 64 pairs, in the middle of a tile under
    static and counter (test_flush_launches_fill_the_list_inside_a_tile).
  * check values D[last][last - k - 1] of exactly 2k + 1 (accepted) and exactly 2k + 2 (rejected), and both outcomes in every launch.
    The values are the DP's rows; on every pair oracle.banded64 answers 127 if and only if that value is above 2k + 1, so a row
    that were wrong at `last` with a right score would show.  (The rows at the earlier tests feed the route model only; the
    oracle has no output that would pin them.)
  * bgsa_hip_query_stream (banded) equals rows_ir.banded_stream_bytes byte for byte at every census (length, k).
"""
import functools
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import banded_census as C  # noqa: E402

R, O, B = C.R, C.O, C.B
K = list(C.THRESHOLDS)


@functools.lru_cache(maxsize=None)
def survey(k):
    """One pass over the census launches of threshold k."""
    out = {"differ": [], "simulator": [], "checks": set(), "one_outcome": [], "routes": {c: [] for c in C.CONFIGS},
           "twin": [], "pairs": 0, "closed_form": [], "check_rows": []}
    for length in C.lengths(k):
        q, s, foreign = C.launch(k, length)
        want, low = C.band_dp(q, s, k, rows=True)
        ref = O.banded64(q, s, k)
        out["pairs"] += want.size
        if not np.array_equal(want, ref):
            out["differ"].append((length, int((want != ref).sum())))
        if not np.array_equal(O.dp_banded(q, s, k), ref):      # the oracle's closed form: the same DP, cell by cell in C
            out["closed_form"].append(length)
        cut = R.banded_cut_rows(k)
        # query 1 is query 0 with 'A' at three positions and row 2 is row 1 again: the simulator, which costs more than everything
        # else here together, takes queries 0 and 3 at every shape and query 1 at every fourth
        for qi in ((0, 1, 3) if C.lengths(k).index(length) % 4 == 0 else (0, 3)):
            sim = R.banded_simulate(s, q[qi], k, cut=cut, groups=2 if cut else 1)
            if not np.array_equal(sim, ref[qi]):
                out["simulator"].append((length, qi))
        if not np.array_equal(q[2], q[1]) or len(foreign) != C.N_FOREIGN or any(q[2, p] != ord("A") or b <= 4 for p, b in foreign):
            out["twin"].append(length)
        last = R.banded_last_check(length, k)
        out["checks"] |= set(np.unique(low[..., last]).tolist())
        if not np.array_equal(ref == 127, low[..., last] > 2 * k + 1):
            out["check_rows"].append(length)
        if not ((want == 127).any() and (want != 127).any()):
            out["one_outcome"].append(length)
        # a read over {G, T} against the query over {A, C}: an error in every row, rejected at every length
        gt = np.isin(s, list(b"GT")).all(axis=1)
        assert gt.sum() >= 8 and (want[3, gt] == 127).all() and np.isin(q[3], list(b"AC")).all(), (k, length)
        for config in C.CONFIGS:
            out["routes"][config].append((length,) + C.routes(k, length, config, low))
    return out


@pytest.mark.parametrize("k", K)
def test_plain_dp_equals_banded64_on_every_census_input(k):
    r = survey(k)
    classes = set().union(*(C.stream_classes(n, k) for n in C.lengths(k)))
    print(f"k = {k}: {len(C.lengths(k))} lengths {C.lengths(k)[0]} .. {C.lengths(k)[-1]}, {len(classes)} classes, {r['pairs']} pairs")
    assert not r["differ"], f"(length, pairs that differ) = {r['differ'][:5]}"
    assert not r["closed_form"], f"oracle.dp_banded differs from oracle.banded64 at lengths {r['closed_form'][:5]}"
    assert not r["twin"]


@pytest.mark.parametrize("k", K)
def test_row_simulator_equals_both_references(k):
    assert not survey(k)["simulator"], f"(length, query) = {survey(k)['simulator'][:5]}"


@pytest.mark.parametrize("k", K)
def test_census_lengths_reach_every_class_of_the_domain(k):
    have = set().union(*(C.stream_classes(n, k) for n in C.lengths(k)))
    want = set().union(*(C.stream_classes(n, k) for n in C.domain(k)))
    assert want == have, sorted(want - have, key=str)
    assert C.domain(k)[0] == 2 * k + 2 and C.domain(k)[-1] == 1100 and set(C.sketch_lengths(k)) <= set(C.lengths(k))
    assert set(C.period_block(k)) <= set(C.lengths(k)) and C.period_block(k)[0] > max(64 + k, k + 48 + 16)
    # what the census is known to reach, so that a classification that lost its grain cannot make it look complete: the merged
    # bytes of the last checkpoint (14: advance, test and latch, on a 32-row word edge; 44: cut, test and latch), all three
    # regimes of `last`, an early window close, both kinds of length
    f = C.form(k)
    events = {(x[1], x[2]) for x in have if x[0] == f}
    bits = {b for b, _ in events}
    assert {12, 14} <= bits and any(b & 1 for b in bits) and any(b & 2 for b in bits), sorted(events)
    assert any(b & 12 == 4 for b in bits)      # a test that does not latch (cut every 8 rows: always merged with a cut or an advance)
    assert (44 in bits) == (k <= 12) and any(b & 32 for b in bits) == (k <= 12)
    assert any(early for _, early in events)
    regimes = {x[3] for x in have if x[0] == f}
    assert regimes == {"len <= 64", "last = 64", "last = len - k"}
    for reg in ("last = 64", "last = len - k"):      # the last checkpoint on a 32-row word edge (with len <= 64 no row follows it)
        assert any(x[:2] == (f, 14) and x[3] == reg for x in have), (k, reg)
    assert {x[4] for x in have if x[0] == f} == {False, True}


@pytest.mark.parametrize("k", K)
def test_routes_of_the_census_launches(k):
    r = survey(k)
    per = {}
    for config in C.CONFIGS:
        push_max = C.push_knobs(config, k)[3]
        kinds, exact, above, flushed, no_push = set(), 0, 0, 0, []
        for length, routes, seen, flush in r["routes"][config]:
            kinds |= {x[0] for x in routes.values()}
            pushes = [x for x in routes.values() if x[0] == "push"]
            exact += sum(1 for x in pushes if x[2] == push_max)
            above += sum(1 for counts in seen.values() for _, n in counts if n == push_max + 1)
            flushed += len(flush)
            last = R.banded_last_check(length, k)
            if not pushes and any(row < last for row, _ in C.test_rows(length, k)):
                no_push.append(length)
            assert all(1 <= x[2] <= push_max and x[3] <= x[2] for x in pushes)
        per[config] = (kinds, exact, above, flushed, no_push)
    print(f"k = {k}: " + "; ".join(f"{c}: routes {sorted(v[0])}, pushes at push_max {v[1]}, tests at push_max + 1 {v[2]}, "
                                     f"flushes inside a tile {v[3]}" for c, v in per.items()))
    assert "push" not in per["first_pass"][0] and per["first_pass"][3] == 0
    assert not per["dense_pass"][4], f"dense_pass: no push at lengths {per['dense_pass'][4]}"
    assert per["static"][0] == {"dead", "push", "end"}
    assert per["counter"] == per["static"]
    for config in ("static", "counter", "dense_pass"):
        assert per[config][1] >= 1 and per[config][2] >= 1, (config, per[config][1:3])
    assert per["dense_pass"][3] >= 1


def test_the_model_counts_both_groups_and_a_lone_group_twice():
    """Two things the route model must reproduce (banded.hip: banded_cut_kernel; gen_rows_asm.py: push_or): the alive counts of both
    groups of a wave are added before they meet push_max, and a wave without a second group runs the first one twice."""
    k, length = 8, 150
    low = np.full((128, length + 1), 100, np.int32)      # every lane far past the limit ...
    low[:5] = k                                          # ... but five of group 0 and four of group 1
    low[64:68] = k
    assert C.route(low, k, length, "static")[0] == ("end",) and C.route(low, k, length, "static")[1][0] == (40, 9)
    low[4] = 100
    assert C.route(low, k, length, "static")[0] == ("push", 40, 8, 8)
    assert C.route(low[:64], k, length, "static")[0] == ("push", 40, 8, 4)       # the wave's only group, counted twice
    low16 = np.full((64, length + 1), 100, np.int32)
    low16[:8] = 16
    assert C.route(low16, 16, length, "static")[0] == ("push", 48, 8, 8)         # one group per wave (k >= 16): counted once
    low[:] = 100
    assert C.route(low, k, length, "static")[0][0] == "dead"
    assert C.waves(8) == [(0, 2), (2, 1)] and C.waves(13) == [(0, 2), (2, 1)] and C.waves(16) == [(0, 1), (1, 1), (2, 1)]
    # the launcher's values: banded.hip: launch_rows
    assert C.push_knobs("static", 8) == (56, 40, 4, 8) and C.push_knobs("dense_pass", 8) == (8, 8, 9, 32)
    assert C.push_knobs("first_pass", 31)[3] == 0 and C.push_knobs("static", 31) == (79, 63, 16, 8)
    # pick_query_tile for launches this small: the smallest power of two that gives a task 512 row-words
    assert [C.query_tile(n, 8) for n in (18, 32, 64, 128, 150, 256)] == [16, 8, 4, 2, 2, 1]
    assert [C.query_tile(n, 16) for n in (34, 64, 128, 256, 512)] == [16, 8, 4, 2, 1]


@pytest.mark.parametrize("k", K)
def test_check_values_on_both_sides_of_the_limit(k):
    r = survey(k)
    assert {2 * k + 1, 2 * k + 2} <= r["checks"], sorted(x for x in r["checks"] if abs(x - 2 * k - 1) < 4)
    assert not r["one_outcome"]
    assert not r["check_rows"], f"oracle.banded64 rejects other pairs than the DP's row at `last` says, at lengths {r['check_rows'][:5]}"


@pytest.mark.parametrize("k,length", C.FLUSH_SHAPES)
def test_flush_launches_fill_the_list_inside_a_tile(k, length):
    """banded.hip: banded_cut_kernel flushes when n_regroup > 64 - push_max at the top of its query loop.  Under the default knobs:
    group 0's eight near-duplicates are pushed by every query, the list holds exactly 64 pairs in front of query 8 — every lane of
    the wave in banded_finish_pair<uint64_t>, s_regroup full — and 64 again at the tile's end; group 1's nine are one too many
    and run to the end; group 2's four make 56 pairs in front of query 14, which does not pass the bound, and 60 in front of query 15,
    which does."""
    q, s, foreign = C.flush_launch(k, length)
    assert q.shape == (C.FLUSH_NQ, length) and s.shape == (C.NS, length) and not foreign
    assert C.form(k) == "funnel64" and C.query_tile(length, k, C.FLUSH_NQ) == 16 and C.waves(k) == [(0, 1), (1, 1), (2, 1)]
    assert any(C.push_knobs("static", k)[1] <= row < length for row, _ in C.test_rows(length, k))      # a test from row k + 32 on, before last
    want, low = C.band_dp(q, s, k, rows=True)
    ref = O.banded64(q, s, k)
    assert np.array_equal(want, ref) and np.array_equal(O.dp_banded(q, s, k), ref)
    assert np.array_equal(ref == 127, low[..., R.banded_last_check(length, k)] > 2 * k + 1)
    assert (ref != 127).sum() == C.FLUSH_NQ * (8 + 9 + 4)
    for qi in (0, 8, 15):
        assert np.array_equal(R.banded_simulate(s, q[qi], k), ref[qi]), qi
    for config in ("static", "counter"):
        routes, seen, flushed = C.routes(k, length, config, low)
        assert flushed == [(0, 0, 8, 64), (2, 0, 15, 60)], (config, flushed)
        assert all(routes[0, qi][0] == "push" and routes[0, qi][2:] == (8, 8) for qi in range(C.FLUSH_NQ)), routes
        assert all(routes[1, qi] == ("end",) and 9 in {n for _, n in seen[1, qi]} for qi in range(C.FLUSH_NQ))
        assert all(routes[2, qi][0] == "push" and routes[2, qi][2:] == (4, 4) for qi in range(C.FLUSH_NQ))
    routes, _, flushed = C.routes(k, length, "first_pass", low)
    assert not flushed and all(x == ("end",) for x in routes.values())
    routes, _, flushed = C.routes(k, length, "dense_pass", low)      # 8, 9 and 4 lanes at the first test: a flush every few queries
    assert all(x[0] == "push" for x in routes.values()) and len(flushed) >= 3


@pytest.mark.parametrize("k", K)
def test_library_streams_equal_the_generator_model_byte_for_byte(k):
    """Extends tests/test_stream_bounds_cpu.py, which only walks the stream."""
    L = B.lib()
    rng = np.random.default_rng(k)
    for length in C.lengths(k):
        row = rng.integers(0, 5, length).astype(np.uint8)
        want = R.banded_stream_bytes(length, k, row, cut=R.banded_cut_rows(k))
        n = L.bgsa_hip_query_stream(B.ALGO_BANDED, row.ctypes.data, length, k, None, 0)
        buf = np.zeros(n, np.uint8)
        assert L.bgsa_hip_query_stream(B.ALGO_BANDED, row.ctypes.data, length, k, buf.ctypes.data, n) == n
        assert buf.tolist() == want, (k, length)


def test_forms_and_blocks():
    assert [C.form(k) for k in (1, 8, 9, 12, 13, 15, 16, 31)] == ["cut16", "cut16", "cut8", "cut8", "funnel32", "funnel32", "funnel64", "funnel64"]
    assert sorted(k for b in C.blocks() for k in C.block_thresholds(b)) == K and len(C.blocks()) == 8
    assert sorted(x for b in C.blocks() for x in C.shapes(b)) == sorted(C.shapes())
    assert sorted(x for b in C.blocks() for x in C.flush_shapes(b)) == sorted(C.FLUSH_SHAPES) and len(C.FLUSH_SHAPES) >= 3
    assert set(C.CONFIGS) == {"static", "counter", "first_pass", "dense_pass"}
    env = C.child_env("dense_pass", {"BGSA_BANDED_IMPL": "c", "BGSA_TASK_TARGET": "1", "HOME": "x"})
    assert env == dict(C.CONFIGS["dense_pass"], HOME="x")

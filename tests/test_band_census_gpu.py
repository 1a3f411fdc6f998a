"""The band census on the MI355X: every subject length of 65 .. 256 bp through the band kernels on the shapes and inputs of
tests/band_census.py — one group per wave, two groups per wave, the rescue band, and either with prefix sharing forced —,
against oracle.dp_edit.  tests/test_band_census_cpu.py proves on the host that those shapes reach every placement of a stream
event and that the inputs stand on both sides of the certificate.

One child process per (configuration, block of 32 subject lengths): the knobs are read once.  Per launch the scores must equal
the DP exactly and the certificate statistics must be what the DP says: bgsa_hip_myers_band_stats = (groups with a lane above B,
groups banded), under the rescue (0, groups) with bgsa_hip_myers_band_rescue_stats = (lanes with D > B' exactly, 0), and (0, 0)
where the band is off.  The counts are what gives the census its bite: a launch that quietly ran full rows would still give
equal scores.  The child reports what the library selected — groups per wave, rescue half-width, prefix depths — per shape, so a
run under another kernel cannot pass.  After the first fault word or HIP error the child launches nothing more."""
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

import band_census as C  # noqa: E402

pytestmark = pytest.mark.gpu

_CHILD = ("import sys; sys.path[:0] = [sys.argv[1], sys.argv[1] + '/tests']\n"
          "import test_band_census_gpu as T\n"
          "T.run_block(sys.argv[2], int(sys.argv[3]))\n")


def run_block(config, block):
    """In the child: every launch of the block; prints one RESULT line."""
    import ctypes

    B = C.B
    L = B.lib()

    def pair(fn):
        st = (ctypes.c_ulonglong * 2)()
        assert fn(st, 1) == 0
        return (int(st[0]), int(st[1]))

    c = C.CONFIGS[config]
    out = {"shapes": 0, "launches": 0, "banded": 0, "lengths": [], "failures": [], "stopped": None}
    a = B.DeviceAligner(B.ALGO_MYERS)
    t0 = time.perf_counter()
    for m, n, q, buckets, h, limit in C.cases(config, block):
        nq, ns = C.launch_shape(config, m, n)
        nw = (n + 31) // 32
        d = (ctypes.c_int * 8)()
        depths = [int(d[j]) for j in range(L.bgsa_hip_myers_prefix_depths(nw, ns, m, n, nq, 0, d, 8))]
        selected = [int(L.bgsa_hip_myers_band_groups(nw, ns, m, n, 0)), int(L.bgsa_hip_myers_band_rescue(m, n, nq, ns)), depths]
        claimed = [C.groups(config, m, n), h if c["rescue"] else 0, C.depths(config, m, n)]
        if selected != claimed:
            out["failures"].append([m, n, config, "selection: groups, rescue half-width, depths", selected, claimed])
            continue
        launches = C.expected(config, q, buckets, h)
        try:
            a.set_queries(q)
            for i, (want, over) in enumerate(launches):
                assert buckets[i].shape[0] == ns
                a.set_subjects(buckets[i])
                pair(L.bgsa_hip_myers_band_stats)
                pair(L.bgsa_hip_myers_band_rescue_stats)
                got = (a.score(0, nq) if c["share"] else a.score(i, i + 1)).cpu().numpy()
                a.check_faults()
                stats = (pair(L.bgsa_hip_myers_band_stats), pair(L.bgsa_hip_myers_band_rescue_stats))
                out["launches"] += 1
                if got.dtype != np.int16 or got.shape != want.shape:
                    out["failures"].append([m, n, config, i, "result", str(got.dtype), list(got.shape)])
                elif not np.array_equal(got, want):
                    row, lane = (int(x) for x in np.argwhere(got != want)[0])
                    out["failures"].append([m, n, config, i if not c["share"] else row, lane, int(got[row, lane]), int(want[row, lane])])
                if stats != C.statistics(config, over, h):
                    out["failures"].append([m, n, config, i, "statistics", stats, C.statistics(config, over, h)])
        except Exception as e:      # a fault word or a HIP error: nothing more is launched
            out["stopped"] = [m, n, config, repr(e)[:300]]
            break
        out["shapes"] += 1
        out["banded"] += 1 if h else 0
        out["lengths"].append(n)
    out["seconds"] = round(time.perf_counter() - t0, 2)
    if out["stopped"] is None:
        out["stream_faults"] = int(L.bgsa_hip_stream_faults(1))
    out["lengths"] = sorted(set(out["lengths"]))
    print("RESULT " + json.dumps(out))


@pytest.mark.parametrize("config,block", [(c, b) for c in C.CONFIGS for b in C.blocks(c)], ids=lambda x: str(x))
def test_band_census(config, block):
    shapes = C.shapes(config, block)
    p = subprocess.run([sys.executable, "-c", _CHILD, str(C.ROOT), config, str(block)], capture_output=True, text=True,
                       timeout=60 + len(shapes) // 2, env=C.child_env(config, os.environ), cwd=str(C.ROOT))
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    r = json.loads([x for x in p.stdout.splitlines() if x.startswith("RESULT ")][-1][7:])
    print(f"band census {config}, block {block}: {r['shapes']} shapes, {r['launches']} launches, {r['seconds']} s in the loop")
    assert r["stopped"] is None, r["stopped"]
    assert not r["failures"], f"{len(r['failures'])} differences, the first: (m, n, configuration, query, lane, got, want) = {r['failures'][:5]}"
    assert r["stream_faults"] == 0
    off = sum(1 for x in shapes if not C.band_on(*x))
    assert (r["shapes"], r["banded"]) == (len(shapes), len(shapes) - off)
    assert r["launches"] == len(shapes) * (1 if C.CONFIGS[config]["share"] else 3)
    assert r["lengths"] == sorted({n for _, n in shapes}) == list(range(65 + 32 * block, 65 + 32 * block + 32))
    if C.CONFIGS[config]["rescue"]:      # the lengths at which a large launch rescues without a knob (asked here, where none is set)
        by_default = [n for n in r["lengths"] if C.rescues_by_default(n, n)]
        print(f"  of them rescue by default: {by_default}")
        assert len(by_default) == 8 or set(C.KNOBS) & set(os.environ)      # 24 in all: tests/test_band_census_cpu.py

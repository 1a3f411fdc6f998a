"""The op list of every public row body of rows_ir.py, pinned by digest: tests/golden/row_body_pins.json holds the sha256 over
the (kind, dst, srcs, imm, dst2) list of each body, under the default knobs and under BGSA_GEN_MYERS_EIGHT=0.  The generator pins
(tests/test_generator_pins_cpu.py) cover what reaches a header; this covers the bodies, widths and arguments that only bench.py,
the tests or scripts/ reach, so a change of rows_ir.py's structure that means to leave every body alone can prove it on the CPU.

After an INTENDED change of a body, re-record with

    python3 tests/test_row_body_pins_cpu.py --record

and commit the file with the change (`--csrc DIR` records from another copy of bgsa_amd/csrc, e.g. the parent commit's)."""
import hashlib
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "bgsa_amd" / "csrc"
PINS = ROOT / "tests" / "golden" / "row_body_pins.json"
SETTINGS = ["default", "BGSA_GEN_MYERS_EIGHT=0"]


def sweep(R):
    """(key, body) of every pinned call."""
    for nw in range(1, 33):
        for groups in (1, 2) if nw <= 5 else (1,):
            for split in (0, 8, 9):
                for park in ("sgpr", "vgpr"):
                    for balanced in (False, True):
                        yield (f"myers_body({nw}, {groups}, split={split}, park={park}, balanced={balanced})",
                               R.myers_body(nw, groups, split, park, balanced))
        for split in (0, 9):
            yield f"myers_semi_body({nw}, split={split})", R.myers_semi_body(nw, split)
    for nw in range(10, 33, 2):
        for split in (0, 9):
            for balanced in (False, True):
                yield f"myers_planes_body({nw}, split={split}, balanced={balanced})", R.myers_planes_body(nw, split, balanced)
    for nw in range(26, 33, 2):
        yield f"myers_semi_planes_body({nw})", R.myers_semi_planes_body(nw)
    for nw in range(12, 29, 2):
        yield f"myers_block_body({nw})", R.myers_block_body(nw)
        yield f"myers_peq_block_body({nw})", R.myers_peq_block_body(nw)
    for nw in range(1, 9):
        for groups in (1, 2):
            yield f"myers_body10({nw}, {groups})", R.myers_body10(nw, groups)
    for nw, a, b in ((5, 0, 4), (5, 1, 3), (8, 2, 2), (8, 3, 7)):
        for groups in (1, 2):
            for balanced in (False, True):
                yield (f"myers_window_body({nw}, {a}, {b}, groups={groups}, balanced={balanced})",
                       R.myers_window_body(nw, a, b, groups, balanced))
    yield "banded_body()", R.banded_body()
    yield "banded_body64()", R.banded_body64()
    yield "banded_phase_body()", R.banded_phase_body()
    for g in (0, 1):
        yield f"banded_body64_sh64({g})", R.banded_body64_sh64(g)
    for groups in (1, 2):
        yield f"banded_cut_body({groups})", R.banded_cut_body(groups)
        for wide, sh64 in ((False, False), (True, False), (True, True)):
            yield f"banded_funnel_body({groups}, wide={wide}, sh64={sh64})", R.banded_funnel_body(groups, wide, sh64)
    for nw in (1, 5):
        yield f"bitpal_body({nw})", R.bitpal_body(nw)
    yield "bitpal_block_body(4)", R.bitpal_block_body(4)[0]
    yield "bitpal_packed_block_body(4)", R.bitpal_packed_block_body(4)[0]


def digests(csrc: Path) -> dict:
    spec = importlib.util.spec_from_file_location("rows_ir_pinned", csrc / "rows_ir.py")
    R = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = R
    spec.loader.exec_module(R)
    return {key: hashlib.sha256(repr([(op.kind, op.dst, op.srcs, op.imm, op.dst2) for op in body.ops]).encode()).hexdigest()
            for key, body in sweep(R)}


def child_digests(csrc: Path, setting: str) -> dict:
    """The sweep in a fresh process: the knobs are read when rows_ir.py is imported."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("BGSA_GEN_")}
    if setting != "default":
        env.update([setting.split("=", 1)])
    p = subprocess.run([sys.executable, __file__, "--digests", "--csrc", str(csrc)], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout)


@pytest.mark.parametrize("setting", SETTINGS)
def test_row_bodies(setting):
    pins = json.loads(PINS.read_text())
    assert sorted(pins) == sorted(SETTINGS)
    got = child_digests(CSRC, setting)
    assert sorted(got) == sorted(pins[setting])
    assert [k for k in got if got[k] != pins[setting][k]] == []


if __name__ == "__main__":
    csrc = Path(sys.argv[sys.argv.index("--csrc") + 1]).resolve() if "--csrc" in sys.argv else CSRC
    if "--digests" in sys.argv:
        print(json.dumps(digests(csrc)))
    else:
        assert "--record" in sys.argv, __doc__
        record = {setting: child_digests(csrc, setting) for setting in SETTINGS}
        PINS.write_text(json.dumps(record, indent=1) + "\n")
        print(f"{PINS}: {sum(len(v) for v in record.values())} digests from {csrc}")

"""Everything the row-loop generator can write, pinned by digest: tests/golden/generator_pins.json holds the sha256 of
every header gen_rows_asm.py / gen_bitpal_sets.py produce — the band header (built, not committed), the row loops of every
score set of the Makefile's BITPAL_SETS and BITPAL_SETS_AB, and for every BGSA_GEN_* knob setting of KNOBS the three
committed-by-default headers plus the band header.  tests/test_generated_inc_cpu.py covers the default knobs byte for byte;
this covers what a measurement build (scripts/build_variant.sh) would compile, so a change of the generator's structure that
means to leave the emitted text alone can prove it on the CPU.  Identical text = identical compiler input.

After an INTENDED change of the generated text, re-record with

    python3 tests/test_generator_pins_cpu.py --record

and commit the file with the change (`--csrc DIR` records from another copy of bgsa_amd/csrc, e.g. the parent commit's)."""
import hashlib
import json
import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "bgsa_amd" / "csrc"
PINS = ROOT / "tests" / "golden" / "generator_pins.json"
HEADERS = ("myers_rows_gen.inc", "bitpal_rows_gen.inc", "banded_rows_gen.inc")
BAND = "myers_band_rows_gen.inc"
KNOBS = [
    "BGSA_GEN_MYERS_SPLIT=8",
    "BGSA_GEN_MYERS_PARK=vgpr",
    "BGSA_GEN_MYERS_ILP=0,24",
    "BGSA_GEN_MYERS_ILP=1,24",
    "BGSA_GEN_MYERS_BALANCED=1",
    "BGSA_GEN_MYERS_ILP_PLANES=1",
    "BGSA_GEN_MYERS_PLANES_SPLIT=9",
    "BGSA_GEN_MYERS_BAND_PAIR_WINDOW=16",
    "BGSA_GEN_MYERS_EIGHT=0",
    "BGSA_GEN_BITPAL_WINDOW=0",
    "BGSA_GEN_BITPAL_ONE_CHAIN=1",
    "BGSA_GEN_BITPAL_INLINE_LE=0",
    "BGSA_GEN_BITPAL_CELL_MAX=0",
    "BGSA_GEN_BITPAL_FOLD_LAST_Z=0",
    "BGSA_GEN_BITPAL_NO_RUN=0",
    "BGSA_GEN_BANDED_WEAVE=0",
]


def _run(csrc: Path, args: list, knob: str = ""):
    env = {k: v for k, v in os.environ.items() if not k.startswith("BGSA_GEN_")}
    if knob:
        env.update([knob.split("=", 1)])
    p = subprocess.run([sys.executable, *map(str, args)], capture_output=True, text=True, timeout=900, env=env, cwd=csrc)
    assert p.returncode == 0, p.stderr[-2000:]


def _digests(out: Path, names) -> dict:
    return {name: hashlib.sha256((out / name).read_bytes()).hexdigest() for name in names}


def generate_knob(csrc: Path, out: Path, knob: str) -> dict:
    """The three headers and the band header under one knob setting ("" = the defaults)."""
    out.mkdir(parents=True, exist_ok=True)
    _run(csrc, [csrc / "gen_rows_asm.py", "--out", out], knob)
    _run(csrc, [csrc / "gen_rows_asm.py", "--band", out / BAND], knob)
    return _digests(out, HEADERS + (BAND,))


def generate_sets(csrc: Path, out: Path) -> dict:
    """bitpal_rows_<tag>.inc of every score set the Makefile builds (the default set's rows are bitpal_rows_gen.inc)."""
    mk = (CSRC / "Makefile").read_text()
    sets = re.search(r"^BITPAL_SETS \?= (.*)$", mk, re.M).group(1).split()
    ab = re.search(r"^BITPAL_SETS_AB \?= (.*)$", mk, re.M).group(1).split()
    out.mkdir(parents=True, exist_ok=True)
    _run(csrc, [csrc / "gen_bitpal_sets.py", "--out", out, *sets, "--ab", *ab])
    names = sorted(f.name for f in out.glob("bitpal_rows_*.inc"))
    assert len(names) == len(set(sets + ab)) - 1, names      # every set but the default 2/-3/-5 has a header of its own
    return _digests(out, names)


@pytest.fixture(scope="module")
def pins():
    return json.loads(PINS.read_text())


def test_every_knob_setting_is_pinned(pins):
    assert sorted(pins) == sorted(["default", "score_sets"] + KNOBS)


def test_default_knobs(pins, tmp_path):
    assert generate_knob(CSRC, tmp_path, "") == pins["default"]


def test_score_sets(pins, tmp_path):
    assert generate_sets(CSRC, tmp_path) == pins["score_sets"]


@pytest.mark.parametrize("knob", KNOBS)
def test_knob(pins, tmp_path, knob):
    assert generate_knob(CSRC, tmp_path, knob) == pins[knob]


if __name__ == "__main__":
    import tempfile
    assert "--record" in sys.argv, __doc__
    csrc = Path(sys.argv[sys.argv.index("--csrc") + 1]).resolve() if "--csrc" in sys.argv else CSRC
    with tempfile.TemporaryDirectory() as tmp:
        record = {"default": generate_knob(csrc, Path(tmp) / "default", ""), "score_sets": generate_sets(csrc, Path(tmp) / "sets")}
        for i, knob in enumerate(KNOBS):
            record[knob] = generate_knob(csrc, Path(tmp) / f"k{i}", knob)
    PINS.write_text(json.dumps(record, indent=1) + "\n")
    print(f"{PINS}: {sum(len(v) for v in record.values())} digests from {csrc}")

"""Which kernel the knobs select, pinned: bgsa_hip_kernel_name() of both library flavours under every knob environment of
tests/golden/kernel_names.json must answer what the build of the selection functions' parent commit answered.  The names are
what bench lines, the PMC stamping and the parity tests treat as "the kernel that ran"; myers_select / banded_select / the
per-set bitpal_select (bgsa_amd/csrc) are the one place they come from.  No GPU: the names are host logic."""
import json
import os
import subprocess
import sys

import pytest

import bgsa_amd as B
from conftest import GOLDEN

TABLE = json.loads((GOLDEN / "kernel_names.json").read_text())["libraries"]

# The knobs are read once per process, so every (library, environment) answers from a child of its own.
_CHILD = r"""
import ctypes, json, sys
L = ctypes.CDLL(sys.argv[1])
L.bgsa_hip_kernel_name.restype = ctypes.c_char_p
name = lambda algo, w: L.bgsa_hip_kernel_name(algo, w).decode()
MYERS, BANDED, BITPAL = 0, 1, 2
out = {}
L.bgsa_hip_select_algorithm(MYERS)
L.bgsa_hip_select_alignment(0)
out["myers_global"] = [name(MYERS, w) for w in range(1, 131)]
L.bgsa_hip_select_alignment(1)
out["myers_semi_global"] = [name(MYERS, w) for w in range(1, 131)]
L.bgsa_hip_select_alignment(0)
L.bgsa_hip_select_algorithm(BITPAL)                      # the default set, 2/-3/-5
out["bitpal_default_set"] = [name(BITPAL, w) for w in range(1, 41)]
assert L.bgsa_hip_select_scores(10, -9, -15) == 0
out["bitpal_10_-9_-15"] = [name(BITPAL, w) for w in range(1, 41)]
L.bgsa_hip_select_algorithm(BANDED)
out["banded_default_k"] = name(BANDED, 5)
print(json.dumps(out))
"""


@pytest.fixture(scope="module")
def libraries():
    if not (B.LIB_PATH.exists() and B.LIB_AB_PATH.exists()):
        B.build_library()
    return {"libbgsa_hip.so": B.HERE / "libbgsa_hip.so", "libbgsa_hip_ab.so": B.LIB_AB_PATH}


def _environment(label):
    return dict(kv.split("=", 1) for kv in label.split()) if label != "default" else {}


@pytest.mark.parametrize("label", sorted(TABLE["libbgsa_hip.so"]))
@pytest.mark.parametrize("flavour", sorted(TABLE))
def test_kernel_names_are_the_parent_commits(libraries, flavour, label):
    knobs = ("BGSA_MYERS_", "BGSA_BANDED_", "BGSA_BITPAL_", "BGSA_HIP_LIB")
    env = {k: v for k, v in os.environ.items() if not k.startswith(knobs)}
    p = subprocess.run([sys.executable, "-c", _CHILD, str(libraries[flavour])], env=dict(env, **_environment(label)),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    got, want = json.loads(p.stdout), TABLE[flavour][label]
    assert sorted(got) == sorted(want)
    for key in want:
        if got[key] != want[key]:
            pairs = [got[key], want[key]] if isinstance(want[key], str) else \
                    [(i + 1, g, w) for i, (g, w) in enumerate(zip(got[key], want[key])) if g != w][:5]
            pytest.fail(f"{flavour} [{label}] {key}: (word count, got, recorded) {pairs}")


def test_the_table_covers_what_it_says():
    assert sorted(TABLE) == ["libbgsa_hip.so", "libbgsa_hip_ab.so"]
    for flavour in TABLE:
        assert len(TABLE[flavour]) == 7 and "default" in TABLE[flavour]
        for names in TABLE[flavour].values():
            assert len(names["myers_global"]) == len(names["myers_semi_global"]) == 130
            assert len(names["bitpal_default_set"]) == len(names["bitpal_10_-9_-15"]) == 40
            assert names["banded_default_k"].startswith("banded_")

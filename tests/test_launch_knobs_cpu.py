"""The launch knobs of the environment (csrc/bn254_g16_plan.h::launch_knobs behind bn254_dbg_launch_knobs): BN254_COOP, BN254_MILLER_RUN_STEPS and
BN254_COOP_FIXED_MAX are read once per process by one reader, and each launcher that takes BN254_MILLER_RUN_STEPS keeps its own rule for what a value means.
Every case is a fresh process, because the values are read once; no GPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 88                       # csrc/bn254_constants.h: BN_ATE_STEPS, the whole Miller loop

_CHILD = ("import ctypes as C, importlib, sys; sys.path.insert(0, %r); L = importlib.import_module('snark-bn254-verifier_amd').lib(); "
          "out = (C.c_int * 6)(); assert L.bn254_dbg_launch_knobs(out) == 0; print(list(out))" % ROOT)
_KNOBS = ("BN254_COOP", "BN254_MILLER_RUN_STEPS", "BN254_COOP_FIXED_MAX", "BN254_WIDE_PER")


def _knobs(**env):
    """{coop_on, steps of bn254_launch_g16, of bn254_launch_g16_keys, of bn254_launch_pairing2_fixed_lanes, of bn254_launch_pairing2_fixed_keys, coop_fixed_max} as a
    process started with `env` (and none of the knobs otherwise) sees them"""
    e = {k: v for k, v in os.environ.items() if k not in _KNOBS}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=e, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(v) for v in re.findall(r"-?\d+", r.stdout.strip().split("\n")[-1])]


def _coop_max_fixed():
    with open(os.path.join(ROOT, "snark-bn254-verifier_amd", "csrc", "bn254_kernels.h")) as f:
        return int(re.search(r"^#define COOP12_MAX_PROOFS_FIXED (\d+)", f.read(), re.M).group(1))


# BN254_MILLER_RUN_STEPS -> what bn254_launch_g16 and bn254_launch_g16_keys hand to g16_launch_form (-1: the plan's choice; 0, one key only: one launch per step) and the
# steps per launch of bn254_launch_pairing2_fixed_lanes (0: one launch per operation) and bn254_launch_pairing2_fixed_keys
@pytest.mark.parametrize("value, want", [
    (None, [-1, -1, STEPS, STEPS]),
    ("-5", [-1, -1, STEPS, STEPS]),
    ("-1", [-1, -1, STEPS, STEPS]),
    ("0", [0, -1, 0, STEPS]),
    ("1", [1, 1, 1, 1]),
    ("11", [11, 11, 11, 11]),
    ("88", [88, 88, 88, 88]),
    ("200", [200, 200, 200, 200]),
])
def test_miller_run_steps(value, want):
    got = _knobs(**({} if value is None else {"BN254_MILLER_RUN_STEPS": value}))
    assert got[1:5] == want
    assert got[0] == 1 and got[5] == _coop_max_fixed()          # the other knobs are untouched


@pytest.mark.parametrize("value, want", [(None, 1), ("0", 0), ("1", 1), ("7", 1)])
def test_coop(value, want):
    got = _knobs(**({} if value is None else {"BN254_COOP": value}))
    assert got[0] == want
    assert got[1:5] == [-1, -1, STEPS, STEPS]


@pytest.mark.parametrize("value, want", [(None, None), ("0", 0)])
def test_coop_fixed_max(value, want):
    got = _knobs(**({} if value is None else {"BN254_COOP_FIXED_MAX": value}))
    assert got[5] == (_coop_max_fixed() if want is None else want)

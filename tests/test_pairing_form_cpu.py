"""The choice between the two forms of a launch of the batch pairing product (csrc/bn254_g16_plan.h::pairing_form behind bn254_dbg_pairing_form; the lane kernels
of csrc/bn254_k_pairing.hip or csrc/bn254_coop12.hip::k_coop12_miller_pairs), without a GPU: the rule n <= coop_max at every pair count, BN254_COOP=0, the clamp and
the read-back of bn254_set_pairing_params, and the argument errors of the probe that forces a form."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LANES, COOP = 1, 2
COOP12_MAX_PROOFS = 30720        # csrc/bn254_kernels.h: the cooperative kernels' range
DEFAULT_COOP_MAX = 16384         # csrc/bn254_g16_plan.h: PAIRING_COOP_MAX_DEFAULT, from the table of DESIGN.md section 9j
E_BAD_ARG = -1
_ENV = ("BN254_COOP", "BN254_PAIRING_COOP_MAX")


@pytest.fixture
def knob(pkg):
    before = pkg.pairing_params()
    yield pkg
    pkg.set_pairing_params(before)


def _coop_on():
    v = os.environ.get("BN254_COOP")
    try:
        return v is None or int(v) != 0
    except ValueError:
        return False           # atoi of a text without digits is 0


def _expected(n, coop_max):
    return COOP if _coop_on() and n <= coop_max and n <= COOP12_MAX_PROOFS else LANES


def test_plan_follows_the_documented_rule(knob):
    """n <= coop_max at every pair count: the rule is on the items of the launch alone"""
    pkg = knob
    for coop_max in (0, 1, 5, 4096, 4097, COOP12_MAX_PROOFS):
        pkg.set_pairing_params(coop_max)
        assert pkg.pairing_params() == coop_max
        for k in range(1, 9):
            for n in sorted({1, 2, 5, 6, max(coop_max - 1, 1), max(coop_max, 1), coop_max + 1, COOP12_MAX_PROOFS, COOP12_MAX_PROOFS + 1, 2 ** 18, 10 ** 6}):
                assert pkg.dbg_pairing_form(k, n) == _expected(n, coop_max), (coop_max, k, n)


def test_never_cooperative_above_the_kernels_range(knob):
    pkg = knob
    pkg.set_pairing_params(10 ** 12)
    assert pkg.pairing_params() == COOP12_MAX_PROOFS
    for k in range(1, 9):
        for n in (COOP12_MAX_PROOFS + 1, 40960, 65536, 786432):
            assert pkg.dbg_pairing_form(k, n) == LANES


def test_set_pairing_params_clamps_keeps_and_switches_off(knob):
    pkg = knob
    pkg.set_pairing_params(1234)
    assert pkg.pairing_params() == 1234
    pkg.set_pairing_params(-1)                      # negative: unchanged
    assert pkg.pairing_params() == 1234
    pkg.set_pairing_params(-10 ** 9)
    assert pkg.pairing_params() == 1234
    pkg.set_pairing_params(COOP12_MAX_PROOFS + 1)   # clamped to the cooperative range
    assert pkg.pairing_params() == COOP12_MAX_PROOFS
    pkg.set_pairing_params(0)                       # 0: the lane form at every size
    assert pkg.pairing_params() == 0
    assert [pkg.dbg_pairing_form(k, n) for k in (1, 8) for n in (1, 5, 4096)] == [LANES] * 6
    L = pkg.lib()
    L.bn254_pairing_params.argtypes = [C.c_void_p]
    L.bn254_pairing_state.argtypes = [C.c_void_p]
    assert L.bn254_pairing_params(None) == E_BAD_ARG and L.bn254_pairing_state(None) == E_BAD_ARG
    a, b = pkg.pairing_state()
    assert a >= 0 and b >= 0


def _child(code, **env):
    e = {k: v for k, v in os.environ.items() if k not in _ENV}
    e.update(env)
    r = subprocess.run([sys.executable, "-c", "import importlib, sys; sys.path.insert(0, %r); pkg = importlib.import_module('snark-bn254-verifier_amd'); " % ROOT + code],
                       env=e, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return eval(r.stdout.strip().splitlines()[-1])


def test_coop_off_answers_lane_everywhere():
    """BN254_COOP is read once per process: a child process, as tests/test_launch_knobs_cpu.py does"""
    code = "pkg.set_pairing_params(30720); print([pkg.dbg_pairing_form(k, n) for k in range(1, 9) for n in (1, 5, 4096, 30720, 30721)])"
    assert _child(code, BN254_COOP="0") == [LANES] * 40
    assert _child(code, BN254_COOP="1") == [COOP, COOP, COOP, COOP, LANES] * 8


def test_initial_value_from_the_environment():
    code = "print([pkg.pairing_params(), pkg.dbg_pairing_form(2, 100), pkg.dbg_pairing_form(2, 101)])"
    assert _child(code) == [DEFAULT_COOP_MAX, COOP, COOP if 101 <= DEFAULT_COOP_MAX else LANES]
    assert _child(code, BN254_PAIRING_COOP_MAX="100") == [100, COOP, LANES]
    assert _child(code, BN254_PAIRING_COOP_MAX="0") == [0, LANES, LANES]
    assert _child(code, BN254_PAIRING_COOP_MAX="99999999") == [COOP12_MAX_PROOFS, COOP, COOP]
    assert _child(code, BN254_PAIRING_COOP_MAX="-3")[0] == DEFAULT_COOP_MAX


def test_form_probe_argument_errors_touch_nothing(pkg):
    L = pkg.lib()
    L.bn254_last_error.restype = C.c_char_p
    fn = L.bn254_dbg_pairing_batch_form
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    L.bn254_dbg_pairing_form.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_int)]
    item = bytes(192 * 8)
    st = (C.c_uint8 * 4)(*([0xEE] * 4)); gt = (C.c_uint8 * (384 * 4))(*([0xEE] * (384 * 4)))
    stp, gtp = C.cast(st, C.c_void_p), C.cast(gt, C.c_void_p)
    no_such_device = 4097

    def untouched():
        return bytes(st) == b"\xee" * 4 and bytes(gt) == b"\xee" * (384 * 4)

    for form in (0, LANES, COOP):
        assert fn(None, 192, 1, 1, gtp, stp, no_such_device, form) == E_BAD_ARG and untouched(), form            # the sibling's argument errors
        assert fn(item, 192, 1, 1, gtp, None, no_such_device, form) == E_BAD_ARG and untouched(), form
        assert fn(item, 192, 0, 1, gtp, stp, no_such_device, form) == E_BAD_ARG and untouched(), form
        assert fn(item, 192 * 9, 9, 1, gtp, stp, no_such_device, form) == E_BAD_ARG and untouched(), form
        assert fn(item, 191, 1, 1, gtp, stp, no_such_device, form) == E_BAD_ARG and untouched(), form
        assert fn(item, 192 * 3, 3, 0, gtp, stp, no_such_device, form) == 0 and untouched(), form                # n == 0
        rc = fn(item, 192, 1, 1, gtp, stp, no_such_device, form)                                                 # past the checks: the device ordinal
        assert rc in (-1, -2) and untouched() and b"device" in L.bn254_last_error().lower(), form
    for form in (LANES, COOP):
        assert fn(item, 192, 1, 1, gtp, stp, -1, form) == E_BAD_ARG and untouched(), form                        # a forced form runs on a device
        assert b"form" in L.bn254_last_error().lower()
    for form in (-1, 3, 77):
        assert fn(item, 192, 1, 1, gtp, stp, 0, form) == E_BAD_ARG and untouched(), form
    big = bytes(192) * (COOP12_MAX_PROOFS + 1)
    big_st = (C.c_uint8 * (COOP12_MAX_PROOFS + 1))(*([0xEE] * (COOP12_MAX_PROOFS + 1)))
    assert fn(big, 192, 1, COOP12_MAX_PROOFS + 1, None, C.cast(big_st, C.c_void_p), 0, COOP) == E_BAD_ARG         # above the cooperative range, before the device
    assert bytes(big_st) == b"\xee" * (COOP12_MAX_PROOFS + 1)
    out = C.c_int(77)
    assert L.bn254_dbg_pairing_form(0, 1, C.byref(out)) == E_BAD_ARG and L.bn254_dbg_pairing_form(9, 1, C.byref(out)) == E_BAD_ARG and out.value == 77
    assert L.bn254_dbg_pairing_form(1, 1, None) == E_BAD_ARG
    # form 0 is the sibling: the host compile answers without a device
    z = bytes(192)
    assert fn(z, 192, 1, 1, None, stp, -1, 0) == 0 and st[0] == 1                                                # (0, 0) pairs: the product is 1

"""What needs no GPU of the cooperative and BN254_FLAG_RLC forms of the PlonK batches over key lists: the argument checks of bn254_plonk_keys_state and of the
probe bn254_dbg_coop12_miller_fixed_keys (made before any device is touched), the clamps of bn254_set_plonk_keys_params and bn254_set_plonk_rlc_params, and the
names of the new entries on the Python, C++ and Rust surfaces."""
import ctypes as C
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD = -1
COOP12_MAX_PROOFS_FIXED = 40960


@pytest.fixture(scope="module")
def two_keys(pkg):
    keys = []
    for seed, shape in ((0x51A0, (2, 1, 6)), (0x51A1, (1, 1, 5))):
        vk, _, _, _ = pkg.synth_plonk(seed, shape[0], shape[1], shape[2], 1, invalid_every=0, threads=1)
        keys.append(pkg.PreparedPlonkVk(vk))
    yield keys
    for k in keys:
        k.close()


def test_state_refuses_null_pointers_and_lists_that_are_not_cached(pkg, two_keys):
    L = pkg.lib()
    fn = L.bn254_plonk_keys_state
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_uint64)]
    arr = (C.c_void_p * 2)(*[k._h.value for k in two_keys])
    out = (C.c_uint64 * 4)(7, 7, 7, 7)
    assert fn(None, 2, 0, out) == BAD
    assert fn(arr, 2, 0, None) == BAD
    assert fn(arr, 0, 0, out) == BAD
    assert fn((C.c_void_p * 2)(two_keys[0]._h.value, None), 2, 0, out) == BAD
    assert fn(arr, 2, 0, out) == BAD and b"cached" in L.bn254_last_error()       # prepared, never used in a list
    assert list(out) == [7, 7, 7, 7]
    with pytest.raises(Exception):
        pkg.PlonkKeySet(two_keys).state()


def test_setters_clamp_and_leave_alone(pkg):
    coop0, rlc0 = pkg.dbg_plonk_keys_knobs()
    try:
        assert 0 <= coop0 <= COOP12_MAX_PROOFS_FIXED and rlc0 >= 64
        pkg.set_plonk_keys_params(10 ** 12)
        assert pkg.dbg_plonk_keys_knobs() == (COOP12_MAX_PROOFS_FIXED, rlc0)           # clamped to the range of the cooperative kernel
        pkg.set_plonk_keys_params(0)
        assert pkg.dbg_plonk_keys_knobs()[0] == 0
        pkg.set_plonk_keys_params(-1)
        assert pkg.dbg_plonk_keys_knobs()[0] == 0                                     # a negative value leaves the knob alone
        pkg.set_plonk_keys_params(4096)
        assert pkg.dbg_plonk_keys_knobs()[0] == 4096
        pkg.set_plonk_rlc_params(0)
        assert pkg.dbg_plonk_keys_knobs() == (4096, 64)                               # never below a group
        pkg.set_plonk_rlc_params(63)
        assert pkg.dbg_plonk_keys_knobs()[1] == 64
        pkg.set_plonk_rlc_params(100000)
        assert pkg.dbg_plonk_keys_knobs()[1] == 100000
        pkg.set_plonk_rlc_params(-7)
        assert pkg.dbg_plonk_keys_knobs()[1] == 100000
        fn = pkg.lib().bn254_dbg_plonk_keys_knobs
        fn.argtypes = [C.c_void_p]
        assert fn(None) == BAD
    finally:
        pkg.set_plonk_keys_params(coop0)
        pkg.set_plonk_rlc_params(rlc0)
    assert pkg.dbg_plonk_keys_knobs() == (coop0, rlc0)


def test_default_of_the_knob_from_the_environment():
    """BN254_PLONK_KEYS_COOP_MAX and BN254_PLONK_RLC_MIN are read once, when the library is loaded: a fresh interpreter per value"""
    import subprocess
    import sys
    code = ("import sys; sys.path.insert(0, %r); import torch, importlib; pkg = importlib.import_module('snark-bn254-verifier_amd'); print(*pkg.dbg_plonk_keys_knobs())" % ROOT)
    for env, want in (({}, None), ({"BN254_PLONK_KEYS_COOP_MAX": "1000", "BN254_PLONK_RLC_MIN": "5"}, (1000, 64)), ({"BN254_PLONK_KEYS_COOP_MAX": "999999"}, (COOP12_MAX_PROOFS_FIXED, 8192))):
        base = {k: v for k, v in os.environ.items() if k not in ("BN254_PLONK_KEYS_COOP_MAX", "BN254_PLONK_RLC_MIN")}
        r = subprocess.run([sys.executable, "-c", code], env=dict(base, **env), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        got = tuple(int(x) for x in r.stdout.split()[-2:])
        if want is None:
            assert 0 <= got[0] <= COOP12_MAX_PROOFS_FIXED and got[1] == 8192
        else:
            assert got == want


def test_probe_arguments_are_checked_before_any_device(pkg, two_keys):
    L = pkg.lib()
    fn = L.bn254_dbg_coop12_miller_fixed_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_uint, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_size_t, C.c_int]
    arr = (C.c_void_p * 2)(*[k._h.value for k in two_keys])
    words = (C.c_uint32 * 4)(0, 1, 0, 1)
    g1 = bytes(64 * 4)
    out = (C.c_uint8 * (384 * 4))()
    good = [arr, 2, words, 0, g1, g1, None, out, 4, 0]
    for pos, v in ((0, None), (1, 0), (2, None), (3, 32), (4, None), (5, None), (7, None), (8, 0), (8, COOP12_MAX_PROOFS_FIXED + 1)):
        args = list(good)
        args[pos] = v
        assert fn(*args) == BAD, (pos, v)
    assert fn((C.c_void_p * 2)(two_keys[0]._h.value, None), 2, words, 0, g1, g1, None, out, 4, 0) == BAD
    assert bytes(out) == bytes(384 * 4)


def test_surfaces_name_the_new_entries(pkg):
    for name in ("set_plonk_keys_params", "set_plonk_rlc_params", "dbg_plonk_keys_knobs"):
        assert callable(getattr(pkg, name))
    assert callable(pkg.PlonkKeySet.state) and callable(pkg.PlonkKeySet.dbg_coop12_miller_fixed)
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, hpp = read("include", "bn254_verify.h"), read("include", "bn254_verify.hpp")
    sys_rs, safe_rs = read("rust", "bn254-verify-amd-sys", "src", "lib.rs"), read("rust", "bn254-verify-amd", "src", "lib.rs")
    for name in ("bn254_set_plonk_keys_params", "bn254_set_plonk_rlc_params", "bn254_plonk_keys_state"):
        assert name + "(" in hdr and name + "(" in hpp and "pub fn %s(" % name in sys_rs and "sys::%s(" % name in safe_rs, name
        assert hasattr(pkg.lib(), name)
    assert "bn254_dbg_coop12_miller_fixed_keys(" in hdr and hasattr(pkg.lib(), "bn254_dbg_coop12_miller_fixed_keys")
    assert "accepted and IGNORED: by its contract the status bytes are those of the exact path (a group of 64" not in hdr

"""Groth16 batches over many verifying keys (include/bn254_verify.h, "Batches over many keys"): what needs no GPU.

The grouping (csrc/bn254_keys.h) compiled for the host behind bn254_dbg_g16_keys_group(device = -1): proofs are brought into slots so that every granule of 64
consecutive slots holds proofs of one key.  The assertions are conditions on any valid grouping, not measurements.  Then the argument checks of the three entries;
with valid arguments and no device they answer BN254_E_NO_DEVICE (there is no CPU fallback)."""
import array
import ctypes as C
import random

import pytest

G = 64                       # csrc/bn254_keys.h: G16_KEYS_GRANULE
NO_PROOF = 0xFFFFFFFF
OK, E_BAD_ARG, E_NO_DEVICE, E_HIP = 0, -1, -2, -3


def _have_gpu():
    import torch
    return torch.cuda.is_available()


def _check_grouping(pkg, key_index, n_keys, device=-1):
    n = len(key_index)
    s2p, gk, n_slots = pkg.dbg_keys_group(key_index, n_keys, device)
    counts = {}
    for k in key_index:
        counts[k] = counts.get(k, 0) + 1
    bound = n + min(n_keys, n) * (G - 1)
    assert len(s2p) == bound // G * G and len(gk) == len(s2p) // G          # the workspace formula, in whole granules
    assert n_slots == sum((c + G - 1) // G * G for c in counts.values())     # every key that has proofs pads its run to whole granules, no key without proofs takes a slot
    assert n_slots % G == 0 and n_slots <= len(s2p) and n_slots - n <= (G - 1) * len(counts)
    live = [p for p in s2p[:n_slots] if p != NO_PROOF]
    assert sorted(live) == list(range(n))                                    # every proof index exactly once
    assert all(p == NO_PROOF for p in s2p[n_slots:])
    for g in range(n_slots // G):
        keys = {key_index[p] for p in s2p[G * g:G * g + G] if p != NO_PROOF}
        assert keys == {gk[g]}, (g, keys, gk[g])                             # single-key, not empty, and the granule -> key word agrees
    return n_slots


@pytest.mark.parametrize("n", [1, G - 1, G, G + 1, 100003])
def test_grouping_sizes(pkg, n):
    rng = random.Random(n)
    assert _check_grouping(pkg, [0] * n, 1) == (n + G - 1) // G * G                              # one key
    _check_grouping(pkg, [rng.randrange(2) for _ in range(n)], 2)
    _check_grouping(pkg, [rng.randrange(257) for _ in range(n)], 257)
    _check_grouping(pkg, [rng.choice([0, 77, 65535, 40000]) for _ in range(n)], 65536)           # most keys empty
    half = [5 if i % 2 else rng.randrange(300) for i in range(n)]                                # skewed: half the proofs on one key
    _check_grouping(pkg, half, 300)


def test_grouping_every_proof_its_own_key(pkg):
    for n in (1, 2, G, 1000, 65536):
        perm = list(range(n))
        random.Random(n).shuffle(perm)
        assert _check_grouping(pkg, perm, n) == n * G


def test_grouping_refuses_bad_arguments(pkg):
    L = pkg.lib()
    L.bn254_dbg_g16_keys_group.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    idx = array.array("I", [0, 0]); out = array.array("I", [0] * 256); ns = C.c_size_t()
    a, o = idx.buffer_info()[0], out.buffer_info()[0]
    assert L.bn254_dbg_g16_keys_group(None, 2, 1, -1, o, o, C.byref(ns)) == E_BAD_ARG
    assert L.bn254_dbg_g16_keys_group(a, 2, 0, -1, o, o, C.byref(ns)) == E_BAD_ARG
    assert L.bn254_dbg_g16_keys_group(a, 2, 65537, -1, o, o, C.byref(ns)) == E_BAD_ARG
    assert L.bn254_dbg_g16_keys_group(a, 0, 1, -1, o, o, C.byref(ns)) == E_BAD_ARG


@pytest.fixture(scope="module")
def keys(pkg):
    out = []
    for seed, npub in ((0x4C01, 2), (0x4C02, 1), (0x4C03, 16), (0x4C04, 17)):
        vk, proofs, inputs, exp = pkg.synth_groth16(seed, npub, 4, invalid_every=2, agree=True, threads=2)
        out.append((pkg.PreparedVk(vk), proofs, inputs, exp, npub))
    yield out
    for k in out:
        k[0].close()


def _call(pkg, handles, n_keys, index, proofs, stride, inputs, input_stride, n, status, flags=0, device=0):
    fn = pkg.lib().bn254_groth16_verify_batch_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    return fn(handles, n_keys, index, proofs, stride, inputs, input_stride, n, status, device, flags)


def test_argument_checks(pkg, keys):
    L = pkg.lib()
    k2, k1, k16, k17 = (k[0] for k in keys)
    proofs = keys[0][1]
    arr = (C.c_void_p * 3)(k2.handle.value, k1.handle.value, k16.handle.value)
    idx = array.array("I", [0, 1, 2, 0]); ip = idx.buffer_info()[0]
    rows = bytes(512 * 4)
    st = (C.c_uint8 * 4)(*[0xEE] * 4)
    untouched = lambda: bytes(st) == b"\xee" * 4
    assert _call(pkg, None, 3, ip, proofs, 256, rows, 512, 4, st) == E_BAD_ARG                   # null list
    assert _call(pkg, arr, 0, ip, proofs, 256, rows, 512, 4, st) == E_BAD_ARG                    # empty list
    assert _call(pkg, arr, 3, None, proofs, 256, rows, 512, 4, st) == E_BAD_ARG                  # null index
    assert _call(pkg, arr, 3, ip, None, 256, rows, 512, 4, st) == E_BAD_ARG                      # null proofs
    assert _call(pkg, arr, 3, ip, proofs, 256, None, 512, 4, st) == E_BAD_ARG                    # null inputs while a key has some
    assert _call(pkg, arr, 3, ip, proofs, 256, rows, 512, 4, None) == E_BAD_ARG                  # null status
    assert _call(pkg, arr, 3, ip, proofs, 255, rows, 512, 4, st) == E_BAD_ARG                    # stride below a raw record
    assert _call(pkg, arr, 3, ip, proofs, 256, rows, 512, 4, st, flags=8) == E_BAD_ARG           # unknown flag
    assert _call(pkg, arr, 3, ip, proofs, 256, rows, 511, 4, st) == E_BAD_ARG                    # input_stride below 32 x 16
    assert b"input_stride" in L.bn254_last_error()
    assert _call(pkg, (C.c_void_p * 2)(k2.handle.value, None), 2, ip, proofs, 256, rows, 512, 4, st) == E_BAD_ARG   # null member
    assert untouched()
    # an index outside the list: the host entry checks the whole vector first and leaves status alone
    bad = array.array("I", [0, 1, 3, 0])
    assert _call(pkg, arr, 3, bad.buffer_info()[0], proofs, 256, rows, 512, 4, st) == E_BAD_ARG and untouched()
    assert b"key_index[2]" in L.bn254_last_error()
    # first-version limits say what they are in bn254_last_diagnostic()
    L.bn254_last_diagnostic.restype = C.c_char_p
    wide = (C.c_void_p * 2)(k2.handle.value, k17.handle.value)
    assert _call(pkg, wide, 2, ip, proofs, 256, rows, 1024, 4, st) == E_BAD_ARG and untouched()
    assert b"17 public inputs" in L.bn254_last_diagnostic()
    many = (C.c_void_p * 65537)(*[k2.handle.value] * 65537)
    assert _call(pkg, many, 65537, ip, proofs, 256, rows, 512, 4, st) == E_BAD_ARG and b"65536" in L.bn254_last_diagnostic()
    L.bn254_groth16_reserve_keys.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_int]
    assert L.bn254_groth16_reserve_keys(wide, 2, 100, 0) == E_BAD_ARG
    assert L.bn254_groth16_reserve_keys(None, 2, 100, 0) == E_BAD_ARG
    # n = 0 is BN254_OK and touches nothing (no device needed); the flags are all accepted
    assert _call(pkg, arr, 3, None, None, 256, None, 512, 0, None, flags=7) == OK
    dev = L.bn254_groth16_verify_batch_keys_device
    dev.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    assert dev(arr, 3, None, None, 256, None, 512, 0, None, 0, None, 0) == OK
    assert dev(arr, 3, None, 1, 256, 1, 512, 4, 1, 0, None, 0) == E_BAD_ARG


def test_no_cpu_fallback_and_set_lifetime(pkg, keys):
    """valid arguments: without a device the entries answer BN254_E_NO_DEVICE and leave status alone.  Freeing a member and then preparing / reserving a NEW list is safe
    (the cache forgets every list that contained the freed key); with a GPU the same sequence verifies."""
    L = pkg.lib()
    gpu = _have_gpu()
    vk, proofs, inputs, exp = pkg.synth_groth16(0x4C05, 2, 4, invalid_every=2, agree=True, threads=2)
    for round_ in range(3):
        a, b = pkg.PreparedVk(vk), keys[0][0]
        ks = pkg.KeySet([a, b])
        if gpu:
            ks.reserve(100)
            assert ks.verify_batch([0, 0, 0, 0], proofs, inputs) == exp
            assert ks.verify_batch([1, 1, 1, 1], keys[0][1], keys[0][2]) == keys[0][3]
        else:
            with pytest.raises(pkg.Bn254Error) as e:
                ks.reserve(100)
            assert "-2" in str(e.value)
            arr = (C.c_void_p * 2)(a.handle.value, b.handle.value)
            idx = array.array("I", [0, 0, 1, 0]); st = (C.c_uint8 * 4)(*[0xEE] * 4)
            assert _call(pkg, arr, 2, idx.buffer_info()[0], proofs, 256, inputs, 64, 4, st) == E_NO_DEVICE and bytes(st) == b"\xee" * 4
        a.close()            # the list [a, b] is gone from the cache; the next round's `a` is a new handle (possibly at the same address)

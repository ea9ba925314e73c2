"""PlonK batches over many verifying keys (include/bn254_verify.h, "PlonK batches over many keys"): what needs no GPU.

The argument checks of the three entries (all reported before any device is touched, with the status bytes untouched), the two refusals that come with a
bn254_last_diagnostic() text, BN254_E_NO_DEVICE with valid arguments where there is no GPU, the lifetime of cached lists when a member is freed, and the plan of a
batch over slots (bn254_dbg_plonk_keys_plan): conditions on any valid plan, not measurements.  Key shapes are (n_public, n_qcp, log2_size)."""
import array
import ctypes as C

import pytest

G = 64
OK, E_BAD_ARG, E_NO_DEVICE = 0, -1, -2
FLAG_RLC = 2


def _have_gpu():
    import torch
    return torch.cuda.is_available()


class K:
    def __init__(self, pkg, seed, shape, n=4):
        self.shape = shape
        self.vk, self.proofs, self.inputs, self.exp = pkg.synth_plonk(seed, shape[0], shape[1], shape[2], n, invalid_every=2, threads=2)
        self.stride = 808 + 96 * shape[1]
        self.pvk = pkg.PreparedPlonkVk(self.vk)


@pytest.fixture(scope="module")
def keys(pkg):
    return [K(pkg, 0x9C01, (2, 1, 26)), K(pkg, 0x9C02, (1, 1, 10)), K(pkg, 0x9C03, (3, 2, 20))]


def _host(pkg):
    fn = pkg.lib().bn254_plonk_verify_batch_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_uint]
    return fn


def _dev(pkg):
    fn = pkg.lib().bn254_plonk_verify_batch_keys_device
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_void_p, C.c_int, C.c_void_p, C.c_uint]
    return fn


def _reserve(pkg):
    fn = pkg.lib().bn254_plonk_reserve_keys
    fn.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    return fn


def test_argument_errors_leave_status_untouched(pkg, keys):
    a, b = keys[0], keys[1]
    arr = (C.c_void_p * 2)(a.pvk._h.value, b.pvk._h.value)
    with_null = (C.c_void_p * 2)(a.pvk._h.value, None)
    idx = array.array("I", [0, 0, 1, 1]); ip = idx.buffer_info()[0]
    proofs = a.proofs[:2 * 904] + b.proofs[:2 * 904]
    rows = a.inputs[:128] + b.inputs[:32].ljust(64, b"\xa5") + b.inputs[32:64].ljust(64, b"\xa5")
    host = _host(pkg)

    def call(*args):
        st = (C.c_uint8 * 4)(*[0xEE] * 4)
        full = list(args)
        full[8] = st if full[8] == "st" else full[8]
        rc = host(*full)
        assert bytes(st) == b"\xee" * 4
        return rc

    good = [arr, 2, ip, proofs, 904, rows, 64, 4, "st", 0, 0]

    def bad(**kw):
        names = ["pvks", "n_keys", "idx", "proofs", "stride", "rows", "in_stride", "n", "st", "device", "flags"]
        v = list(good)
        for k, x in kw.items():
            v[names.index(k)] = x
        return call(*v)

    assert bad(pvks=None) == E_BAD_ARG
    assert bad(n_keys=0) == E_BAD_ARG                                  # an empty list
    assert bad(pvks=with_null) == E_BAD_ARG                            # a null member
    assert bad(idx=None) == E_BAD_ARG and bad(proofs=None) == E_BAD_ARG and bad(st=None) == E_BAD_ARG and bad(rows=None) == E_BAD_ARG
    assert bad(stride=903) == E_BAD_ARG                                # below 808 + 96 * n_qcp
    assert bad(in_stride=63) == E_BAD_ARG                              # below 32 x the widest key (2 inputs)
    assert bad(flags=1) == E_BAD_ARG and bad(flags=4) == E_BAD_ARG and bad(flags=FLAG_RLC | 8) == E_BAD_ARG
    # an index outside the list: the host-buffer entry looks at the whole vector first and names the position
    idx2 = array.array("I", [0, 0, 2, 1])
    assert bad(idx=idx2.buffer_info()[0]) == E_BAD_ARG
    assert "key_index[2]" in pkg.lib().bn254_last_error().decode()
    # the device entry and the reservation make the same checks
    dev = _dev(pkg)
    assert dev(None, 2, 1, 1, 904, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 0, 1, 1, 904, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(with_null, 2, 1, 1, 904, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, None, 1, 904, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, None, 904, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, 1, 904, None, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, 1, 904, 1, 64, 4, None, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, 1, 903, 1, 64, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, 1, 904, 1, 32, 4, 1, 0, None, 0) == E_BAD_ARG
    assert dev(arr, 2, 1, 1, 904, 1, 64, 4, 1, 0, None, 1) == E_BAD_ARG
    res = _reserve(pkg)
    assert res(None, 2, 100, 904, 0) == E_BAD_ARG and res(arr, 0, 100, 904, 0) == E_BAD_ARG and res(with_null, 2, 100, 904, 0) == E_BAD_ARG
    assert res(arr, 2, 100, 807, 0) == E_BAD_ARG


def test_refusals_with_a_diagnostic(pkg, keys):
    a, c = keys[0], keys[2]                                            # (2, 1, 26) and (3, 2, 20): one and two commitments
    mixed = (C.c_void_p * 2)(a.pvk._h.value, c.pvk._h.value)
    idx = array.array("I", [0]); st = (C.c_uint8 * 1)(0xEE)
    assert _host(pkg)(mixed, 2, idx.buffer_info()[0], a.proofs, 1000, a.inputs.ljust(96, b"\0"), 96, 1, st, 0, 0) == E_BAD_ARG and bytes(st) == b"\xee"
    d = pkg.last_diagnostic()
    assert "2 BSB22 commitments" in d and "entry 0 has 1" in d and "entry 1" in d, d
    assert _reserve(pkg)(mixed, 2, 10, 1000, 0) == E_BAD_ARG
    many = (C.c_void_p * 257)(*[a.pvk._h.value] * 257)
    assert _host(pkg)(many, 257, idx.buffer_info()[0], a.proofs, 904, a.inputs, 64, 1, st, 0, 0) == E_BAD_ARG and bytes(st) == b"\xee"
    d = pkg.last_diagnostic()
    assert "256" in d and "257" in d, d
    assert _dev(pkg)(many, 257, 1, 1, 904, 1, 64, 1, 1, 0, None, 0) == E_BAD_ARG
    assert _reserve(pkg)(many, 257, 10, 904, 0) == E_BAD_ARG


def test_empty_batch_is_ok_and_touches_nothing(pkg, keys):
    arr = (C.c_void_p * 1)(keys[0].pvk._h.value)
    assert _host(pkg)(arr, 1, None, None, 904, None, 64, 0, None, 0, 0) == OK
    assert _dev(pkg)(arr, 1, None, None, 904, None, 64, 0, None, 0, None, 0) == OK
    assert _host(pkg)(arr, 1, None, None, 904, None, 64, 0, None, 0, FLAG_RLC) == OK
    assert pkg.PlonkKeySet([keys[0].pvk]).verify_batch([], b"", b"") == b""


def test_no_cpu_fallback_and_set_lifetime(pkg, keys):
    """valid arguments: without a device the entries answer BN254_E_NO_DEVICE and leave status alone.  Freeing a member and then building a NEW list with a new handle is
    safe (the cache forgets every list that contained the freed key); with a GPU the same sequence verifies."""
    gpu = _have_gpu()
    b = keys[1]
    fresh = K(pkg, 0x9C04, (2, 1, 8))
    for round_ in range(3):
        a = pkg.PreparedPlonkVk(fresh.vk)
        ks = pkg.PlonkKeySet([a, b.pvk])
        if gpu:
            ks.reserve(100)
            assert ks.verify_batch([0, 0, 0, 0], fresh.proofs, fresh.inputs) == fresh.exp
            assert ks.verify_batch([1, 1, 1, 1], b.proofs, b"".join(b.inputs[32 * j:32 * j + 32].ljust(64, b"\xa5") for j in range(4))) == b.exp
        else:
            with pytest.raises(pkg.Bn254Error) as e:
                ks.reserve(100)
            assert "-2" in str(e.value)
            arr = (C.c_void_p * 2)(a._h.value, b.pvk._h.value)
            idx = array.array("I", [0, 0, 0, 0]); st = (C.c_uint8 * 4)(*[0xEE] * 4)
            assert _host(pkg)(arr, 2, idx.buffer_info()[0], fresh.proofs, 904, fresh.inputs, 64, 4, st, 0, 0) == E_NO_DEVICE and bytes(st) == b"\xee" * 4
            assert _dev(pkg)(arr, 2, 1, 1, 904, 1, 64, 4, 1, 0, None, 0) == E_NO_DEVICE
        a.close()            # the list [a, b] is gone from the cache; the next round's `a` is a new handle (possibly at the same address)


def _round_up(c):
    return (c + G - 1) // G * G


@pytest.mark.parametrize("n_keys", [1, 3, 256])
def test_plan_walk(pkg, n_keys):
    """Every pass starts and ends on a multiple of 64 (the last may end at S, itself one), the passes cover [0, S) exactly once, and none exceeds the capacity a
    reservation for (n, n_keys) gives the contexts -- for the fewest and the most slots a batch of n proofs over n_keys entries can take."""
    for n in (1, 63, 64, 65, 5040, 5041, 9000, 9001, 20000, 40001, 65536, 70000, 262144):
        bound = (n + min(n_keys, n) * (G - 1)) // G * G
        for slots in sorted({_round_up(n), bound}):
            p = pkg.dbg_plonk_keys_plan(n, n_keys, slots)
            assert p["slot_bound"] == bound
            assert 1 <= p["workers"] <= 8 and p["per_worker"] % G == 0 and p["per_pass"] % G == 0 and p["per_pass"] > 0
            covered = 0
            passes = []
            for w in range(p["workers"]):
                lo, hi = w * p["per_worker"], min((w + 1) * p["per_worker"], slots)
                assert lo < hi, (n, n_keys, slots, p)
                off = lo
                while off < hi:
                    passes.append((off, min(off + p["per_pass"], hi)))
                    off += p["per_pass"]
            assert [a for a, _ in passes] == p["pass_first"]
            for a, e in sorted(passes):
                assert a == covered and a % G == 0 and e % G == 0 and e > a       # (S is a multiple of 64)
                assert e - a <= p["ctx_capacity"], (n, n_keys, slots, p)
                covered = e
            assert covered == slots


def test_plan_probe_refuses_bad_arguments(pkg):
    for args in ((0, 1, 64), (10, 0, 64), (10, 257, 64), (10, 1, 0), (10, 1, 63), (10, 1, 128)):
        with pytest.raises(pkg.Bn254Error):
            pkg.dbg_plonk_keys_plan(*args)
